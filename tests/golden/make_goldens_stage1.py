#!/usr/bin/env python3
"""Golden vectors of stage-1 prompt learning, from the REFERENCE's own loss and scheduler.

Run in the build container only (needs the reference, imported in place by file path; nothing of it is copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_stage1.py

Writes tests/golden/stage1.npz:
  <case>_loss, <case>_dtxt, <case>_dimg   for every case of stage1_cases.GOLDEN_SUPCON: loss/supcontrast.py::SupConLoss on the
                                          float64 copies of the case's seeded fp32 inputs, called as the stage-1 loop calls it
                                          (loss_i2t = xent(img, txt, y, y), loss_t2i = xent(txt, img, y, y)), and torch.autograd's
                                          gradients of loss_i2t + loss_t2i; all float64.  The inputs are regenerated from the seed.
  lr_default, lr_nowarmup                 solver/scheduler_factory.py::create_scheduler(...)._get_lr(epoch)[0] for epochs 1..100 at
                                          the SOLVER.STAGE1A defaults and at warmup_t = 0 (float64), when the reference's solver
                                          package imports here; has_lr says whether it did.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import stage1_cases as sc  # noqa: E402


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_supcon(out):
    xent = by_path("ref_supcontrast", "loss/supcontrast.py").SupConLoss("cpu")
    for case in sc.GOLDEN_SUPCON:
        img, txt, labels = sc.supcon_case(*case)
        I = torch.from_numpy(img).double().requires_grad_(True)
        T = torch.from_numpy(txt).double().requires_grad_(True)
        y = torch.from_numpy(labels)
        l_i2t, l_t2i = xent(I, T, y, y), xent(T, I, y, y)
        d_txt, d_img = torch.autograd.grad(l_i2t + l_t2i, [T, I])
        key = sc.case_key(case)
        out[key + "_loss"] = np.array([float(l_i2t), float(l_t2i)], np.float64)
        out[key + "_dtxt"], out[key + "_dimg"] = d_txt.numpy(), d_img.numpy()
        want = sc.supcon_f64(img, txt, labels)
        print(key, "restatement: loss", np.abs(want[0] - out[key + "_loss"]).max(), "d_txt", sc.rel_l2(want[1], d_txt.numpy()),
              "d_img", sc.rel_l2(want[2], d_img.numpy()))


def gen_schedule(out):
    try:
        sys.path.insert(0, REF)
        from solver.scheduler_factory import create_scheduler
    except Exception as e:   # the package pulls in what this container may not have: the test then restates the formula alone
        print("the reference's solver package does not import here:", repr(e))
        out["has_lr"] = np.array(0)
        return
    finally:
        sys.path.remove(REF)
    s = sc.SCHEDULE
    for name, warmup_t in (("lr_default", s["warmup_t"]), ("lr_nowarmup", 0)):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([{"params": [p], "lr": s["base_lr"]}])
        sched = create_scheduler(opt, num_epochs=s["num_epochs"], lr_min=s["lr_min"], warmup_lr_init=s["warmup_lr_init"],
                                 warmup_t=warmup_t, noise_range=None)
        out[name] = np.array([sched._get_lr(e)[0] for e in range(1, 101)], np.float64)
    out["has_lr"] = np.array(1)


if __name__ == "__main__":
    arrs = {}
    gen_supcon(arrs)
    gen_schedule(arrs)
    path = os.path.join(HERE, "stage1.npz")
    np.savez_compressed(path, **arrs)
    print("stage1.npz: %.0f KiB, %d arrays" % (os.path.getsize(path) / 1024, len(arrs)))
