#!/usr/bin/env python3
"""Golden vectors of the stage-2 head's losses, from the REFERENCE's own loss classes.

Run in the build container only (needs the reference, imported in place by file path; nothing of it is copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_stage2_head.py

Writes tests/golden/stage2_head.npz:
  xent_<case>_loss, xent_<case>_grad      for every case of stage2_head_cases.GOLDEN_XENT: loss/softmax_loss.py::
                                          CrossEntropyLabelSmooth(classes, epsilon, use_gpu=False) on the float64 copy of the case's
                                          seeded fp32 logits, and torch.autograd's gradient (up to GRAD_MAX elements); float64.  (The reference builds its
                                          targets in fp32: they carry fp32's rounding of epsilon / classes.)
  tri_<case>_loss, _ap, _an, _grad        for every case of GOLDEN_TRIPLET (equal group sizes: the reference answers no others):
                                          loss/triplet_loss.py::TripletLoss(margin) or TripletLoss() on the float64 features, its
                                          dist_ap and dist_an, and the gradient of the loss (up to GRAD_MAX elements); float64.
The inputs are regenerated from the seed.  The reference's triplet_loss.py begins with `from turtle import pd`, which needs
tkinter; a stand-in module named turtle is placed into sys.modules before the import.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MPREID_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import stage2_head_cases as hc  # noqa: E402

GRAD_MAX = 4500   # a gradient of more elements is not stored (the file stays far below 1 MiB); its loss and distances are stored


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_xent(out):
    ref = by_path("ref_softmax_loss", "loss/softmax_loss.py")
    for case in hc.GOLDEN_XENT:
        rows, classes, eps, _ = case
        logits, labels = hc.xent_case(*case)
        x = torch.from_numpy(logits).double().requires_grad_(True)
        loss = ref.CrossEntropyLabelSmooth(classes, epsilon=eps, use_gpu=False)(x, torch.from_numpy(labels))
        (g,) = torch.autograd.grad(loss, [x])
        key = "xent_" + hc.xent_key(case)
        out[key + "_loss"] = np.array(float(loss))
        if g.numel() <= GRAD_MAX:
            out[key + "_grad"] = g.numpy()
        want = hc.xent_f64(logits, labels, eps)
        print(key, "restatement: loss", abs(want[0] - float(loss)), "grad", hc.rel_l2(want[1], g.numpy()))


def gen_triplet(out):
    stand_in = types.ModuleType("turtle")
    stand_in.pd = None
    sys.modules.setdefault("turtle", stand_in)
    ref = by_path("ref_triplet_loss", "loss/triplet_loss.py")
    for case in hc.GOLDEN_TRIPLET:
        x, y = hc.triplet_case(*case)
        X = torch.from_numpy(x).double().requires_grad_(True)
        crit = ref.TripletLoss() if case[2] is None else ref.TripletLoss(case[2])
        loss, ap, an = crit(X, torch.from_numpy(y))
        (g,) = torch.autograd.grad(loss, [X])
        key = "tri_" + hc.triplet_key(case)
        out[key + "_loss"] = np.array(float(loss))
        if g.numel() <= GRAD_MAX:
            out[key + "_grad"] = g.numpy()
        out[key + "_ap"], out[key + "_an"] = ap.detach().numpy(), an.detach().numpy()
        want = hc.triplet_f64(x, y, case[2])
        print(key, "restatement: loss", abs(want[0] - float(loss)), "grad", hc.rel_l2(want[1], g.numpy()),
              "ap", np.abs(want[2] - out[key + "_ap"]).max(), "an", np.abs(want[3] - out[key + "_an"]).max())


if __name__ == "__main__":
    arrs = {}
    gen_xent(arrs)
    gen_triplet(arrs)
    path = os.path.join(HERE, "stage2_head.npz")
    np.savez_compressed(path, **arrs)
    print("stage2_head.npz: %.0f KiB, %d arrays" % (os.path.getsize(path) / 1024, len(arrs)))
