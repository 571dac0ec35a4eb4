#!/usr/bin/env python3
"""Golden vectors of stage-2 training, from the REFERENCE's own scheduler and optimizer factories.

Needs a checkout of the reference, imported in place by file path (nothing of it is copied):

    MPREID_REFERENCE=<the reference's root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_stage2_train.py

Writes tests/golden/stage2_train.npz (data only):
  lr_<name>                       solver/lr_scheduler.py::WarmupMultiStepLR over one group of base lr 3e-4: the group's learning
                                  rate after scheduler.step(epoch) for epochs 1..100 (float64), for every entry of
                                  stage2_train_cases.SCHEDULES (the SOLVER.STAGE2 defaults, the constant warm-up, WARMUP_ITERS 0
                                  and 10); lr0_<name>: the rate right after construction
  sel_<name>_names / _lr / _wd    the groups solver/make_optimizer_prompt.py::make_optimizer_2astage / _2bstage build for the
                                  stand-in module of stage2_train_cases (this project's parameter names, 1-element tensors), for
                                  every entry of SELECTIONS (BIAS_LR_FACTOR 2, LARGE_FC_LR off and on); _grad: the names left
                                  requiring grad; _center_lr: the learning rate of optimizer_center
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MPREID_REFERENCE") or sys.exit("set MPREID_REFERENCE to the root of a checkout of the reference")
sys.dont_write_bytecode = True
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "mp-reid_amd")):
    sys.path.insert(0, p)
import stage2_train_cases as s2  # noqa: E402


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_schedules(out):
    cls = by_path("ref_lr_scheduler", "solver/lr_scheduler.py").WarmupMultiStepLR
    for name, (steps, gamma, factor, iters, method) in s2.SCHEDULES.items():
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([{"params": [p], "lr": s2.SCHEDULE_BASE_LR}])
        sched = cls(opt, steps, gamma, factor, iters, method)
        out["lr0_" + name] = np.float64(opt.param_groups[0]["lr"])
        lrs = []
        for epoch in range(1, s2.SCHEDULE_EPOCHS + 1):
            sched.step(epoch)
            lrs.append(opt.param_groups[0]["lr"])
        out["lr_" + name] = np.array(lrs, np.float64)
        want = [s2.schedule_f64(e, s2.SCHEDULE_BASE_LR, steps, gamma, factor, iters, method) for e in range(1, s2.SCHEDULE_EPOCHS + 1)]
        print(name, "restatement:", np.abs(np.array(want) / out["lr_" + name] - 1).max())


def gen_selections(out):
    ref = by_path("ref_make_optimizer_prompt", "solver/make_optimizer_prompt.py")
    for name in s2.SELECTIONS:
        names, lr, wd, grad, center_lr = s2.run_selection(ref.make_optimizer_2astage, ref.make_optimizer_2bstage, name)
        out[f"sel_{name}_names"], out[f"sel_{name}_lr"], out[f"sel_{name}_wd"] = np.array(names), lr, wd
        out[f"sel_{name}_grad"], out[f"sel_{name}_center_lr"] = np.array(grad), np.float64(center_lr)
        print(name, len(names), "groups,", len(grad), "names require grad")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    arrs = {}
    gen_schedules(arrs)
    gen_selections(arrs)
    path = os.path.join(HERE, "stage2_train.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")
