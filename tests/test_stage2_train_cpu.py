"""Host-side checks of stage-2 training: the schedule and the two parameter selections against what the reference's own classes
give (tests/golden/stage2_train.npz), the float64 restatements of SGD and Adam against torch.optim in float64, the optimizer's
state dict, the argument checks and the device-free queries of the library, and the refusals of the training mode.  Inputs and
restatements: tests/stage2_train_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import stage1_cases as sc
import stage2_train_cases as s2
from mpreid import _lib, ops


@pytest.fixture(scope="module")
def gold():
    return np.load(s2.GOLDEN)


class _Groups:
    """anything with param_groups"""

    def __init__(self, lrs):
        self.param_groups = [{"lr": lr} for lr in lrs]


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(s2.SCHEDULES))
def test_warmup_multistep_schedule_equals_the_reference(gold, name):
    """scheduler.step(epoch) for epochs 1 .. 100 on a torch optimizer, on a TensorOptimizer and on a bare object with param_groups:
    the learning rates of the reference's WarmupMultiStepLR to 1e-15 relative, the rate after construction included; the formula's
    restatement too; a second group keeps its own base rate"""
    from solver.lr_scheduler import WarmupMultiStepLR
    steps, gamma, factor, iters, method = s2.SCHEDULES[name]
    want, want0 = gold["lr_" + name], float(gold["lr0_" + name])
    p = torch.nn.Parameter(torch.zeros(1))
    makers = [lambda: torch.optim.Adam([{"params": [p], "lr": s2.SCHEDULE_BASE_LR}, {"params": [torch.nn.Parameter(torch.zeros(1))],
                                                                                     "lr": 2 * s2.SCHEDULE_BASE_LR}]),
              lambda: ops.TensorOptimizer([{"params": [torch.zeros(1)], "lr": s2.SCHEDULE_BASE_LR},
                                           {"params": [torch.zeros(1)], "lr": 2 * s2.SCHEDULE_BASE_LR}], "SGD"),
              lambda: _Groups([s2.SCHEDULE_BASE_LR, 2 * s2.SCHEDULE_BASE_LR])]
    for make in makers:
        opt = make()
        sched = WarmupMultiStepLR(opt, steps, gamma, factor, iters, method)
        assert abs(opt.param_groups[0]["lr"] / want0 - 1) <= 1e-15 and sched.last_epoch == 0
        got = []
        for epoch in range(1, s2.SCHEDULE_EPOCHS + 1):
            sched.step(epoch)
            got.append([g["lr"] for g in opt.param_groups])
            assert sched.get_last_lr() == got[-1]
        got = np.array(got)
        assert np.abs(got[:, 0] / want - 1).max() <= 1e-15
        assert np.abs(got[:, 1] / (2 * want) - 1).max() <= 1e-15
    mine = np.array([s2.schedule_f64(e, s2.SCHEDULE_BASE_LR, steps, gamma, factor, iters, method) for e in range(1, 101)])
    assert np.abs(mine / want - 1).max() <= 1e-15
    assert want[39] < want[38] or iters > 40      # the milestone at epoch 40 shows once the warm-up is over


def test_schedule_steps_and_refusals():
    from solver.lr_scheduler import WarmupMultiStepLR
    opt = _Groups([1.0])
    sched = WarmupMultiStepLR(opt, (2, 4), 0.5, 0.1, 0, "linear")
    seen = []
    for _ in range(5):
        sched.step()
        seen.append(opt.param_groups[0]["lr"])
    assert seen == [1.0, 0.5, 0.5, 0.25, 0.25]
    state = sched.state_dict()
    assert "optimizer" not in state and state["last_epoch"] == 5
    with pytest.raises(ValueError):
        WarmupMultiStepLR(_Groups([1.0]), (4, 2))
    with pytest.raises(ValueError):
        WarmupMultiStepLR(_Groups([1.0]), (2, 4), warmup_method="cosine")
    with pytest.raises(KeyError):
        WarmupMultiStepLR(_Groups([1.0]), (2, 4), last_epoch=3)


# ---- the selections -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(s2.SELECTIONS))
def test_stage2_parameter_selection_equals_the_reference(gold, name):
    """make_optimizer_2astage / make_optimizer_2bstage on the stand-in module: the groups' names in order, their learning rates
    and weight decays (1e-15 relative), the names left requiring grad and the centers' learning rate are the reference's"""
    from solver.make_optimizer_prompt import make_optimizer_2astage, make_optimizer_2bstage
    names, lr, wd, grad, center_lr = s2.run_selection(make_optimizer_2astage, make_optimizer_2bstage, name)
    assert names == gold[f"sel_{name}_names"].tolist()
    assert grad == gold[f"sel_{name}_grad"].tolist()
    assert np.abs(lr / gold[f"sel_{name}_lr"] - 1).max() <= 1e-15
    assert np.array_equal(wd, gold[f"sel_{name}_wd"])
    assert center_lr == float(gold[f"sel_{name}_center_lr"])
    # what the rules mean on this project's names
    by = dict(zip(names, zip(lr, wd)))
    assert not any("expert" in n or "text_encoder" in n or "prompt_learner" in n for n in names)
    base = 3e-4
    assert by["image_encoder.ln_post.bias"] == (2 * base, s2.SELECTION_WD_BIAS) and by["image_encoder.proj"] == (base, 5e-4)
    if name.startswith("2a"):
        assert {"classifier.weight", "cv_embed", "visual_prompt", "bottleneck_proj.bias"} <= set(names)
        assert by["classifier.weight"][0] == (2 * s2.SELECTION_SOLVER_BASE_LR if name.endswith("large_fc") else base)
    else:
        assert all(n.startswith("image_encoder.") for n in names) and any("gate" in n for n in names)


def test_large_fc_lr_reads_solver_base_lr_and_raises_without_it():
    from solver.make_optimizer_prompt import make_optimizer_2astage
    cfg = s2.selection_cfg(2, True)
    del cfg.SOLVER["BASE_LR"]
    model = s2.standin_module()
    center = torch.nn.Linear(1, 1)
    with pytest.raises(AttributeError, match="BASE_LR"):
        make_optimizer_2astage(cfg, model, center)


def test_stage2_config_defaults_are_the_reference_values():
    from config import cfg_base
    s = cfg_base.SOLVER.STAGE2
    assert (s.IMS_PER_BATCH, s.OPTIMIZER_NAME, s.MAX_EPOCHS, s.BASE_LR, s.LARGE_FC_LR, s.BIAS_LR_FACTOR) == (64, "Adam", 100, 3e-4, False, 1)
    assert (s.MOMENTUM, s.CENTER_LR, s.CENTER_LOSS_WEIGHT, s.WEIGHT_DECAY, s.WEIGHT_DECAY_BIAS) == (0.9, 0.5, 0.0005, 0.0005, 0.0005)
    assert (s.GAMMA, list(s.STEPS), s.WARMUP_FACTOR, s.WARMUP_ITERS, s.WARMUP_METHOD) == (0.1, [40, 70], 0.01, 500, "linear")
    assert (s.CHECKPOINT_PERIOD, s.LOG_PERIOD, s.EVAL_PERIOD, s.WARMUP_EPOCHS, s.LR_MIN) == (10, 100, 10, 5, 0.000016)
    assert cfg_base.SOLVER.SEED == 1234 and "EXP_SETTING" in cfg_base.DATASETS


# ---- the restatements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", s2.SGD_WD)
def test_sgd_restatement_equals_torch_optim_in_float64(wd):
    n = 257
    p0, _, _, _ = s2.opt_state(n, 1)
    grads = [s2.opt_state(n, 10 + s)[1] for s in range(5)]
    pw, buf = p0.astype(np.float64), np.zeros(n)
    pt = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=s2.SGD_LR, momentum=s2.SGD_MU, weight_decay=wd, foreach=False)
    for step, g in enumerate(grads, 1):
        pw, buf = s2.sgd_f64(pw, g, buf, step, s2.SGD_LR, s2.SGD_MU, wd)
        pt.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    assert sc.rel_l2(pw - p0, pt.detach().numpy() - p0) <= 1e-12
    # the line-by-line fp32 form stays within an ulp or two of float64 per step
    lp, lb = s2.sgd_lines(p0, grads[0], np.zeros(n), 1, s2.SGD_LR, s2.SGD_MU, wd)
    ep, _ = s2.sgd_f64(p0, grads[0], np.zeros(n), 1, sc.f32(s2.SGD_LR), sc.f32(s2.SGD_MU), sc.f32(wd))
    assert np.all(np.abs(lp - ep) <= 1.0 * sc.ulp32(ep))


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_restatement_equals_torch_optim_in_float64(decoupled):
    n, wd = 257, 5e-4
    p0 = s2.opt_state(n, 2)[0]
    grads = [s2.opt_state(n, 20 + s)[1] for s in range(5)]
    pw, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pt = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([pt], lr=sc.LR, betas=(sc.BETA1, sc.BETA2), eps=sc.EPS, weight_decay=wd, foreach=False)
    for step, g in enumerate(grads, 1):
        pw, m, v = sc.adam_f64(pw, g, m, v, step, sc.LR, sc.BETA1, sc.BETA2, sc.EPS, wd, decoupled)
        pt.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    assert sc.rel_l2(pw - p0, pt.detach().numpy() - p0) <= 1e-10


def test_float64_training_reference_is_deterministic_and_falls():
    """the float64 loop of the fused-step tests: the loss falls over ten steps under both optimizers, the never-bound parameters do
    not move, the unused SIE row receives no gradient, both bottlenecks' statistics move"""
    for algo in ("SGD", "Adam"):
        w = s2.train_f64(True, algo, s2.TRAIN["steps"])
        assert w["losses"][-1] < w["losses"][0] and np.isfinite(w["losses"]).all()
        head = s2.train_setup()["head"]
        for k in s2.NEVER_BOUND:
            assert np.array_equal(w["params"][k], head[k].astype(np.float64))
        assert not w["grads"]["cv_embed"][2].any() and w["grads"]["cv_embed"][3].any()
        for k in ("bottleneck", "bottleneck_proj"):
            assert not np.allclose(w["stats"][k + ".running_mean"], head[k + ".running_mean"])


# ---- the optimizer object -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["SGD", "Adam", "AdamW"])
def test_tensor_optimizer_state_dict_round_trips(algo):
    """param_groups and state in the shape of torch's optimizers; load_state_dict into a fresh optimizer gives the same
    state_dict back; a state of another algorithm or other groups is refused; a step without a device is an error, not a
    fallback; bind refuses a foreign tensor and a buffer of another size"""
    def make():
        a, b, c = torch.zeros(3), torch.zeros(2, 2), torch.zeros(5)
        return ops.TensorOptimizer([{"params": [a], "lr": 1e-3, "weight_decay": 0.1}, b, {"params": [c]}], algo, lr=3e-4,
                                   weight_decay=5e-4, momentum=0.9), (a, b, c)
    opt, (a, b, c) = make()
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 3e-4, 3e-4] and [g["weight_decay"] for g in opt.param_groups] == [0.1, 5e-4, 5e-4]
    assert ("momentum" in opt.param_groups[0]) == (algo == "SGD") and ("betas" in opt.param_groups[0]) == (algo != "SGD")
    keys = ("momentum_buffer",) if algo == "SGD" else ("exp_avg", "exp_avg_sq")
    sd = {"algo": algo, "param_groups": [dict({k: v for k, v in g.items() if k != "params"}, params=[i], lr=0.5 + i)
                                         for i, g in enumerate(opt.param_groups)],
          "state": {0: dict({k: torch.arange(3.0) + j for j, k in enumerate(keys)}, step=4),
                    2: dict({k: torch.arange(5.0) * (j + 2) for j, k in enumerate(keys)}, step=7)}}
    opt.load_state_dict(sd)
    out = opt.state_dict()
    assert out["algo"] == algo and [g["lr"] for g in out["param_groups"]] == [0.5, 1.5, 2.5]
    assert [g["params"] for g in out["param_groups"]] == [[0], [1], [2]] and sorted(out["state"]) == [0, 2]
    for i in (0, 2):
        assert out["state"][i]["step"] == sd["state"][i]["step"]
        for k in keys:
            assert torch.equal(out["state"][i][k], sd["state"][i][k]) and out["state"][i][k] is not sd["state"][i][k]
    other, _ = make()
    other.load_state_dict(out)
    again = other.state_dict()
    assert again["param_groups"] == out["param_groups"] and sorted(again["state"]) == [0, 2]
    assert all(torch.equal(again["state"][i][k], out["state"][i][k]) for i in (0, 2) for k in keys)
    with pytest.raises(ValueError):
        other.load_state_dict(dict(out, algo="Adam" if algo == "SGD" else "SGD"))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(out, param_groups=out["param_groups"][:2]))
    a.grad = torch.ones(3)
    with pytest.raises(RuntimeError):
        opt.step()
    opt.zero_grad()
    assert a.grad is None
    opt.step()                                      # nothing has a gradient: nothing to do, no device needed
    with pytest.raises(KeyError):
        opt.bind(torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError):
        ops.TensorOptimizer([a, a], algo)
    with pytest.raises(ValueError):
        ops.TensorOptimizer([a], "RMSprop")


# ---- the library's argument checks, without a device ------------------------------------------------------------------------------
def _entry(p=0x1000, g=0x2000, s1=0x3000, s2_=0x4000, n=16, hyper=0):
    return _lib.OptimEntry(p, g, s1, s2_, n, hyper, 0)


def _step(entries, classes=((1e-3, 0.0),), algo=_lib.OPTIM_ADAM, step=1, betas=(0.9, 0.999), eps=1e-8, mu=0.9, n_entries=None,
          n_classes=None):
    L = _lib.load()
    tab = (_lib.OptimEntry * max(len(entries), 1))(*entries) if entries is not None else None
    cls = (_lib.OptimClass * max(len(classes), 1))(*[_lib.OptimClass(a, b) for a, b in classes]) if classes is not None else None
    return L.mpreid_optim_step_multi_f32(tab, len(entries or ()) if n_entries is None else n_entries, cls,
                                         len(classes or ()) if n_classes is None else n_classes, algo, step, betas[0], betas[1], eps, mu,
                                         None)


def test_optimizer_table_errors_need_no_device():
    """every argument error of mpreid_optim_step_multi_f32 is MPREID_ERR_ARG with a message, found on the host before any HIP call: an
    empty or NULL table, a NULL or misaligned pointer (state2 only where the algorithm reads it), n < 1, a class index out of
    range, more than 8 classes, a non-finite or negative lr or weight decay, step < 1, an unknown algorithm, bad betas / eps /
    momentum -- also when the bad entry is the last of 200 good ones"""
    L = _lib.load()
    inf, nan = float("inf"), float("nan")
    bad = {
        "empty table": dict(entries=[]), "NULL table": dict(entries=None, n_entries=1), "NULL classes": dict(entries=[_entry()], classes=None, n_classes=1),
        "no class": dict(entries=[_entry()], classes=[]), "nine classes": dict(entries=[_entry()], classes=[(1e-3, 0.0)] * 9),
        "NULL param": dict(entries=[_entry(p=None)]), "NULL grad": dict(entries=[_entry(g=None)]), "NULL state1": dict(entries=[_entry(s1=None)]),
        "NULL state2 (Adam)": dict(entries=[_entry(s2_=None)]), "NULL state2 (AdamW)": dict(entries=[_entry(s2_=None)], algo=_lib.OPTIM_ADAMW),
        "misaligned": dict(entries=[_entry(g=0x2002)]), "n = 0": dict(entries=[_entry(n=0)]), "n < 0": dict(entries=[_entry(n=-4)]),
        "n = 2^38": dict(entries=[_entry(n=1 << 38)]),
        "class 1 of 1": dict(entries=[_entry(hyper=1)]), "class -1": dict(entries=[_entry(hyper=-1)]),
        "lr NaN": dict(entries=[_entry()], classes=[(nan, 0.0)]), "lr inf": dict(entries=[_entry()], classes=[(inf, 0.0)]),
        "lr < 0": dict(entries=[_entry()], classes=[(-1e-3, 0.0)]), "wd NaN": dict(entries=[_entry()], classes=[(1e-3, nan)]),
        "wd < 0": dict(entries=[_entry()], classes=[(1e-3, -0.1)]), "second class bad": dict(entries=[_entry()], classes=[(1e-3, 0.0), (1e-3, inf)]),
        "step 0": dict(entries=[_entry()], step=0), "step -1": dict(entries=[_entry()], step=-1), "algo 3": dict(entries=[_entry()], algo=3),
        "beta1 = 1": dict(entries=[_entry()], betas=(1.0, 0.999)), "eps = 0": dict(entries=[_entry()], eps=0.0),
        "momentum < 0": dict(entries=[_entry()], algo=_lib.OPTIM_SGD, mu=-0.1), "momentum NaN": dict(entries=[_entry()], algo=_lib.OPTIM_SGD, mu=nan),
        "the last of 201": dict(entries=[_entry() for _ in range(200)] + [_entry(n=0)]),
    }
    for what, kw in bad.items():
        assert _step(**kw) == _lib.ERR_ARG, what
        assert L.mpreid_last_error().decode(), what
    assert "entry 200" in L.mpreid_last_error().decode()


def test_absmax_table_errors_and_workspace_query_need_no_device():
    """mpreid_absmax_multi_f32: a NULL / empty table, a NULL or misaligned source, n < 1, a NULL output are MPREID_ERR_ARG, a NULL or
    short workspace MPREID_ERR_WORKSPACE, all before any HIP call; the workspace query is one float per chunk of 4096 elements,
    rounded up to 256 bytes, and 0 for a bad table; the launch count query: 64 tensors per launch"""
    L = _lib.load()

    def tab(*pairs):
        return (_lib.AbsmaxEntry * len(pairs))(*[_lib.AbsmaxEntry(a, n) for a, n in pairs])
    good = tab((0x1000, 5000), (0x8000, 1))
    assert L.mpreid_absmax_multi_workspace_bytes(good, 2) == 256
    assert L.mpreid_absmax_multi_workspace_bytes(tab((0x1000, 4096 * 64), (0x2000, 1)), 2) == 512
    assert L.mpreid_absmax_multi_workspace_bytes(tab((0x1000, 768 * 3072)), 1) == 576 * 4
    for t, n in ((None, 1), (good, 0), (tab((None, 4)), 1), (tab((0x1002, 4)), 1), (tab((0x1000, 0)), 1), (tab((0x1000, 4), (0x2000, -1)), 2)):
        assert L.mpreid_absmax_multi_workspace_bytes(t, n) == 0
        assert L.mpreid_absmax_multi_f32(t, n, ctypes.c_void_p(0x9000), ctypes.c_void_p(0x10000), 4096, None) == _lib.ERR_ARG
    assert L.mpreid_absmax_multi_f32(good, 2, None, ctypes.c_void_p(0x10000), 4096, None) == _lib.ERR_ARG
    assert L.mpreid_absmax_multi_f32(good, 2, ctypes.c_void_p(0x9000), None, 4096, None) == _lib.ERR_WORKSPACE
    assert L.mpreid_absmax_multi_f32(good, 2, ctypes.c_void_p(0x9000), ctypes.c_void_p(0x10000), 255, None) == _lib.ERR_WORKSPACE
    assert "workspace too small" in L.mpreid_last_error().decode()
    assert L.mpreid_absmax_multi_f32(good, 2, ctypes.c_void_p(0x9000), ctypes.c_void_p(0x10010), 4096, None) == _lib.ERR_ARG
    assert [L.mpreid_optim_step_launches(n) for n in (-1, 0, 1, 64, 65, 155, 200)] == [0, 0, 1, 1, 2, 3, 4]
    assert ops.optim_step_launches(155) <= 8
    assert (_lib.OPTIM_CHUNK, _lib.OPTIM_MAX_CLASSES, _lib.OPTIM_TENSORS_PER_LAUNCH) == (s2.CHUNK, 8, 64)
    assert ctypes.sizeof(_lib.OptimEntry) == 48 and ctypes.sizeof(_lib.OptimClass) == 8 and ctypes.sizeof(_lib.AbsmaxEntry) == 16


def test_python_wrappers_refuse_bad_tables_on_the_host():
    with pytest.raises(ValueError):
        ops.OptimTable([])
    with pytest.raises(ValueError):
        ops.OptimTable([(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), 0)])      # not on the device


# ---- the training mode's refusals -------------------------------------------------------------------------------------------------
def _small_cfg(*opts):
    from config import cfg_base
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["INPUT.SIZE_TRAIN", [32, 32], "INPUT.SIZE_TEST", [32, 32]] + list(opts))
    return cfg


@pytest.mark.parametrize("tower", ["moe", "rn50"])
def test_training_mode_refuses_moe_and_rn50(tower):
    """enable_stage2_training() and the training-mode forward of the Uni-Prompt model raise NotImplementedError that names what is
    missing, before a device is asked for"""
    from model import make_model_uniprompt as mu
    opts = (["MODEL.MOE.ENABLED", True, "MODEL.MOE.NUM_EXPERTS", 2, "MODEL.MOE.TOP_K", 1, "MODEL.MOE.MOE_LAYERS", 1] if tower == "moe"
            else ["MODEL.NAME", "RN50"])
    m = mu.make_model(_small_cfg(*opts), num_class=3, camera_num=1, view_num=1)
    word = "MoE tower has no backward" if tower == "moe" else "RN50 tower has no backward"
    with pytest.raises(NotImplementedError, match=word):
        m.enable_stage2_training()
    m.train()
    with pytest.raises(NotImplementedError, match=word):
        m(x=torch.zeros(2, 3, 32, 32), label=torch.zeros(2, dtype=torch.long))
    m.eval()


def test_training_mode_needs_enable_stage2_training_and_the_base_model_keeps_its_error():
    from model import make_model as mb
    from model import make_model_uniprompt as mu
    cfg = _small_cfg()
    m = mu.make_model(cfg, num_class=3, camera_num=1, view_num=1)
    m.train()
    with pytest.raises(NotImplementedError, match="enable_stage2_training"):
        m(x=torch.zeros(2, 3, 32, 32), label=torch.zeros(2, dtype=torch.long))
    with pytest.raises(RuntimeError, match="enable_stage2_training"):
        m.stage2_trainer(cfg, None, None)
    assert m.eval() is m and not m.training
    b = mb.make_model(cfg, num_class=3, camera_num=1, view_num=1)
    b.train()
    with pytest.raises(NotImplementedError, match="out of scope"):
        b(torch.zeros(2, 3, 32, 32))
