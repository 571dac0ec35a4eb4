"""Host-side checks of stage-1 prompt learning: the float64 restatements of tests/stage1_cases.py against what the
reference's own loss and scheduler gave (tests/golden/stage1.npz), the schedule and the torch form of the drop-in loss against
the same goldens, the workspace query and every argument error of the three entry points without a device, the batch slicing
of do_train_stage1, the config keys."""
import ctypes
import math

import numpy as np
import pytest
import torch

import stage1_cases as sc
from mpreid import _lib


@pytest.fixture(scope="module")
def gold():
    return np.load(sc.GOLDEN)


@pytest.mark.parametrize("case", sc.GOLDEN_SUPCON, ids=sc.case_key)
def test_restated_loss_and_gradients_equal_the_reference(gold, case):
    """loss: relative error <= 1e-12 (absolute below 1e-300: batch 1 gives 0); each gradient: relative L2 <= 1e-12"""
    key = sc.case_key(case)
    loss, d_txt, d_img = sc.supcon_want(*case)
    want = gold[key + "_loss"]
    assert np.all(np.abs(loss - want) <= 1e-12 * np.abs(want) + 1e-300), (loss, want)
    assert sc.rel_l2(d_txt, gold[key + "_dtxt"]) <= 1e-12 and sc.rel_l2(d_img, gold[key + "_dimg"]) <= 1e-12
    if case[0] == 1:
        assert not loss.any() and not d_txt.any() and not d_img.any()
    if case[3] == sc.SCALE_HOT:
        img, txt, _ = sc.supcon_case(*case)
        assert float((img.astype(np.float64) @ txt.astype(np.float64).T).max()) > sc.OVERFLOW_LOGIT
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(np.float32(sc.OVERFLOW_LOGIT)))     # what an unstabilised fp32 kernel would compute


def test_every_case_has_the_shape_and_labels_it_names():
    for b, d, pattern, scale in sc.supcon_cases():
        img, txt, lab = sc.supcon_case(b, d, pattern, scale)
        assert img.shape == txt.shape == (b, d) and img.dtype == np.float32 and lab.shape == (b,) and lab.dtype == np.int64
        n = len(set(lab.tolist()))
        assert n == (b if pattern == "distinct" else 1 if pattern == "equal" else n)
        if pattern == "groups" and b >= 63:
            sizes = sorted(np.unique(lab, return_counts=True)[1].tolist())
            assert sizes[0] == 1 and sizes[-1] >= 10       # unequal groups
    assert len(sc.supcon_cases()) == 7 * 3 * 3 + 7 * 3


def _fake_optimizer(lr):
    class Opt:
        param_groups = [{"lr": lr}, {"lr": lr}]
    return Opt()


@pytest.mark.parametrize("name,warmup_t", [("lr_default", 5), ("lr_nowarmup", 0)])
def test_schedule_equals_the_reference(gold, name, warmup_t):
    """the reference's solver package imports in the build container, so the goldens hold its _get_lr(epoch) for epochs 1..100;
    the restatement and the drop-in scheduler agree with them to 1e-15 relative"""
    from solver.scheduler_factory import create_scheduler
    assert int(gold["has_lr"]) == 1
    want = gold[name]
    s = dict(sc.SCHEDULE, warmup_t=warmup_t)
    opt = _fake_optimizer(s["base_lr"])
    sched = create_scheduler(opt, s["num_epochs"], s["lr_min"], s["warmup_lr_init"], s["warmup_t"])
    assert opt.param_groups[0]["lr"] == (s["warmup_lr_init"] if warmup_t else s["base_lr"])
    for epoch in range(1, 101):
        w = want[epoch - 1]
        assert abs(sc.schedule_f64(epoch, **s) - w) <= 1e-15 * abs(w), epoch
        got = sched._get_lr(epoch)
        assert len(got) == 2 and all(abs(g - w) <= 1e-15 * abs(w) for g in got), epoch
        sched.step(epoch)
        assert opt.param_groups[1]["lr"] == got[1]
    assert want[99] == s["lr_min"] and want[0] > want[98]
    with pytest.raises(NotImplementedError):
        create_scheduler(opt, 100, 0.0, 0.0, 0, noise_range=(0, 10))


def test_drop_in_loss_in_torch_form_equals_the_reference(gold):
    """host tensors, two different label vectors and a non-square batch take the torch formula: float64 in, the golden out"""
    from loss.supcontrast import SupConLoss
    xent = SupConLoss("cpu")
    for case in [c for c in sc.GOLDEN_SUPCON if c[1] == 64]:
        img, txt, lab = sc.supcon_case(*case)
        I, T, y = torch.from_numpy(img).double().requires_grad_(True), torch.from_numpy(txt).double().requires_grad_(True), torch.from_numpy(lab)
        l1, l2 = xent(I, T, y, y), xent(T, I, y, y)
        want = gold[sc.case_key(case) + "_loss"]
        assert abs(float(l1.detach()) - want[0]) <= 1e-12 * abs(want[0]) and abs(float(l2.detach()) - want[1]) <= 1e-12 * abs(want[1])
        d_txt, d_img = torch.autograd.grad(l1 + l2, [T, I])
        assert sc.rel_l2(d_txt.numpy(), gold[sc.case_key(case) + "_dtxt"]) <= 1e-12
        assert sc.rel_l2(d_img.numpy(), gold[sc.case_key(case) + "_dimg"]) <= 1e-12
    a, b = torch.randn(3, 8, dtype=torch.float64), torch.randn(5, 8, dtype=torch.float64)
    la, lb = torch.tensor([0, 1, 0]), torch.tensor([1, 0, 0, 2, 1])
    logp = torch.log_softmax(a @ b.T, 1)
    m = (la[:, None] == lb[None, :]).double()
    assert float(xent(a, b, la, lb)) == pytest.approx(float(-((m * logp).sum(1) / m.sum(1)).mean()), rel=1e-14)


def test_segment_sum_restatement_is_the_index_backward():
    """the sequential fp32 restatement equals, in float64 to rounding, autograd's gradient of ctx[idx] placed in its window"""
    for name, batch, tokens, width, tok0, n_tok, n_seg, idx in sc.segment_cases():
        src = sc.segment_src(batch, tokens, width)
        got = sc.segment_sum_f32(src, idx, tok0, n_tok, n_seg)
        ctx = torch.zeros(n_seg, n_tok, width, dtype=torch.float64, requires_grad=True)
        (ctx[torch.tensor(idx)] * torch.from_numpy(src[:, tok0:tok0 + n_tok]).double()).sum().backward()
        assert got.dtype == np.float32 and np.abs(got - ctx.grad.numpy()).max() <= 1e-5, name
        empty = [s for s in range(n_seg) if s not in idx]
        assert not got[empty].any()


def test_adam_restatement_equals_torch_in_float64():
    """both forms, with and without weight decay, three steps from a given state: torch.optim in float64 to 1e-13"""
    for decoupled in (False, True):
        for wd in sc.ADAM_WD:
            p0, g, m0, v0 = (t.astype(np.float64) for t in sc.adam_state(257, 3, False))
            p = torch.from_numpy(p0.copy()).requires_grad_(True)
            cls = torch.optim.AdamW if decoupled else torch.optim.Adam
            opt = cls([p], lr=sc.LR, betas=(sc.BETA1, sc.BETA2), eps=sc.EPS, weight_decay=wd, foreach=False)
            pw, mw, vw = p0, np.zeros_like(p0), np.zeros_like(p0)
            for step in (1, 2, 3):
                p.grad = torch.from_numpy(g * step)
                opt.step()
                pw, mw, vw = sc.adam_f64(pw, g * step, mw, vw, step, sc.LR, sc.BETA1, sc.BETA2, sc.EPS, wd, decoupled)
            assert sc.rel_l2(p.detach().numpy() - p0, pw - p0) <= 1e-13, (decoupled, wd)
            st = opt.state[p]
            assert sc.rel_l2(st["exp_avg"].numpy(), mw) <= 1e-13 and sc.rel_l2(st["exp_avg_sq"].numpy(), vw) <= 1e-13


def test_workspace_query_and_argument_errors_need_no_gpu():
    """mpreid_supcon_workspace_bytes needs no device and answers 0 for a bad request; every argument error of the three entry
    points is found before anything is launched, so it is reported on a machine without a device too"""
    L = _lib.load()
    assert L.mpreid_supcon_workspace_bytes(64, 512) >= 2 * 64 * 64 * 4
    assert L.mpreid_supcon_workspace_bytes(_lib.SUPCON_MAX_BATCH, 1) >= 2 * 1024 * 1024 * 4
    for bad in ((0, 8), (-1, 8), (_lib.SUPCON_MAX_BATCH + 1, 8), (8, 0), (8, -3)):
        assert L.mpreid_supcon_workspace_bytes(*bad) == 0, bad
    p, q, r, o, w = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000    # aligned dummies: nothing is dereferenced before the checks
    need = L.mpreid_supcon_workspace_bytes(8, 4)

    def supcon(img=p, txt=q, lab=r, B=8, D=4, loss=o, d_txt=o + 256, d_img=None, ws=w, ws_bytes=need):
        return L.mpreid_supcon_pair_f32(img, txt, lab, B, D, loss, d_txt, d_img, ws, ws_bytes, None)
    for kw in (dict(img=None), dict(txt=None), dict(lab=None), dict(loss=None), dict(B=0), dict(B=-2), dict(D=0), dict(img=p + 2),
               dict(lab=r + 4), dict(d_txt=o + 1), dict(d_img=o + 2), dict(ws=w + 128)):
        assert supcon(**kw) == _lib.ERR_ARG, kw
        assert b"bad argument" in L.mpreid_last_error()
    assert supcon(B=_lib.SUPCON_MAX_BATCH + 1) == _lib.ERR_UNSUPPORTED and b"MPREID_SUPCON_MAX_BATCH" in L.mpreid_last_error()
    assert supcon(ws=None) == _lib.ERR_WORKSPACE and supcon(ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert b"workspace too small" in L.mpreid_last_error()
    for dirs in (0, 4, -1):
        assert L.mpreid_supcon_f32(p, q, r, 8, 4, dirs, o, o + 256, None, w, need, None) == _lib.ERR_ARG

    def seg(src=p, idx=r, batch=7, tokens=21, width=128, tok0=1, n_tok=8, n_seg=6, out=o):
        return L.mpreid_rows_segment_sum_f32(src, idx, batch, tokens, width, tok0, n_tok, n_seg, out, None)
    for kw in (dict(src=None), dict(idx=None), dict(out=None), dict(batch=0), dict(tokens=0), dict(width=0), dict(n_seg=0), dict(tok0=-1),
               dict(n_tok=0), dict(tok0=14), dict(tok0=21, n_tok=1), dict(src=p + 1), dict(out=o + 2), dict(idx=r + 4),
               dict(tokens=1 << 20, width=1 << 10, n_tok=1 << 15)):
        assert seg(**kw) == _lib.ERR_ARG, kw

    def adam(param=p, grad=q, m=r, v=o, n=10, step=1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4, decoupled=0):
        return L.mpreid_adam_step_f32(param, grad, m, v, n, step, lr, b1, b2, eps, wd, decoupled, None)
    for kw in (dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-5), dict(step=0), dict(lr=-1.0),
               dict(lr=math.inf), dict(lr=math.nan), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=math.nan), dict(eps=0.0),
               dict(eps=-1e-8), dict(wd=-1.0), dict(wd=math.nan), dict(param=p + 2), dict(v=o + 1), dict(n=1 << 38)):
        assert adam(**kw) == _lib.ERR_ARG, kw
    assert ctypes.sizeof(ctypes.c_int64) == 8


def test_batch_slicing_skips_the_empty_last_batch():
    """the reference runs num_image // batch + 1 batches, the last one empty when the batch size divides the image count"""
    from processor.processor_uniprompt_stage1 import stage1_batches
    assert stage1_batches(128, 64) == [(0, 64), (64, 128)]
    assert stage1_batches(130, 64) == [(0, 64), (64, 128), (128, 130)]
    assert stage1_batches(3, 64) == [(0, 3)] and stage1_batches(0, 64) == []
    for n in range(0, 70):
        sl = stage1_batches(n, 8)
        assert all(hi > lo for lo, hi in sl) and sum(hi - lo for lo, hi in sl) == n
        assert len(sl) == n // 8 + (1 if n % 8 else 0)
    with pytest.raises(ValueError):
        stage1_batches(10, 0)


def test_config_carries_the_stage1_sections_of_the_reference():
    from config import cfg_base
    for sec in ("STAGE1", "STAGE1A", "STAGE1B"):
        s = cfg_base.SOLVER[sec]
        assert (s.IMS_PER_BATCH, s.OPTIMIZER_NAME, s.MAX_EPOCHS, s.BASE_LR, s.WEIGHT_DECAY) == (64, "Adam", 100, 3e-4, 0.0005)
        assert (s.WARMUP_EPOCHS, s.WARMUP_LR_INIT, s.LR_MIN, s.CHECKPOINT_PERIOD, s.LOG_PERIOD, s.MOMENTUM) == (5, 0.01, 0.000016, 10, 100, 0.9)
    assert sc.SCHEDULE == dict(base_lr=cfg_base.SOLVER.STAGE1A.BASE_LR, num_epochs=cfg_base.SOLVER.STAGE1A.MAX_EPOCHS,
                               lr_min=cfg_base.SOLVER.STAGE1A.LR_MIN, warmup_lr_init=cfg_base.SOLVER.STAGE1A.WARMUP_LR_INIT,
                               warmup_t=cfg_base.SOLVER.STAGE1A.WARMUP_EPOCHS)


def test_make_optimizer_falls_through_to_torch_for_host_tensors_and_other_names():
    """the library's Adam needs device tensors: host tensors, SGD and AdamW with amsgrad get torch.optim, as the reference does"""
    from config import cfg_base
    from solver.make_optimizer_prompt import make_optimizer_1stage

    class Learner:
        def __init__(self):
            self.t = [torch.zeros(2, 3, requires_grad=True), torch.zeros(2, 3)]

        def parameters(self):
            return iter(self.t)

    class Model:
        prompt_learner = Learner()
    cfg = cfg_base.clone()
    opt = make_optimizer_1stage(cfg, Model(), "STAGE1A")
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["weight_decay"] == 0.0005
    cfg.SOLVER.STAGE1B.OPTIMIZER_NAME = "SGD"
    assert isinstance(make_optimizer_1stage(cfg, Model(), "STAGE1B"), torch.optim.SGD)
    cfg.SOLVER.STAGE1B.OPTIMIZER_NAME = "AdamW"
    assert isinstance(make_optimizer_1stage(cfg, Model(), "STAGE1B"), torch.optim.AdamW)
    Model.prompt_learner.t[0].requires_grad_(False)
    with pytest.raises(ValueError):
        make_optimizer_1stage(cfg, Model(), "STAGE1A")
