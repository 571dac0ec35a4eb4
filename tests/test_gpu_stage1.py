"""Stage-1 prompt learning on the GPU (csrc/prompt_train.hip through mpreid.ops and the drop-in modules): the loss pair and its
gradients against float64, their memory discipline and run-to-run bits; the context gradient as a segment sum, bit for bit;
the Adam / AdamW step against float64 and against torch.optim; the fused PromptTrainer step against the autograd step, on a
reduced tower and through do_train_stage1 on the Uni-Prompt model with its checkpoint round trip; a run that learns; limits
and errors.  Inputs and float64 oracles: tests/stage1_cases.py."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import stage1_cases as sc
import text_cases as tc
import text_grad_cases as tg
from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345   # a NaN pattern


def _guarded(shape, guard=64):
    """(whole int32 buffer of sentinels, the fp32 view of `shape` in its middle, a function that says the guards are intact)"""
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    view = buf[guard:guard + n].view(torch.float32).view(*shape)

    def intact():
        return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())
    return buf, view, intact


def _nan_tail(a, rows=8):
    """the array on the device followed by NaN guard rows in the same allocation -> (the view of the data, the guard rows)"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0] + rows,) + tuple(a.shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = a.cuda()
    return buf[:a.shape[0]], buf[a.shape[0]:]


# ---- 1. loss and gradients against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.supcon_cases(), ids=sc.case_key)
def test_loss_and_gradients_against_float64(case):
    """relative L2 of d_txt and of d_img <= 2e-5, relative error of each loss <= 2e-5 (the project's split-mode bar); batch 1
    gives exact zeros; everything finite.  The fp32 autograd figure of the host is printed beside each.
    Largest figures measured on an MI355X over the 84 cases: loss 9.2e-6 (batch 2, dim 64, distinct labels, scale 3: a loss of 0.05
    from logits of 147; the host's fp32 autograd: 4.9e-6), d_txt 2.7e-6 and d_img 2.7e-6 (batch 63, dim 64, groups, scale 3; the
    host: the same 2.6e-6 and 2.7e-6); at scale 0.6 the losses stay below 3.8e-6 and the gradients below 2.5e-6."""
    batch, dim, pattern, scale = case
    img, txt, labels = sc.supcon_case(*case)
    want_loss, want_dtxt, want_dimg = sc.supcon_want(*case)
    loss, d_txt, d_img = ops.supcon_pair(torch.from_numpy(img).cuda(), torch.from_numpy(txt).cuda(), torch.from_numpy(labels).cuda(),
                                         need_d_img=True)
    loss, d_txt, d_img = loss.cpu().numpy(), d_txt.cpu().numpy(), d_img.cpu().numpy()
    assert np.isfinite(loss).all() and np.isfinite(d_txt).all() and np.isfinite(d_img).all()
    if batch == 1:
        assert not loss.any() and not d_txt.any() and not d_img.any()
        return
    host = sc.supcon_torch(img, txt, labels, torch.float32)

    def figures(l, dt, di):
        return (float(np.max(np.abs(l - want_loss) / np.abs(want_loss))), sc.rel_l2(dt, want_dtxt), sc.rel_l2(di, want_dimg))
    fig, hfig = figures(loss, d_txt, d_img), figures(*host)
    print("supcon %s: loss %.3e d_txt %.3e d_img %.3e; fp32 autograd on the host %.3e %.3e %.3e" % ((sc.case_key(case),) + fig + hfig))
    assert max(fig) <= sc.BOUND, fig


# ---- 2. memory discipline and bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(65, 64, "groups", sc.SCALE), (3, 4, "distinct", sc.SCALE), (257, 512, "groups", sc.SCALE)],
                         ids=sc.case_key)
def test_loss_writes_its_outputs_and_nothing_else(case):
    """NaN guard rows behind img and txt, sentinel guards around loss, d_txt and d_img: every output element written, no guard
    touched; with d_img NULL the other outputs keep their bits; a second call gives the same bits"""
    img, txt, labels = sc.supcon_case(*case)
    want = sc.supcon_want(*case)
    B, D = img.shape
    I, gi = _nan_tail(img)
    T, gt = _nan_tail(txt)
    y = torch.from_numpy(labels).cuda()
    (_, loss, ok_l), (_, d_txt, ok_t), (_, d_img, ok_i) = _guarded((2,)), _guarded((B, D)), _guarded((B, D))
    ops.supcon_pair(I, T, y, need_d_img=True, loss=loss, d_txt=d_txt, d_img=d_img)
    torch.cuda.synchronize()
    assert ok_l() and ok_t() and ok_i() and bool(torch.isnan(gi).all()) and bool(torch.isnan(gt).all())
    for t in (loss, d_txt, d_img):
        assert bool(torch.isfinite(t).all())      # none keeps the sentinel's NaN
    assert sc.rel_l2(d_txt.cpu().numpy(), want[1]) <= sc.BOUND and sc.rel_l2(d_img.cpu().numpy(), want[2]) <= sc.BOUND
    (_, loss2, ok_l2), (_, d_txt2, ok_t2) = _guarded((2,)), _guarded((B, D))
    out = ops.supcon_pair(I, T, y, loss=loss2, d_txt=d_txt2)
    torch.cuda.synchronize()
    assert len(out) == 2 and ok_l2() and ok_t2()
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(d_txt2.view(torch.int32), d_txt.view(torch.int32))
    again = ops.supcon_pair(I, T, y, need_d_img=True)
    for a, b in zip(again, (loss, d_txt, d_img)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # one direction at a time: the two gradients add up to the pair's (to rounding), the losses are the pair's own bits
    parts = [ops.supcon_pair(I, T, y, need_d_img=True, directions=d) for d in (1, 2)]
    for p in parts:
        assert torch.equal(p[0].view(torch.int32), loss.view(torch.int32))
    assert sc.rel_l2((parts[0][1].double() + parts[1][1].double()).cpu().numpy(), want[1]) <= sc.BOUND
    assert sc.rel_l2((parts[0][2].double() + parts[1][2].double()).cpu().numpy(), want[2]) <= sc.BOUND


def test_drop_in_loss_is_the_kernel_with_its_gradients():
    """loss/supcontrast.py on device tensors: each direction's value and autograd gradients against float64 autograd of that
    direction alone; the sum of the two calls is the pair"""
    from loss.supcontrast import SupConLoss
    case = (64, 64, "groups", sc.SCALE)
    img, txt, labels = sc.supcon_case(*case)
    want = sc.supcon_want(*case)
    xent = SupConLoss("cuda")
    I, T = torch.from_numpy(img).cuda().requires_grad_(True), torch.from_numpy(txt).cuda().requires_grad_(True)
    y = torch.from_numpy(labels).cuda()
    l_i2t, l_t2i = xent(I, T, y, y), xent(T, I, y.clone(), y)
    assert l_i2t.grad_fn is not None and type(l_i2t.grad_fn).__name__.startswith("_SupConRows")
    assert abs(float(l_i2t.detach()) - want[0][0]) <= sc.BOUND * want[0][0]
    assert abs(float(l_t2i.detach()) - want[0][1]) <= sc.BOUND * want[0][1]
    I64, T64 = torch.from_numpy(img).double().requires_grad_(True), torch.from_numpy(txt).double().requires_grad_(True)
    one = tg.contrastive(I64, T64, torch.from_numpy(labels), torch.from_numpy(labels))
    w_i, w_t = torch.autograd.grad(one, [I64, T64])
    g_i, g_t = torch.autograd.grad(l_i2t, [I, T], retain_graph=True)
    assert tc.rel_l2(g_i, w_i) <= sc.BOUND and tc.rel_l2(g_t, w_t) <= sc.BOUND
    (l_i2t + l_t2i).backward()
    assert sc.rel_l2(T.grad.cpu().numpy(), want[1]) <= sc.BOUND and sc.rel_l2(I.grad.cpu().numpy(), want[2]) <= sc.BOUND
    # another label vector on one side: the torch formula on the device, same numbers
    other = y.clone()
    other[0] = other[0] + 1000
    mixed = xent(I.detach(), T.detach(), y, other)
    ref = tg.contrastive(I64.detach(), T64.detach(), torch.from_numpy(labels), other.cpu())
    assert mixed.is_cuda and abs(float(mixed) - float(ref)) <= 1e-5 * abs(float(ref))


# ---- 3. rows_segment_sum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.segment_cases(), ids=lambda c: c[0])
def test_segment_sum_is_bit_equal_to_the_sequential_restatement(case):
    name, batch, tokens, width, tok0, n_tok, n_seg, idx = case
    src = sc.segment_src(batch, tokens, width)
    want = sc.segment_sum_f32(src, idx, tok0, n_tok, n_seg)
    S, guard = _nan_tail(src, rows=2)
    _, out, intact = _guarded((n_seg, n_tok, width))
    got = ops.rows_segment_sum(S, torch.tensor(idx, dtype=torch.int64).cuda(), tok0, n_tok, n_seg, out=out)
    torch.cuda.synchronize()
    assert got is out and intact() and bool(torch.isnan(guard).all())
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    empty = [s for s in range(n_seg) if s not in idx]
    assert bool((out[empty] == 0.0).all())
    again = ops.rows_segment_sum(S, torch.tensor(idx, dtype=torch.int64).cuda(), tok0, n_tok, n_seg)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    if width % 4 == 0 and n_seg * n_tok * width > 1:
        # a destination that is not 16-byte aligned takes the one-element path: the same bits
        buf = torch.full((n_seg * n_tok * width + 2,), float("nan"), dtype=torch.float32, device="cuda")
        odd = buf[1:-1].view(n_seg, n_tok, width)
        ops.rows_segment_sum(S, torch.tensor(idx, dtype=torch.int64).cuda(), tok0, n_tok, n_seg, out=odd)
        assert torch.equal(odd.view(torch.int32), out.view(torch.int32)) and bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))


# ---- 4. adam_step ---------------------------------------------------------------------------------------------------------------
def _adam_call(p, g, m, v, step, wd, decoupled, guard=True):
    """one adam_step on guarded device copies -> (p, m, v) as float32 numpy; the gradient buffer must keep its bits"""
    bufs = []
    for a in (p, m, v):
        _, view, intact = _guarded((a.size,))
        view.copy_(torch.from_numpy(a))
        bufs.append((view, intact))
    gd = torch.from_numpy(g).cuda()
    ops.adam_step(bufs[0][0], gd, bufs[1][0], bufs[2][0], step, sc.LR, (sc.BETA1, sc.BETA2), sc.EPS, wd, decoupled)
    torch.cuda.synchronize()
    assert all(intact() for _, intact in bufs) and np.array_equal(gd.cpu().numpy(), g)
    return tuple(view.cpu().numpy() for view, _ in bufs)


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("wd", sc.ADAM_WD)
@pytest.mark.parametrize("step", sc.ADAM_STEPS)
@pytest.mark.parametrize("n", sc.ADAM_N)
def test_adam_one_step_against_float64(n, step, wd, decoupled):
    """one step from given fp32 states (exp_avg carries the gradient's sign: no term cancels, so the count of roundings bounds
    the error) against float64 with the hyperparameters as the C ABI receives them:
    |dp| <= 1 ulp(p) + 16 * 2^-24 * |update|, exp_avg and exp_avg_sq within 4 ulp.  The roundings of the stated order: fmaf(-lw, p, p) or
    fmaf(wd, p, grad), g - m, the fmaf of m; g * g, beta2 * v, the fmaf of v; sqrt, / r, + eps, m / denominator, the four
    host-rounded constants, the closing fmaf -- twelve on the update, at most one ulp of p itself."""
    p, g, m, v = sc.adam_state(n, step, same_sign=True)
    hp = (sc.f32(sc.LR), sc.f32(sc.BETA1), sc.f32(sc.BETA2), sc.f32(sc.EPS), sc.f32(wd))
    pw, mw, vw = sc.adam_f64(p, g, m, v, step, *hp, decoupled)
    pg, mg, vg = _adam_call(p, g, m, v, step, wd, decoupled)
    base = p.astype(np.float64) * (1.0 - hp[0] * hp[4]) if decoupled else p.astype(np.float64)
    update = np.abs(pw - base)
    ulp_p = sc.ulp32(np.maximum(np.abs(p), np.abs(pw)))       # (of the larger of the parameter before and after the step)
    assert np.all(np.abs(pg - pw) <= ulp_p + 16 * 2.0 ** -24 * update), float(np.max(np.abs(pg - pw) / ulp_p))
    assert np.all(np.abs(mg - mw) <= 4 * sc.ulp32(mw)) and np.all(np.abs(vg - vw) <= 4 * sc.ulp32(vw))
    assert float(update.max()) > 0


def test_adam_zero_gradient_on_zero_state_leaves_the_parameters():
    p = sc.adam_state(257, 0, False)[0]
    z = np.zeros_like(p)
    pg, mg, vg = _adam_call(p, z, z.copy(), z.copy(), 1, 0.0, False)
    assert np.array_equal(pg.view(np.int32), p.view(np.int32)) and not mg.any() and not vg.any()


def test_adam_unaligned_buffers_take_the_one_element_path_with_the_same_bits():
    n = 259
    p, g, m, v = sc.adam_state(n, 7, False)
    want = _adam_call(p, g, m, v, 3, 5e-4, False)
    dev = []
    for a in (p, g, m, v):
        buf = torch.full((n + 2,), float("nan"), dtype=torch.float32, device="cuda")
        buf[1:-1] = torch.from_numpy(a).cuda()
        dev.append(buf)
    ops.adam_step(dev[0][1:-1], dev[1][1:-1], dev[2][1:-1], dev[3][1:-1], 3, sc.LR, (sc.BETA1, sc.BETA2), sc.EPS, 5e-4, False)
    for buf, w in zip((dev[0], dev[2], dev[3]), want):
        assert np.array_equal(buf[1:-1].cpu().numpy().view(np.int32), w.view(np.int32))
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_twenty_steps_against_torch_optim(decoupled):
    """twenty steps with a fresh seeded gradient each: the relative L2 distance of the parameters' total update from the float64
    run is at most 4x that of torch.optim.Adam / AdamW in fp32 on the host (foreach=False) from the same float64 run; the
    factor allows for a different but equally valid rounding order.  Both figures are printed.  Measured on an MI355X: Adam
    1.43e-6 (the host 1.43e-6), AdamW 6.8e-6 (the host 1.14e-5: it rounds 1 - lr * weight_decay to fp32)."""
    n, wd = 8 * 512 * 6, 5e-4
    hp = (sc.f32(sc.LR), sc.f32(sc.BETA1), sc.f32(sc.BETA2), sc.f32(sc.EPS), sc.f32(wd))
    p0 = sc.adam_state(n, 99, False)[0]
    grads = [sc.adam_state(n, 100 + s, False)[1] for s in range(20)]
    pw, mw, vw = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    ph = torch.from_numpy(p0.copy()).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([ph], lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4], foreach=False)
    pd = torch.from_numpy(p0.copy()).cuda()
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    for s, g in enumerate(grads, 1):
        pw, mw, vw = sc.adam_f64(pw, g, mw, vw, s, *hp, decoupled)
        ph.grad = torch.from_numpy(g.copy())
        opt.step()
        ops.adam_step(pd, torch.from_numpy(g).cuda(), md, vd, s, sc.LR, (sc.BETA1, sc.BETA2), sc.EPS, wd, decoupled)
    want = pw - p0
    fig = sc.rel_l2(pd.cpu().numpy().astype(np.float64) - p0, want)
    host = sc.rel_l2(ph.detach().numpy().astype(np.float64) - p0, want)
    print("adam twenty steps (%s): %.3e against float64; torch.optim in fp32 on the host %.3e" % ("AdamW" if decoupled else "Adam", fig, host))
    assert fig <= 4 * host


# ---- 5. the fused step equals the autograd step -----------------------------------------------------------------------------------
def _learner(tensors):
    from model.make_model_uniprompt import PromptLearner
    pl = PromptLearner()
    pl.set_tensors(tensors, "cuda")
    return pl


@pytest.fixture(scope="module")
def reduced_tower():
    sd = synth.text_state_dict(tc.REDUCED, seed=61)
    return sd, ops.TextEncoder(tc.REDUCED, sd, ws_tag="stage1_reduced")


@pytest.mark.parametrize("stage", ["1a", "1b"])
def test_fused_step_equals_the_autograd_step(reduced_tower, stage):
    """one PromptTrainer.step against TextEncoder.forward_grad + the torch loss + torch.optim.Adam from the same state: the
    context gradients agree to 2e-5 relative L2, the update is Adam's of the trainer's own gradient (the bound of the one-step
    test), the untrained context tensors keep their bits, the returned losses are those before the update.  Measured on an
    MI355X: ctx_generic 6.6e-7, ctx_modality 6.5e-7, ctx_platform 6.3e-7."""
    sd, enc = reduced_tower
    cfg = tc.REDUCED
    tensors = tc.prompt_learner_tensors(6, seed=62, tokens=cfg["tokens"], dim=cfg["width"])
    label = torch.tensor([3, 0, 5, 5, 1, 3, 5, 0])
    view = torch.tensor([0, 5, 6, 11, 12, 13, 7, 12])      # both sides of 6, 12 and 13
    g = torch.Generator().manual_seed(63)
    img = torch.randn(8, cfg["out_dim"], generator=g) * 0.5
    eot, lr, wd = 19, 1e-3, 5e-4
    names = ("ctx_generic",) if stage == "1a" else ("ctx_modality", "ctx_platform")
    frozen = [k for k in ("ctx_generic", "ctx_modality", "ctx_platform") if k not in names]

    # the autograd step
    t = {k: v.clone() for k, v in tensors.items()}      # host leaves: the assembled prompts are copied to the device under autograd
    for k in names:
        t[k].requires_grad_(True)
    prompts = tc.assemble_prompts(t, label, stage, view if stage == "1b" else None).cuda()
    feats = enc.forward_grad(prompts, [eot] * 8)
    loss = tg.contrastive(img.cuda(), feats, label.cuda(), label.cuda()), tg.contrastive(feats, img.cuda(), label.cuda(), label.cuda())
    (loss[0] + loss[1]).backward()
    want_grad = {k: t[k].grad.clone() for k in names}
    torch.optim.Adam([t[k] for k in names], lr=lr, weight_decay=wd, foreach=False).step()

    # the fused step
    pl = _learner(tensors)
    pl.set_training_stage(stage)
    before = {k: getattr(pl, k).clone() for k in ("ctx_generic", "ctx_modality", "ctx_platform")}
    trainer = ops.PromptTrainer(enc, pl, stage, eot=eot, lr=lr, weight_decay=wd)
    got_loss = trainer.step(img.cuda(), label.cuda(), views=view.cuda() if stage == "1b" else None).clone()
    loss = [float(v.detach()) for v in loss]
    assert abs(float(got_loss[0]) - loss[0]) <= sc.BOUND * abs(loss[0]) and abs(float(got_loss[1]) - loss[1]) <= sc.BOUND * abs(loss[1])
    hp = (sc.f32(lr), sc.f32(sc.BETA1), sc.f32(sc.BETA2), sc.f32(sc.EPS), sc.f32(wd))
    for k in names:
        fig = tc.rel_l2(trainer.grads[k], want_grad[k])
        print("stage %s fused step: %s gradient rel L2 %.3e against the autograd step" % (stage, k, fig))
        assert fig <= sc.BOUND, k
        p0, gk = before[k].cpu().numpy().ravel(), trainer.grads[k].cpu().numpy().ravel()
        pw, _, _ = sc.adam_f64(p0, gk, np.zeros_like(p0), np.zeros_like(p0), 1, *hp, False)
        pg = getattr(pl, k).detach().cpu().numpy().ravel()
        assert np.all(np.abs(pg - pw) <= sc.ulp32(np.maximum(np.abs(p0), np.abs(pw))) + 16 * 2.0 ** -24 * np.abs(pw - p0)), k
        assert not np.array_equal(pg, p0)
        # the two paths moved the tensor the same way: all but a sliver of the elements (those whose gradient is within
        # rounding of zero, where Adam's g / (|g| + eps) is steep) agree to a thousandth of the step
        close = (getattr(pl, k).detach().cpu() - t[k].detach()).abs() <= 1e-3 * lr
        assert float(close.float().mean()) >= 0.99, k
    for k in frozen:
        assert torch.equal(getattr(pl, k), before[k]), k
    if stage == "1a":
        unused = [c for c in range(6) if c not in label.tolist()]
        assert bool((trainer.grads["ctx_generic"][unused] == 0.0).all())
    # a second step continues from the optimizer's state; 1b without views is refused, so is a learner in the other stage
    trainer.step(img.cuda(), label.cuda(), views=view.cuda() if stage == "1b" else None)
    assert trainer.optimizer.state[id(getattr(pl, names[0]))]["step"] == 2
    if stage == "1b":
        with pytest.raises(ValueError):
            trainer.step(img.cuda(), label.cuda())
    pl.set_training_stage("1b" if stage == "1a" else "1a")
    with pytest.raises(ValueError):
        trainer.step(img.cuda(), label.cuda(), views=view.cuda())


class _Loader:
    """three batches of four (img, vid, target_cam, target_view), seeded"""

    def __init__(self, hw, n=12, batch=4):
        g = torch.Generator().manual_seed(71)
        self.img = torch.randn(n, 3, *hw, generator=g)
        self.vid = torch.tensor([3, 0, 6, 6, 1, 3, 2, 0, 6, 1, 5, 3])
        self.view = torch.tensor([0, 6, 11, 12, 13, 5, 7, 12, 0, 13, 6, 11])
        self.batch = batch

    def __iter__(self):
        for s in range(0, len(self.vid), self.batch):
            e = s + self.batch
            yield self.img[s:e], self.vid[s:e], torch.zeros(self.batch, dtype=torch.int64), self.view[s:e]


def _stage1_model(out_dir):
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.OUTPUT_DIR = str(out_dir)
    for sec in ("STAGE1", "STAGE1A", "STAGE1B"):
        cfg.SOLVER[sec].update(IMS_PER_BATCH=4, MAX_EPOCHS=1, CHECKPOINT_PERIOD=1, LOG_PERIOD=1)
    m = mu.make_model(cfg, num_class=7, camera_num=6, view_num=1)
    m.eval()
    return cfg, m


def test_do_train_stage1_fused_equals_autograd_and_checkpoint_round_trip(tmp_path, caplog):
    """the Uni-Prompt model at CLIP size, stage 1a and then stage 1b, each one epoch of three batches of four through
    do_train_stage1: with the library's Adam (the fused step) and with torch.optim.Adam (the autograd step) from the same state
    and the same permutation the trained tensors move the same way (all but a sliver of the elements to a thousandth of the
    three steps), the others keep their bits; the checkpoint the loop wrote goes through load_param to the same get_text bits"""
    from processor.processor_uniprompt_stage1 import do_train_stage1
    from solver.make_optimizer_prompt import make_optimizer_1stage
    from solver.scheduler_factory import create_scheduler
    cfg, m = _stage1_model(tmp_path)
    pl = m.prompt_learner
    keys = ("ctx_generic", "ctx_modality", "ctx_platform")
    loader = _Loader(tuple(cfg.INPUT.SIZE_TEST))
    label, view = loader.vid.cuda(), loader.view.cuda()
    for stage in ("1a", "1b"):
        sec = "STAGE1B" if stage == "1b" else "STAGE1A"
        (m.enable_stage1b_training if stage == "1b" else m.enable_stage1a_training)()
        names = ("ctx_generic",) if stage == "1a" else ("ctx_modality", "ctx_platform")
        start = {k: getattr(pl, k).detach().clone() for k in keys}

        def sched(opt):
            s = cfg.SOLVER[sec]
            return create_scheduler(opt, s.MAX_EPOCHS, s.LR_MIN, s.WARMUP_LR_INIT, s.WARMUP_EPOCHS)

        opt = make_optimizer_1stage(cfg, m, sec)
        assert isinstance(opt, ops.PromptAdam) and len(opt.param_groups) == len(names)
        torch.manual_seed(5)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.train"):
            do_train_stage1(cfg, m, loader, opt, sched(opt), 0, is_stage1b=(stage == "1b"))
        text = caplog.text
        assert "fused (mpreid.ops.PromptTrainer)" in text and "Epoch[1] Iteration[3/3] Loss:" in text and "nan" not in text.lower()
        fused = {k: getattr(pl, k).detach().clone() for k in keys}
        assert all(opt.state[id(getattr(pl, k))]["step"] == 3 for k in names)
        with torch.no_grad():
            tuned = [m(label=label, get_text=True, view=v).clone() for v in (view, None)]

        # the checkpoint of the loop -> load_param -> the same get_text bits
        path = tmp_path / ("ViT-B-16_stage%s_1.pth" % stage)
        assert path.exists()
        _, m2 = _stage1_model(tmp_path)
        m2.load_param(str(path))
        m2.prompt_learner.set_training_stage(stage)
        with torch.no_grad():
            got = [m2(label=label, get_text=True, view=v) for v in (view, None)]
        assert torch.equal(got[0], tuned[0]) and torch.equal(got[1], tuned[1])
        del m2

        # the autograd path from the same state and permutation
        with torch.no_grad():
            for k in keys:
                getattr(pl, k).copy_(start[k])
        topt = torch.optim.Adam([{"params": [getattr(pl, k)], "lr": cfg.SOLVER[sec].BASE_LR,
                                  "weight_decay": cfg.SOLVER[sec].WEIGHT_DECAY} for k in names], foreach=False)
        torch.manual_seed(5)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.train"):
            do_train_stage1(cfg, m, loader, topt, sched(topt), 0, is_stage1b=(stage == "1b"))
        assert "autograd step" in caplog.text
        lr = sched(topt)._get_lr(1)[0]
        for k in names:
            assert float((getattr(pl, k).detach() - start[k]).abs().max()) > 0
            close = (fused[k] - getattr(pl, k).detach()).abs() <= 3e-3 * lr
            print("do_train_stage1 %s: %s, %.4f of the elements agree with the autograd path" % (stage, k, float(close.float().mean())))
            assert float(close.float().mean()) >= 0.99, k
        for k in keys:
            if k not in names:
                assert torch.equal(fused[k], start[k]) and torch.equal(getattr(pl, k).detach(), start[k]), k


# ---- 6. it learns ------------------------------------------------------------------------------------------------------------------
def test_forty_fused_steps_learn_and_follow_the_float64_curve(reduced_tower):
    """stage 1a on the reduced tower, 6 identities, 48 image features around a hidden teacher, 40 steps on the whole set: the
    last loss is below the first, and the loss curve's largest relative deviation from the float64 host run of the same loop is
    at most 4x that of the fp32 host run.  End points on the host (float64 / fp32): 11.842184 -> 4.181430 / 11.842184 ->
    4.181430, fp32 deviation 1.4e-7; measured on an MI355X: 11.842182 -> 4.181430, deviation 1.9e-7."""
    cfg, sd, student, img, labels = sc.learn_setup()
    enc = ops.TextEncoder(cfg, sd, ws_tag="stage1_learn")
    pl = _learner(student)
    pl.set_training_stage("1a")
    L = sc.LEARN
    trainer = ops.PromptTrainer(enc, pl, "1a", eot=L["eot"], lr=L["lr"], weight_decay=L["weight_decay"])
    I, y = torch.from_numpy(img).cuda(), torch.from_numpy(labels).cuda()
    curve = torch.stack([trainer.step(I, y).sum() for _ in range(L["steps"])]).cpu().numpy().astype(np.float64)
    want, host = sc.learn_curve_host(torch.float64), sc.learn_curve_host(torch.float32)
    assert want[-1] < 0.5 * want[0]         # the float64 curve itself falls
    dev, hdev = sc.curve_deviation(curve, want), sc.curve_deviation(host, want)
    print("forty steps: loss %.6f -> %.6f (float64 %.6f -> %.6f, fp32 host %.6f -> %.6f); deviation %.3e, fp32 host %.3e"
          % (curve[0], curve[-1], want[0], want[-1], host[0], host[-1], dev, hdev))
    assert np.isfinite(curve).all() and curve[-1] < curve[0]
    assert dev <= 4 * hdev


# ---- 7. limits and errors -----------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_next_call_intact():
    case = (65, 64, "groups", sc.SCALE)
    img, txt, labels = sc.supcon_case(*case)
    want = sc.supcon_want(*case)
    I, T, y = torch.from_numpy(img).cuda(), torch.from_numpy(txt).cuda(), torch.from_numpy(labels).cuda()
    L = _lib.load()

    def good():
        loss, d_txt = ops.supcon_pair(I, T, y)
        assert sc.rel_l2(d_txt.cpu().numpy(), want[1]) <= sc.BOUND and sc.rel_l2(loss.cpu().numpy(), want[0]) <= sc.BOUND

    good()
    # the largest batch works; one more is MPREID_ERR_UNSUPPORTED
    top = _lib.SUPCON_MAX_BATCH
    rng = np.random.default_rng(81)
    big_i, big_t = (rng.standard_normal((top + 1, 4)) * sc.SCALE).astype(np.float32), (rng.standard_normal((top + 1, 4)) * sc.SCALE).astype(np.float32)
    big_y = rng.integers(0, 300, top + 1)
    w = sc.supcon_f64(big_i[:top], big_t[:top], big_y[:top])
    loss, d_txt, d_img = ops.supcon_pair(torch.from_numpy(big_i[:top]).cuda(), torch.from_numpy(big_t[:top]).cuda(),
                                         torch.from_numpy(big_y[:top]).cuda(), need_d_img=True)
    fig = (sc.rel_l2(loss.cpu().numpy(), w[0]), sc.rel_l2(d_txt.cpu().numpy(), w[1]), sc.rel_l2(d_img.cpu().numpy(), w[2]))
    print("supcon at batch %d: loss %.3e d_txt %.3e d_img %.3e" % ((top,) + fig))
    assert max(fig) <= sc.BOUND
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.supcon_pair(torch.from_numpy(big_i).cuda(), torch.from_numpy(big_t).cuda(), torch.from_numpy(big_y).cuda())
    good()
    with pytest.raises(ValueError):
        ops.supcon_pair(I, T[:-1], y)
    with pytest.raises(ValueError):
        ops.supcon_pair(I, T, y[:-1])
    # a short workspace, misaligned pointers, a null pointer: through the C entry point
    B, D = img.shape
    need = L.mpreid_supcon_workspace_bytes(B, D)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    loss, d_txt = torch.empty(2, device="cuda"), torch.empty(B, D, device="cuda")

    def call(img_ptr, loss_ptr, ws_ptr, ws_bytes):
        return L.mpreid_supcon_pair_f32(img_ptr, T.data_ptr(), y.data_ptr(), B, D, loss_ptr, d_txt.data_ptr(), None, ws_ptr, ws_bytes,
                                        _lib.stream_ptr())
    assert call(I.data_ptr(), loss.data_ptr(), ws.data_ptr(), need - 1) == _lib.ERR_WORKSPACE
    assert call(I.data_ptr() + 2, loss.data_ptr(), ws.data_ptr(), need) == _lib.ERR_ARG
    assert call(I.data_ptr(), loss.data_ptr() + 1, ws.data_ptr(), need) == _lib.ERR_ARG
    assert call(I.data_ptr(), loss.data_ptr(), ws.data_ptr() + 16, need) == _lib.ERR_ARG
    assert call(None, loss.data_ptr(), ws.data_ptr(), need) == _lib.ERR_ARG
    good()
    assert call(I.data_ptr(), loss.data_ptr(), ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert sc.rel_l2(d_txt.cpu().numpy(), want[1]) <= sc.BOUND
    # the segment sum and the optimizer: host-side validation and library errors, then a good call
    src = torch.from_numpy(sc.segment_src(7, 21, 128)).cuda()
    idx = torch.tensor([5, 0, 3, 3, 0, 5, 3]).cuda()
    ref = sc.segment_sum_f32(src.cpu().numpy(), idx.tolist(), 1, 8, 6)
    with pytest.raises(ValueError):
        ops.rows_segment_sum(src, torch.tensor([5, 0, 3, 3, 0, 6, 3]).cuda(), 1, 8, 6)
    with pytest.raises(ValueError):
        ops.rows_segment_sum(src, idx, 14, 8, 6)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_ARG):
        ops.rows_segment_sum(src, idx, 1, 8, 0, out=torch.empty(0, 8, 128, device="cuda"), validate=False)
    assert np.array_equal(ops.rows_segment_sum(src, idx, 1, 8, 6).cpu().numpy(), ref)
    # an index outside the segments is never an address: validate=False, the row belongs to no segment
    loose = ops.rows_segment_sum(src, torch.tensor([5, 0, 3, 3, 0, 99, -4]).cuda(), 1, 8, 6, validate=False)
    assert np.array_equal(loose.cpu().numpy(), sc.segment_sum_f32(src.cpu().numpy(), [5, 0, 3, 3, 0, 99, -4], 1, 8, 6))
    p = torch.zeros(10, device="cuda")
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_ARG):
        ops.adam_step(p, torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(10, device="cuda"), 0, 1e-3)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_ARG):
        ops.adam_step(p, torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(10, device="cuda"), 1, 1e-3, betas=(0.9, 1.0))
    assert not p.any()
    ops.adam_step(p, torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(10, device="cuda"), 1, 1e-3)
    assert torch.allclose(p, torch.full((10,), -1e-3, device="cuda"), rtol=1e-5)
    good()
    assert ctypes.sizeof(ctypes.c_float) == 4
