"""The text tower's gradient with respect to the prompts on the GPU (mpreid_text_backward and its kernels): causal attention
backward and LayerNorm backward against float64 autograd, their memory discipline and run-to-run bits; the tower's prompt
gradient against the float64 restatement; exact zeros behind the read-out row, exact homogeneity, batch independence; autograd
end to end on the Uni-Prompt model; the checkpoint round trip; limits and errors.  Oracles: tests/text_grad_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import text_cases as tc
import text_grad_cases as tg
from row_kernel_cases import massive_rows
from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu

BOUND = 2e-5   # relative L2, the project's split-mode bar (text_cases.BOUND_SPLIT for the slab-relative figure)


@pytest.fixture(scope="module")
def towers():
    """name -> (cfg, encoder, prompts on the device, eot, grad_out on the device, float64 gradient), built once"""
    out = {}
    for name in ("reduced", "full"):
        cfg, sd, prompts, eot, g, want = tg.tower_grad_case(name)
        out[name] = (cfg, ops.TextEncoder(cfg, sd, ws_tag="textgrad_" + name), torch.from_numpy(prompts).cuda(), eot,
                     torch.from_numpy(g).cuda(), want)
    return out


# ---- 1. the attention backward kernel against float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", tg.GRAD_TOKENS)
@pytest.mark.parametrize("width,heads", tc.ATT_SHAPES)
def test_attention_backward_against_float64(width, heads, tokens):
    """slab-relative error of dq | dk | dv (text_grad_cases.grad_figure) <= 2e-5.  Largest figure measured on an MI355X over the
    18 cases: 2.6e-6 ((512, 8), L = 3); 4e-7 .. 2.2e-6 elsewhere.  For information, fp32 autograd on the host is printed beside it:
    within a factor 2.2 either way, except (512, 8), L = 2, where a saturated two-token slab costs the plain form of dS four
    digits (1.2e-4) and the kernel's form, taken about the strongest key, none (9.5e-7)"""
    qkv, d_o, want = tg.attention_grad_case(width, heads, tokens)
    got = ops.text_attention_backward(qkv.cuda(), d_o.cuda(), tc.ATT_BATCH, tokens, heads)
    assert bool(torch.isfinite(got).all())
    fig = tg.grad_figure(got, want, tc.ATT_BATCH, heads)
    host = tg.grad_figure(tg.attention_grad(qkv, d_o, tc.ATT_BATCH, heads, dtype=torch.float32), want, tc.ATT_BATCH, heads)
    print("attention backward (%d, %d) L = %d: %.3e; fp32 autograd on the host %.3e, ratio %.2f"
          % (width, heads, tokens, fig, host, fig / host if host else float("inf")))
    assert fig <= tc.BOUND_SPLIT


SAT_CASES = [(w, h, t, False) for w, h in tc.ATT_SHAPES for t in tg.SAT_TOKENS] + [(128, 2, tg.TIED_TOKENS, True)]


@pytest.mark.parametrize("width,heads,tokens,tied", SAT_CASES)
def test_attention_backward_on_saturated_slabs(width, heads, tokens, tied):
    """slab (prompt 0, head 0) saturated on every row, row i's strongest key (37 i + 5) mod (i + 1): on both lane halves at 128
    tokens (text_grad_cases.saturate; premises in test_clip_like_premises_cpu.py: the kernel's expressions in fp32 are within
    1e-5, plain fp32 autograd is 1.4e-3 .. 0.56 away on that slab).  tied: slab (1, 0) holds exact copies of key 63 at 64 and
    of key 0 at L - 1, and every fourth row (and the last) is pointed at one of them: two keys hold the maximum to the bit.
    Finite; the slab-relative figure <= 2e-5 (its scale is per slab, so the saturated slab is judged on its own); a second call
    gives the same bits; prompt 0 alone has the bits it has inside the batch.
    Measured on an MI355X over the 11 cases: 1.3e-6 .. 5.0e-6 (largest (128, 2), L = 77), the tied case 1.7e-6; fp32 autograd on
    the host 1.4e-3 .. 0.56"""
    qkv, d_o, want = tg.saturated_case(width, heads, tokens, tied)
    B = tc.ATT_BATCH
    q, g = qkv.cuda(), d_o.cuda()
    got = ops.text_attention_backward(q, g, B, tokens, heads).clone()
    assert bool(torch.isfinite(got).all())
    fig = tg.grad_figure(got, want, B, heads)
    host = tg.attention_grad(qkv, d_o, B, heads, dtype=torch.float32)
    on_slab = [tg.grad_figure(tg.slab(x, B, heads, 0, 0), tg.slab(want, B, heads, 0, 0), 1, 1) for x in (got, host)]
    print("attention backward, saturated%s (%d, %d) L = %d: %.3e (slab (0, 0) %.3e); fp32 autograd on the host %.3e (slab (0, 0) %.3e)"
          % (" and tied" if tied else "", width, heads, tokens, fig, on_slab[0], tg.grad_figure(host, want, B, heads), on_slab[1]))
    assert fig <= tc.BOUND_SPLIT
    again = ops.text_attention_backward(q, g, B, tokens, heads)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    alone = ops.text_attention_backward(q[:tokens].contiguous(), g[:tokens].contiguous(), 1, tokens, heads)
    assert torch.equal(alone.view(torch.int32), got[:tokens].view(torch.int32))


# ---- 2. poison, and the same bits twice ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [17, 77])
def test_attention_backward_writes_d_qkv_and_nothing_else(tokens):
    """qkv and d_o are followed by NaN guard rows in their allocations, d_qkv lies between sentinel guard rows: finite results,
    every element of d_qkv written (none keeps the sentinel's NaN), every guard byte untouched; a second call gives the same bits"""
    width, heads = 128, 2
    B, G = tc.ATT_BATCH, 32
    qkv, d_o, want = tg.attention_grad_case(width, heads, tokens)
    M = B * tokens
    buf = torch.full((M + G, 3 * width), float("nan"), dtype=torch.float32, device="cuda")
    buf[:M] = qkv.cuda()
    gbuf = torch.full((M + G, width), float("nan"), dtype=torch.float32, device="cuda")
    gbuf[:M] = d_o.cuda()
    sentinel = 0x7FC12345   # a NaN pattern
    obuf = torch.full((G + M + G, 3 * width), sentinel, dtype=torch.int32, device="cuda")
    out = obuf[G:G + M].view(torch.float32)
    ops.text_attention_backward(buf[:M], gbuf[:M], B, tokens, heads, out=out)
    torch.cuda.synchronize()
    assert bool((obuf[:G] == sentinel).all()) and bool((obuf[G + M:] == sentinel).all())
    assert bool(torch.isnan(buf[M:]).all()) and bool(torch.isnan(gbuf[M:]).all())
    assert bool(torch.isfinite(out).all())
    assert tg.grad_figure(out, want, B, heads) <= tc.BOUND_SPLIT
    again = ops.text_attention_backward(buf[:M], gbuf[:M], B, tokens, heads)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


# ---- 3. LayerNorm backward -----------------------------------------------------------------------------------------------------
def _ln_grad64(x, dy, gamma):
    x64 = x.double().requires_grad_(True)
    y = tc._ln64(x64, gamma.double(), torch.zeros_like(gamma).double())
    return torch.autograd.grad(y, x64, grad_outputs=dy.double())[0]


@pytest.mark.parametrize("width", [128, 512, 768, 1024])
def test_layernorm_backward_against_float64(width):
    """rows of tiny variance (far below eps: sigma is eps's), of ordinary and of large variance, and rows with the massive
    channels of a trained CLIP tower under gammas of x30-100 and 0.02 (massive_rows; the kernel's expressions in fp32 on the
    host give 6e-8 .. 1e-7 there); the plain and the accumulate form; relative L2 <= 2e-5 per group of rows.
    Measured on an MI355X on the massive rows: 6.2e-8 .. 9.5e-8 plain, 6.2e-8 .. 1.0e-7 accumulate"""
    g = torch.Generator().manual_seed(width)
    rows = 37   # not a multiple of the four rows of a workgroup
    groups = {"tiny": 0.5 + 1e-4 * torch.randn(rows, width, generator=g), "unit": torch.randn(rows, width, generator=g),
              "large": 100.0 + 1e3 * torch.randn(rows, width, generator=g)}
    gamma_plain = 1.0 + 0.05 * torch.randn(width, generator=g)
    x_massive, gamma_massive = massive_rows(rows, width, 1000 + width)
    groups["massive"] = x_massive
    for name, x in groups.items():
        gamma = gamma_massive if name == "massive" else gamma_plain
        dy = torch.randn(rows, width, generator=g)
        want = _ln_grad64(x, dy, gamma)
        got = ops.layernorm_backward(x.cuda(), dy.cuda(), gamma.cuda())
        base = torch.randn(rows, width, generator=g) * float(want.abs().mean())
        acc = base.cuda().clone()
        assert ops.layernorm_backward(x.cuda(), dy.cuda(), gamma.cuda(), out=acc) is acc
        e_plain, e_acc = tc.rel_l2(got, want), tc.rel_l2(acc, base.double() + want)
        print("layernorm backward W = %d, %s rows: %.3e plain, %.3e accumulate" % (width, name, e_plain, e_acc))
        assert e_plain <= BOUND and e_acc <= BOUND, (name, e_plain, e_acc)


# ---- 4. the tower's prompt gradient against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reduced", "full"])
def test_tower_gradient_against_float64(towers, name):
    """relative L2 <= 2e-5 against torch.autograd.grad of the float64 restatement; rows behind the read-out row are 0.0 exactly.
    Measured on an MI355X: 7.2e-7 (reduced), 1.8e-6 (full)"""
    cfg, enc, prompts, eot, g, want = towers[name]
    got = enc.backward(prompts, eot, g)
    assert got.shape == prompts.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    fig = tc.rel_l2(got, want)
    print("text tower gradient %s: rel L2 %.3e against float64" % (name, fig))
    assert fig <= BOUND
    rows = torch.arange(cfg["tokens"], device="cuda")[None, :]
    e = torch.as_tensor(np.asarray(eot)).cuda().long()[:, None]
    behind = (rows > e)[:, :, None].expand_as(got)
    assert int(behind.sum()) > 0 and bool((got[behind] == 0.0).all())
    assert bool((got[torch.arange(len(eot), device="cuda"), e[:, 0]] != 0.0).any(dim=1).all())   # the read-out rows themselves
    assert float(want[behind.cpu()].abs().max()) == 0.0


# ---- 5. exact homogeneity --------------------------------------------------------------------------------------------------------
def test_gradient_is_exactly_homogeneous_in_grad_out(towers):
    cfg, enc, prompts, eot, g, _ = towers["reduced"]
    s = 2.0 ** -40
    full = enc.backward(prompts, eot, g)
    assert torch.equal((enc.backward(prompts, eot, g * s)).view(torch.int32), (full * s).view(torch.int32))
    g0 = g.clone()
    g0[1] = 0.0
    z = enc.backward(prompts, eot, g0)
    assert bool((z[1] == 0.0).all()) and torch.equal(z[0], full[0]) and torch.equal(z[2:], full[2:])


# ---- 6. batch independence -------------------------------------------------------------------------------------------------------
def test_a_prompt_gradient_has_the_same_bits_alone_in_a_batch_and_across_the_chunk_edge(towers):
    cfg, enc, prompts, eot, g, _ = towers["reduced"]
    n = prompts.shape[0]
    alone = [enc.backward(prompts[i:i + 1], eot[i:i + 1], g[i:i + 1]).clone() for i in range(n)]
    three = enc.backward(prompts[1:4], eot[1:4], g[1:4])
    for k in range(3):
        assert torch.equal(three[k:k + 1], alone[1 + k]), k
    assert enc.CHUNK == 512
    enc.CHUNK = 2       # on the instance: chunks of prompts (0, 1), (2, 3), (4)
    try:
        chunked = enc.backward(prompts, eot, g)
    finally:
        del enc.CHUNK
    assert enc.CHUNK == 512
    whole = enc.backward(prompts, eot, g)
    for i in range(n):
        assert torch.equal(chunked[i:i + 1], alone[i]) and torch.equal(whole[i:i + 1], alone[i]), i


# ---- 7. / 8. autograd end to end on the Uni-Prompt model, and the checkpoint round trip --------------------------------------
def _make_model():
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    return cfg, mu, mu.make_model(cfg, num_class=7, camera_num=6, view_num=1)


def _grads64(mu, m, eot_row, stage, label, view, img):
    """float64: PromptLearner.forward + tower + symmetric contrastive loss -> the gradients of the three context tensors"""
    t = {k: getattr(m.prompt_learner, k).detach().cpu().double() for k in mu.PROMPT_KEYS}
    for k in ("ctx_generic", "ctx_modality", "ctx_platform"):
        t[k].requires_grad_(True)
    sd = {k[len("text_encoder."):]: v for k, v in m.text_state_dict().items() if k.startswith("text_encoder.")}
    prompts = tc.assemble_prompts(t, label.cpu(), stage, None if view is None else view.cpu())
    feats = tg.tower(mu.TEXT_CFG, tg.weights(sd), prompts, [eot_row] * len(label))
    loss = tg.symmetric_loss(img.cpu().double(), feats, label.cpu())
    names = ("ctx_generic",) if stage == "1a" else ("ctx_modality", "ctx_platform")
    return float(loss.detach()), dict(zip(names, torch.autograd.grad(loss, [t[k] for k in names])))


def test_autograd_end_to_end_and_checkpoint_round_trip(tmp_path):
    """measured on an MI355X: ctx_generic.grad 1.8e-6, ctx_modality.grad 2.1e-6, ctx_platform.grad 2.6e-6 (relative L2)"""
    cfg, mu, m = _make_model()
    m.eval()
    pl = m.prompt_learner
    label = torch.tensor([3, 0, 6, 6, 1]).cuda()     # a repeated label: its two prompts accumulate into one ctx_generic row
    view = torch.tensor([0, 6, 11, 12, 13]).cuda()
    g = torch.Generator().manual_seed(3)
    img = (torch.randn(5, 512, generator=g) * 0.1).cuda()   # the pre-computed image features of stage 1: fixed
    eot_row = cfg.MODEL.PROMPT_EOT_INDEX

    # nothing enabled: the evaluation call, no graph
    plain = m(label=label, get_text=True)
    assert plain.grad_fn is None and not plain.requires_grad
    assert all(not p.requires_grad for p in pl.parameters())
    by_hand = m.text_tower().forward(tc.assemble_prompts({k: getattr(pl, k).cpu() for k in mu.PROMPT_KEYS}, label.cpu(), "1a").cuda(),
                                     [eot_row] * 5)
    assert torch.equal(plain, by_hand)
    plain = plain.clone()

    # stage 1a
    m.enable_stage1a_training()
    assert pl.training_stage == "1a" and pl.ctx_generic.requires_grad and pl.ctx_generic.is_leaf
    assert not pl.ctx_modality.requires_grad and not pl.ctx_platform.requires_grad
    feats = m(label=label, get_text=True, view=view)
    assert feats.grad_fn is not None and torch.equal(feats.detach(), plain)
    with torch.no_grad():
        assert m(label=label, get_text=True).grad_fn is None
    loss = tg.symmetric_loss(img, feats, label)
    loss.backward()
    want_loss, want = _grads64(mu, m, eot_row, "1a", label, None, img)
    fig = tc.rel_l2(pl.ctx_generic.grad, want["ctx_generic"])
    print("stage 1a: loss %.6f (float64 %.6f), ctx_generic.grad rel L2 %.3e, |text feature| %.3f"
          % (float(loss.detach()), want_loss, fig, float(feats.detach().norm(dim=1).mean())))
    assert fig <= BOUND
    assert pl.ctx_modality.grad is None and pl.ctx_platform.grad is None
    untouched = [c for c in range(7) if c not in label.tolist()]
    assert bool((pl.ctx_generic.grad[untouched] == 0.0).all()) and bool((pl.ctx_generic.grad[6] != 0.0).any())

    # an optimizer over prompt_learner.parameters() takes a step: the tuned model
    opt = torch.optim.SGD(pl.parameters(), lr=0.5)
    before = pl.ctx_generic.detach().clone()
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert not torch.equal(pl.ctx_generic.detach(), before)

    # stage 1b with the view
    m.enable_stage1b_training()
    assert pl.training_stage == "1b" and not pl.ctx_generic.requires_grad
    assert pl.ctx_modality.requires_grad and pl.ctx_platform.requires_grad
    feats = m(label=label, get_text=True, view=view)
    loss = tg.symmetric_loss(img, feats, label)
    loss.backward()
    want_loss, want = _grads64(mu, m, eot_row, "1b", label, view, img)
    for k in ("ctx_modality", "ctx_platform"):
        fig = tc.rel_l2(getattr(pl, k).grad, want[k])
        print("stage 1b: loss %.6f (float64 %.6f), %s.grad rel L2 %.3e" % (float(loss.detach()), want_loss, k, fig))
        assert fig <= BOUND, k
    assert pl.ctx_generic.grad is None

    # text_state_dict -> torch.save -> load_param reproduces the tuned model's text features bit for bit
    with torch.no_grad():
        tuned = [m(label=label, get_text=True, view=v).clone() for v in (view, None)]
    assert not torch.equal(tuned[0], tuned[1])
    sd = m.text_state_dict()
    assert set(sd) == {"text_encoder." + k for k in mu.text_shapes()} | {"prompt_learner." + k for k in mu.PROMPT_KEYS}
    assert all(v.device.type == "cpu" and not v.requires_grad for v in sd.values())
    path = tmp_path / "tuned_text.pth"
    torch.save(sd, path)
    _, _, m2 = _make_model()
    m2.eval()
    m2.load_param(str(path))
    m2.prompt_learner.set_training_stage("1b")
    got = [m2(label=label, get_text=True, view=v) for v in (view, None)]
    assert got[0].grad_fn is None and torch.equal(got[0], tuned[0]) and torch.equal(got[1], tuned[1])
    m2.prompt_learner.set_training_stage("1a")
    assert not torch.equal(m2(label=label, get_text=True), plain)     # the step moved ctx_generic


# ---- 9. limits and errors --------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_next_call_intact(towers):
    cfg, enc, prompts, eot, g, want = towers["reduced"]
    L = _lib.load()

    def good():
        assert tc.rel_l2(enc.backward(prompts, eot, g), want) <= BOUND

    good()
    # tokens = MPREID_TEXT_MAX_TOKENS works (the attention kernel's largest LDS request), the last row read out
    top = dict(tc.REDUCED, tokens=_lib.TEXT_MAX_TOKENS)
    sd = synth.text_state_dict(top, seed=41)
    p = tc.make_prompts(top, 2, 42)
    e = [_lib.TEXT_MAX_TOKENS - 1, 100]
    go = tg.make_grad_out(2, top["out_dim"], 43)
    fig = tc.rel_l2(ops.TextEncoder(top, sd, ws_tag="textgrad_top").backward(torch.from_numpy(p).cuda(), e, torch.from_numpy(go).cuda()),
                    tg.tower_grad(top, sd, p, e, go))
    print("text tower gradient at %d tokens: rel L2 %.3e against float64" % (_lib.TEXT_MAX_TOKENS, fig))
    assert fig <= BOUND
    # one token more, a head dimension other than 64: MPREID_ERR_UNSUPPORTED
    over = dict(tc.REDUCED, tokens=_lib.TEXT_MAX_TOKENS + 1)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.TextEncoder(over, synth.text_state_dict(over, seed=41), ws_tag="textgrad_over").backward(
            torch.zeros((1, over["tokens"], over["width"]), device="cuda"), [0], torch.zeros((1, over["out_dim"]), device="cuda"))
    good()
    wide = dict(tc.REDUCED, heads=4)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.TextEncoder(wide, synth.text_state_dict(wide, seed=41), ws_tag="textgrad_wide").backward(prompts, eot, g)
    good()
    qkv = tc.make_qkv(128, 2, 1, 17).cuda()
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.text_attention_backward(qkv.half(), torch.zeros((17, 128), device="cuda"), 1, 17, 2)
    # a short workspace, misaligned pointers, a null pointer: through the C entry point
    n = len(eot)
    out = torch.empty_like(prompts)
    e_dev = torch.from_numpy(ops.check_eot(eot, n, cfg["tokens"])).cuda()
    need = L.mpreid_text_backward_workspace_bytes(ctypes.byref(enc.c_cfg), n)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def call(prompts_ptr, out_ptr, ws_ptr, ws_bytes):
        return L.mpreid_text_backward(ctypes.byref(enc.c_cfg), ctypes.byref(enc.c_w), ctypes.byref(enc._transposed_weights()), prompts_ptr,
                                      e_dev.data_ptr(), g.data_ptr(), n, out_ptr, ws_ptr, ws_bytes, _lib.stream_ptr())
    assert call(prompts.data_ptr(), out.data_ptr(), ws.data_ptr(), need - 1) == _lib.ERR_WORKSPACE
    good()
    assert call(prompts.data_ptr() + 4, out.data_ptr(), ws.data_ptr(), need) == _lib.ERR_ARG
    assert call(prompts.data_ptr(), out.data_ptr() + 8, ws.data_ptr(), need) == _lib.ERR_ARG
    assert call(prompts.data_ptr(), out.data_ptr(), ws.data_ptr() + 16, need) == _lib.ERR_ARG
    assert call(None, out.data_ptr(), ws.data_ptr(), need) == _lib.ERR_ARG
    good()
    assert call(prompts.data_ptr(), out.data_ptr(), ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert tc.rel_l2(out, want) <= BOUND
    with pytest.raises(ValueError):
        enc.backward(prompts, [0, 1, 2, 3, cfg["tokens"]], g)
    with pytest.raises(ValueError):
        enc.backward(prompts, eot, g[:, :-1])
    good()
