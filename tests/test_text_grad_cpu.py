"""Host-side checks of the text tower's prompt gradient: the differentiable float64 restatement (text_grad_cases.py) against
text_cases' own, torch.autograd.gradcheck on it, the premise that a wrong mask is far from the causal one in the GRADIENT's
error figure, the workspace query and the argument checks of the new entry points.  No GPU."""
import ctypes

import pytest
import torch

import text_cases as tc
import text_grad_cases as tg
from mpreid import _lib, synth


def test_restatement_forward_equals_tower_f64_exactly():
    cfg, sd, prompts, eot, _, f64 = tc.golden_case("reduced")
    got = tg.tower(cfg, tg.weights(sd), tc._t64(prompts), eot)
    assert torch.equal(got, f64)
    qkv, want, _ = tc.attention_case(128, 2, 17)
    assert torch.equal(tg.attention(qkv.double(), tc.ATT_BATCH, 2), want)


def test_gradcheck_of_the_restatement():
    """torch.autograd.gradcheck with its defaults on a 1-layer, width-128, 5-token tower and on the attention restatement"""
    cfg = dict(tokens=5, width=128, layers=1, heads=2, out_dim=16)
    g = tg.weights(synth.text_state_dict(cfg, seed=11))
    p = tc._t64(tc.make_prompts(cfg, 2, 12)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: tg.tower(cfg, g, x, [4, 2]), (p,))
    qkv = tc.make_qkv(128, 2, 2, 5).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: tg.attention(x, 2, 2), (qkv,))


@pytest.mark.parametrize("tokens", tg.GRAD_TOKENS)
def test_gradient_data_tells_wrong_masks_apart(tokens):
    """every wrong mask of text_cases.WRONG_MASKS that differs from the causal one at this length changes the float64 attention
    gradient by >= MUTANT_FLOOR in the figure of the GPU test (no (mask, count) pair had to be left out)"""
    width, heads = tc.ATT_SHAPES[0]
    qkv, d_o, want = tg.attention_grad_case(width, heads, tokens)
    right = tc.causal_mask(tokens)
    tried = 0
    for name, fn in tc.WRONG_MASKS.items():
        wrong = fn(tokens)
        if bool((wrong == right).all()):
            continue
        tried += 1
        fig = tg.grad_figure(tg.attention_grad(qkv, d_o, tc.ATT_BATCH, heads, wrong), want, tc.ATT_BATCH, heads)
        print(tokens, name, fig)
        assert fig >= tc.MUTANT_FLOOR, (tokens, name, fig)
    assert tried >= 1, tried


def test_new_symbols_resolve():
    L = _lib.load()
    for name in ("mpreid_text_backward_workspace_bytes", "mpreid_text_backward", "mpreid_text_attention_backward",
                 "mpreid_layernorm_backward_f32"):
        assert name in _lib.PROTOTYPES and hasattr(L, name), name


def test_backward_workspace_query_needs_no_device():
    L = _lib.load()
    fwd, bwd = L.mpreid_text_workspace_bytes, L.mpreid_text_backward_workspace_bytes
    for c in (synth.CLIP_TEXT, tc.REDUCED):
        cfg = _lib.TextCfg(**c)
        prev = 0
        for batch in (1, 3, 4, 512, 513):
            mpad = -(-batch * c["tokens"] // 256) * 256
            need = bwd(ctypes.byref(cfg), batch)
            assert need >= fwd(ctypes.byref(cfg), batch) + c["layers"] * mpad * c["width"] * 4, (c, batch)
            assert need >= prev, (c, batch)
            prev = need
        assert bwd(ctypes.byref(cfg), 513) > bwd(ctypes.byref(cfg), 1)
        assert bwd(ctypes.byref(cfg), 0) == 0 and bwd(ctypes.byref(cfg), -3) == 0
    assert bwd(None, 4) == 0
    assert bwd(ctypes.byref(_lib.TextCfg(0, 128, 2, 2, 64)), 2) == 0 and bwd(ctypes.byref(_lib.TextCfg(21, 0, 2, 2, 64)), 2) == 0
    assert bwd(ctypes.byref(_lib.TextCfg(21, 128, -1, 2, 64)), 2) == 0


# mpreid_text_backward_workspace_bytes as the library answered before both sweeps took their shared regions (x_l, dx, dh, t,
# dqkv) through one definition: (tower, batch) -> bytes.  "small" is TEXT of tests/test_gpu_tower_launches.py
SMALL_TEXT = dict(tokens=17, width=128, layers=2, heads=2, out_dim=64)
BACKWARD_WORKSPACE_BYTES = {("small", 1): 2621952, ("small", 3): 2622976, ("small", 64): 13139968,
                            ("full", 1): 15730688, ("full", 3): 15734784, ("full", 64): 314703872}


@pytest.mark.parametrize("size,batch", sorted(BACKWARD_WORKSPACE_BYTES))
def test_backward_workspace_bytes(size, batch):
    c = SMALL_TEXT if size == "small" else synth.CLIP_TEXT
    cfg = _lib.TextCfg(*(c[k] for k in ("tokens", "width", "layers", "heads", "out_dim")))
    assert _lib.load().mpreid_text_backward_workspace_bytes(ctypes.byref(cfg), batch) == BACKWARD_WORKSPACE_BYTES[(size, batch)]


def test_text_backward_checks_its_arguments_before_any_launch():
    """no device here: every refusal below happens before the first HIP call"""
    L = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    layers = (_lib.VitLayer * 2)()
    w = _lib.TextWeights(pos_emb=0x1000, ln_final_g=0x1000, ln_final_b=0x1000, proj=0x1000,
                         layers=ctypes.cast(layers, ctypes.POINTER(_lib.VitLayer)))
    tl = (_lib.TextLayerT * 2)()
    for t in tl:
        t.in_proj_t = t.out_proj_t = t.fc_t = t.proj_t = 0x1000
    wt = _lib.TextWeightsT(proj_t=0x1000, layers=ctypes.cast(tl, ctypes.POINTER(_lib.TextLayerT)))

    def run(cfg, prompts=dummy, eot=dummy, grad_out=dummy, batch=2, out=dummy, ws=None, ws_bytes=0, weights=w, weights_t=wt):
        return L.mpreid_text_backward(ctypes.byref(cfg), None if weights is None else ctypes.byref(weights),
                                      None if weights_t is None else ctypes.byref(weights_t), prompts, eot, grad_out, batch, out,
                                      ws, ws_bytes, None)
    good = _lib.TextCfg(21, 128, 2, 2, 64)
    assert run(good) == _lib.ERR_WORKSPACE and "workspace too small" in L.mpreid_last_error().decode()
    need = L.mpreid_text_backward_workspace_bytes(ctypes.byref(good), 2)
    assert run(good, ws=dummy, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert run(good, ws=ctypes.c_void_p(0x1010), ws_bytes=need) == _lib.ERR_ARG          # the workspace: 256-byte aligned
    for what, cfg in {"tokens over the limit": _lib.TextCfg(_lib.TEXT_MAX_TOKENS + 1, 128, 2, 2, 64), "one token": _lib.TextCfg(1, 128, 2, 2, 64),
                      "head dim 32": _lib.TextCfg(21, 128, 2, 4, 64), "width 64": _lib.TextCfg(21, 64, 2, 1, 64),
                      "width 1152": _lib.TextCfg(21, 1152, 2, 18, 64)}.items():
        assert run(cfg) == _lib.ERR_UNSUPPORTED, what
        assert L.mpreid_last_error().decode(), what
    for kw in ("prompts", "eot", "grad_out", "out", "weights", "weights_t"):
        assert run(good, **{kw: None}) == _lib.ERR_ARG, kw
    assert run(good, batch=0) == _lib.ERR_ARG
    assert run(good, prompts=ctypes.c_void_p(0x1004)) == _lib.ERR_ARG and run(good, out=ctypes.c_void_p(0x1008)) == _lib.ERR_ARG
    tl[1].fc_t = 0
    assert run(good) == _lib.ERR_ARG
    tl[1].fc_t = 0x1000
    # the unit entry points
    att = L.mpreid_text_attention_backward
    assert att(None, dummy, 1, 17, 128, 2, dummy, None) == _lib.ERR_ARG and att(dummy, None, 1, 17, 128, 2, dummy, None) == _lib.ERR_ARG
    assert att(dummy, dummy, 1, 17, 128, 2, None, None) == _lib.ERR_ARG and att(dummy, dummy, 0, 17, 128, 2, dummy, None) == _lib.ERR_ARG
    assert att(dummy, ctypes.c_void_p(0x1008), 1, 17, 128, 2, dummy, None) == _lib.ERR_ARG
    assert att(dummy, dummy, 1, _lib.TEXT_MAX_TOKENS + 1, 128, 2, dummy, None) == _lib.ERR_UNSUPPORTED
    assert att(dummy, dummy, 1, 1, 128, 2, dummy, None) == _lib.ERR_UNSUPPORTED
    assert att(dummy, dummy, 1, 17, 128, 4, dummy, None) == _lib.ERR_UNSUPPORTED
    ln = L.mpreid_layernorm_backward_f32
    assert ln(None, dummy, dummy, 4, 128, 0, dummy, None) == _lib.ERR_ARG and ln(dummy, dummy, dummy, 4, 0, 0, dummy, None) == _lib.ERR_ARG
    assert ln(dummy, dummy, dummy, -1, 128, 0, dummy, None) == _lib.ERR_ARG and ln(dummy, dummy, dummy, 0, 128, 1, dummy, None) == 0
