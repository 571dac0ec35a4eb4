"""Host-side checks of the image tower's gradient work: the float64 restatement of the tower (vit_grad_cases.py) against
oracle.vit_features, torch.autograd.gradcheck on it, the premises of the attention data (a saturated slab at two tokens; a
causally masked gradient is far from the unmasked one at every token count), the workspace query and the argument checks of
the new entry points.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import text_cases as tc
import text_grad_cases as tg
import vit_grad_cases as vg
from mpreid import _lib, synth
from oracle import oracle

NEW_SYMBOLS = ("mpreid_vit_forward_train", "mpreid_vit_attention_backward_workspace_bytes", "mpreid_vit_attention_backward",
               "mpreid_vit_backward_workspace_bytes", "mpreid_vit_backward", "mpreid_transpose_pad_f32",
               "mpreid_colsum_workspace_bytes", "mpreid_colsum_f32")


def test_new_symbols_resolve():
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and hasattr(L, name), name


@pytest.mark.parametrize("name", ["stride12", "one_layer", "two_layers"])
def test_restatement_forward_equals_the_oracle(name):
    """f | f_proj of the restatement equals oracle.vit_features(..., dtype="float64") to 1e-12; f_last is ln_pre's CLS row with
    one layer and differs from it with more"""
    cfg, img_hw, sd, imgs, cv, (f_last, f, f_proj) = vg.tower_case(name)
    ref = oracle.vit_features(sd, cfg, imgs, cv_emb=cv, dtype="float64")
    assert tc.rel_l2(torch.cat([f, f_proj], dim=1), ref) <= 1e-12
    one = vg.tower(dict(cfg, layers=1), vg.weights(sd), tc._t64(imgs), tc._t64(cv))[0]
    zero = vg.tower(dict(cfg, layers=0), vg.weights(sd), tc._t64(imgs), tc._t64(cv))[0]
    assert torch.equal(one, zero)                       # ln_pre's output either way
    assert torch.equal(f_last, one) == (cfg["layers"] == 1)


def test_gradcheck_of_the_restatement():
    """torch.autograd.gradcheck with its defaults: the tower in two parameter tensors, cv_emb and (attention alone) qkv"""
    cfg = vg.tower_cfg((32, 32), layers=2, out_dim=16)
    g = vg.weights(synth.vit_state_dict(cfg, seed=11, ln_jitter=0.1))
    imgs = tc._t64(synth.synthetic_images(2, 32, 32, seed=12))
    cv = (0.05 * torch.randn(2, cfg["width"], generator=torch.Generator().manual_seed(1), dtype=torch.float64)).requires_grad_(True)
    names = ("transformer.resblocks.0.attn.in_proj_bias", "ln_pre.weight")
    leaves = [g[k].clone().requires_grad_(True) for k in names]

    def run(cv_, *params):
        return vg.tower(cfg, dict(g, **dict(zip(names, params))), imgs, cv_)
    assert torch.autograd.gradcheck(run, (cv, *leaves))
    qkv = vg.make_qkv(128, 2, 2, 5).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: tg.attention(x, 2, 2, vg.all_keys(5)), (qkv,))


def test_two_token_slab_is_saturated():
    """both rows of (image 0, head 0) at two tokens put all but 1e-10 .. 1e-6 of their probability on one key: below what fp32
    holds of 1 - P to any digit, within what float64 holds to six"""
    for width, heads in vg.ATT_SHAPES:
        p = vg.probabilities(vg.make_qkv(width, heads, vg.ATT_BATCH, 2), vg.ATT_BATCH, heads)[0, 0]
        rest = 1.0 - p.max(dim=1).values
        print(width, heads, rest.tolist())
        assert bool((rest <= 1e-6).all()) and bool((rest >= 1e-10).all()), rest
        others = vg.probabilities(vg.make_qkv(width, heads, vg.ATT_BATCH, 2), vg.ATT_BATCH, heads)[1:]
        assert float((1.0 - others.max(dim=-1).values).min()) > 1e-4   # the other images' slabs are ordinary


@pytest.mark.parametrize("tokens", vg.ATT_TOKENS + [vg.ATT_MAX[2]])
def test_a_causally_masked_gradient_is_far_from_the_unmasked_one(tokens):
    """a kernel that masks (the text tower's) cannot pass: the float64 gradient under the causal mask differs from the unmasked
    one by >= 0.1 in the figure of the GPU test, at every token count"""
    width, heads = vg.ATT_SHAPES[0]
    batch = vg.ATT_MAX[3] if tokens == vg.ATT_MAX[2] else vg.ATT_BATCH
    qkv, d_o, want = vg.attention_grad_case(width, heads, tokens, batch)
    fig = tg.grad_figure(tg.attention_grad(qkv, d_o, batch, heads, tc.causal_mask(tokens)), want, batch, heads)
    print(tokens, fig)
    assert fig >= vg.MASK_FLOOR


def test_attention_backward_workspace_query_needs_no_device():
    q = _lib.load().mpreid_vit_attention_backward_workspace_bytes
    for batch, tokens, heads in ((1, 2, 2), (3, 129, 12), (64, 129, 12), (1, 1025, 2)):
        assert q(batch, tokens, heads) >= batch * tokens * heads * 16
        assert q(batch, tokens, heads) % 256 == 0
    assert q(0, 129, 12) == 0 and q(3, 1, 12) == 0 and q(3, 1026, 12) == 0 and q(3, 129, 0) == 0


def test_attention_backward_checks_its_arguments_before_any_launch():
    """no device here: every refusal below happens before the first HIP call"""
    L = _lib.load()
    att = L.mpreid_vit_attention_backward
    d = ctypes.c_void_p(0x1000)
    need = L.mpreid_vit_attention_backward_workspace_bytes(1, 17, 2)

    def run(qkv=d, d_o=d, batch=1, tokens=17, width=128, heads=2, out=d, ws=d, ws_bytes=need):
        return att(qkv, d_o, batch, tokens, width, heads, out, ws, ws_bytes, None)
    for kw in ("qkv", "d_o", "out"):
        assert run(**{kw: None}) == _lib.ERR_ARG, kw
        assert run(**{kw: ctypes.c_void_p(0x1008)}) == _lib.ERR_ARG, kw
    assert run(batch=0) == _lib.ERR_ARG
    assert run(ws=None) == _lib.ERR_WORKSPACE and run(ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert "workspace too small" in L.mpreid_last_error().decode()
    assert run(ws=ctypes.c_void_p(0x1004)) == _lib.ERR_ARG
    for what, kw in {"one token": dict(tokens=1), "over the limit": dict(tokens=1026), "head dim 32": dict(heads=4),
                     "width 64": dict(width=64, heads=1), "width 1152": dict(width=1152, heads=18)}.items():
        assert run(**kw) == _lib.ERR_UNSUPPORTED, what
        assert L.mpreid_last_error().decode(), what


def test_forward_train_checks_its_arguments_before_any_launch():
    L = _lib.load()
    d = ctypes.c_void_p(0x1000)
    layers = (_lib.VitLayer * 3)()
    w = _lib.VitWeights(layers=ctypes.cast(layers, ctypes.POINTER(_lib.VitLayer)))
    img = _lib.ImageIn(f32_dev=0x1000)

    def cfg(layers=3, precision=_lib.VIT_SPLIT, heads=2):
        return _lib.VitCfg(64, 32, 16, 16, 4, 2, 128, layers, heads, 64, 0, 1, precision)

    def run(c, weights=w, image=img, batch=2, f_last=d, f=d, f_proj=d, ws=None, ws_bytes=0):
        return L.mpreid_vit_forward_train(ctypes.byref(c), None if weights is None else ctypes.byref(weights),
                                          None if image is None else ctypes.byref(image), batch, None, f_last, f, f_proj, ws,
                                          ws_bytes, None)
    good = cfg()
    assert run(good) == _lib.ERR_WORKSPACE
    need = L.mpreid_vit_workspace_bytes(ctypes.byref(good), 2)
    assert run(good, ws=d, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    for what, c in {"no layer": cfg(layers=0), "fp16": cfg(precision=_lib.VIT_F16), "head dim 32": cfg(heads=4)}.items():
        assert run(c) == _lib.ERR_UNSUPPORTED, what
        assert L.mpreid_last_error().decode(), what
    for kw in ("f_last", "f", "f_proj", "weights", "image"):
        assert run(good, **{kw: None}) == _lib.ERR_ARG, kw
    assert run(good, batch=0) == _lib.ERR_ARG
    assert run(good, f=ctypes.c_void_p(0x1002)) == _lib.ERR_ARG


def test_backward_workspace_bytes_and_argument_errors_before_any_launch():
    L = _lib.load()
    d = ctypes.c_void_p(0x1000)
    n_layers = 3
    layers = (_lib.VitLayer * n_layers)()
    w = _lib.VitWeights(layers=ctypes.cast(layers, ctypes.POINTER(_lib.VitLayer)))
    for k in ("conv_w", "class_emb", "pos_emb", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b", "proj"):
        setattr(w, k, 0x1000)
    lt = (_lib.TextLayerT * n_layers)()
    for t in lt:
        for k in ("in_proj_t", "out_proj_t", "fc_t", "proj_t"):
            setattr(t, k, 0x1000)
    wt = _lib.VitWeightsT(ctypes.cast(lt, ctypes.POINTER(_lib.TextLayerT)))
    img = _lib.ImageIn(f32_dev=0x1000)

    def cfg(layers=n_layers, precision=_lib.VIT_SPLIT, heads=2):
        return _lib.VitCfg(64, 32, 16, 16, 4, 2, 128, layers, heads, 64, 0, 1, precision)

    def run(c, weights=w, weights_t=wt, image=img, batch=2, seed=d, grads=None, d_tokens=None, ws=None, ws_bytes=0):
        ref = lambda o: None if o is None else ctypes.byref(o)
        return L.mpreid_vit_backward(ctypes.byref(c), ref(weights), ref(weights_t), ref(image), batch, None, seed, seed, seed,
                                     ref(grads), d_tokens, ws, ws_bytes, None)
    good = cfg()
    need = L.mpreid_vit_backward_workspace_bytes(ctypes.byref(good), 2)
    fwd = L.mpreid_vit_workspace_bytes(ctypes.byref(good), 2)
    rows = 256   # 2 x 9 token rows, rounded up to the GEMM's tile
    assert need > fwd + rows * 128 * 4 * (1 + n_layers + 1 + 4 + 1 + 3)   # tokens, x_l, dx, dh, t, dqkv
    assert need % 256 == 0
    assert L.mpreid_vit_backward_workspace_bytes(ctypes.byref(good), 4) > need
    assert L.mpreid_vit_backward_workspace_bytes(ctypes.byref(good), 0) == 0
    assert L.mpreid_vit_backward_workspace_bytes(None, 2) == 0
    for what, c in {"no layer": cfg(layers=0), "fp16": cfg(precision=_lib.VIT_F16), "head dim 32": cfg(heads=4)}.items():
        assert L.mpreid_vit_backward_workspace_bytes(ctypes.byref(c), 2) == 0, what
        assert run(c) == _lib.ERR_UNSUPPORTED, what
        assert L.mpreid_last_error().decode(), what
    assert run(good) == _lib.ERR_WORKSPACE
    assert run(good, ws=d, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert "workspace too small" in L.mpreid_last_error().decode()
    assert run(good, ws=ctypes.c_void_p(0x1010), ws_bytes=need) == _lib.ERR_ARG
    for kw in ("weights", "weights_t", "image"):
        assert run(good, **{kw: None}) == _lib.ERR_ARG, kw
    assert run(good, batch=0) == _lib.ERR_ARG
    most = 65535 * 128 // 9                                                      # the column reduction's grid: 65 535 pieces of 128 rows
    assert run(good, batch=most) == _lib.ERR_WORKSPACE
    assert run(good, batch=most + 1) == _lib.ERR_ARG
    assert run(good, seed=ctypes.c_void_p(0x1002)) == _lib.ERR_ARG
    assert run(good, d_tokens=ctypes.c_void_p(0x1008)) == _lib.ERR_ARG
    lg = (_lib.VitLayerGrads * n_layers)()
    assert run(good, grads=_lib.VitGrads()) == _lib.ERR_ARG                      # a grads struct without its layer array
    g = _lib.VitGrads(layers=ctypes.cast(lg, ctypes.POINTER(_lib.VitLayerGrads)))
    assert run(good, grads=g) == _lib.ERR_WORKSPACE                              # all members NULL: fine
    g.proj = 0x1001
    assert run(good, grads=g) == _lib.ERR_ARG
    g.proj = 0
    lg[1].fc_b = 0x1002
    assert run(good, grads=g) == _lib.ERR_ARG
    lt[2].fc_t = 0
    assert run(good) == _lib.ERR_ARG


# (mpreid_vit_backward_workspace_bytes, mpreid_vit_attention_backward_workspace_bytes) as the library answered before both
# sweeps took their shared regions (x_l, dx, dh, t, dqkv) through one definition.  "small" is SMALL of
# tests/test_gpu_tower_launches.py at 64 x 32, "full" ViT-B/16 at 256 x 128; both in the split precision
SMALL_VIT = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
BACKWARD_WORKSPACE_BYTES = {("small", 1): (4089600, 512), ("small", 3): (4200704, 1024), ("small", 64): (14297600, 18432),
                            ("full", 1): (32397824, 24832), ("full", 3): (64715776, 74496), ("full", 64): (1064735232, 1585152)}


@pytest.mark.parametrize("size,batch", sorted(BACKWARD_WORKSPACE_BYTES))
def test_backward_workspace_bytes(size, batch):
    L = _lib.load()
    c, hw = (SMALL_VIT, (64, 32)) if size == "small" else (synth.VIT_B16, (256, 128))
    cfg = _lib.VitCfg(hw[0], hw[1], c["patch"], c["stride"], c["h_res"], c["w_res"], c["width"], c["layers"], c["heads"],
                      c["out_dim"], 0, 1, _lib.VIT_SPLIT)
    got = (L.mpreid_vit_backward_workspace_bytes(ctypes.byref(cfg), batch),
           L.mpreid_vit_attention_backward_workspace_bytes(batch, c["h_res"] * c["w_res"] + 1, c["heads"]))
    assert got == BACKWARD_WORKSPACE_BYTES[(size, batch)]


def test_transpose_and_colsum_check_their_arguments():
    L = _lib.load()
    d = ctypes.c_void_p(0x1000)
    assert L.mpreid_colsum_workspace_bytes(0, 64) == 0 and L.mpreid_colsum_workspace_bytes(7, 0) == 0
    need = L.mpreid_colsum_workspace_bytes(257, 768)
    assert need >= 2 * 3 * 768 * 4 + 257 * 8 and need % 256 == 0                 # two partial arrays of 3 pieces, the row statistics
    assert L.mpreid_colsum_f32(d, d, 257, 768, d, d, d, need - 1, None) == _lib.ERR_WORKSPACE
    assert L.mpreid_colsum_f32(d, d, 257, 768, d, d, None, need, None) == _lib.ERR_WORKSPACE
    assert L.mpreid_colsum_f32(None, d, 257, 768, d, d, d, need, None) == _lib.ERR_ARG
    assert L.mpreid_colsum_f32(d, None, 257, 768, d, d, d, need, None) == _lib.ERR_ARG      # the gamma sum needs x
    assert L.mpreid_colsum_f32(d, d, 257, 768, None, None, d, need, None) == _lib.ERR_ARG
    assert L.mpreid_colsum_f32(d, d, 0, 768, d, d, d, need, None) == _lib.ERR_ARG
    assert L.mpreid_transpose_pad_f32(None, 4, 64, d, 4, None) == _lib.ERR_ARG
    assert L.mpreid_transpose_pad_f32(d, 4, 64, d, 3, None) == _lib.ERR_ARG
    assert L.mpreid_transpose_pad_f32(d, 0, 64, d, 4, None) == _lib.ERR_ARG


def test_kernel_restatements_agree_with_float64():
    """the sequential fp32 restatements the GPU kernels are held to bit for bit are themselves right to fp32 accuracy"""
    dy, x = vg.kernel_inputs(257, 128)
    s, sx = vg.colsum_ref(dy, x)
    x64 = x.astype(np.float64)
    xhat = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-5)
    assert np.abs(s - dy.astype(np.float64).sum(0)).max() <= 1e-4
    assert np.abs(sx - (dy.astype(np.float64) * xhat).sum(0)).max() <= 1e-4
    assert np.array_equal(vg.transpose_pad_ref(dy, 260)[:, :257], dy.T) and not vg.transpose_pad_ref(dy, 260)[:, 257:].any()


def test_tower_gradients_premises():
    """the K third of in_proj_bias's float64 gradient is zero to rounding, so it can only be judged inside the whole tensor;
    with d_f_last alone nothing reaches the last block; every seed and cv_emb reach the embedded sequence"""
    name = "stride12"
    cfg = vg.tower_case(name)[0]
    g = vg.tower_grads(name)
    for i in range(cfg["layers"]):
        assert vg.k_slice_share(g["transformer.resblocks.%d.attn.in_proj_bias" % i], cfg["width"]) <= 1e-12
    alone = vg.tower_grads(name, (True, False, False))
    assert not bool(alone["transformer.resblocks.%d.mlp.c_fc.weight" % (cfg["layers"] - 1)].any())
    assert bool(alone["transformer.resblocks.0.mlp.c_fc.weight"].any())
    assert torch.equal(g["cv_emb"], g["tokens"][:, 0]) and float(g["tokens"].norm()) > 0
    assert torch.allclose(g["class_embedding"], g["tokens"][:, 0].sum(0)) and torch.allclose(g["positional_embedding"], g["tokens"].sum(0))


def test_restatement_gradients_equal_the_reference_golden():
    """tests/golden/vit_grad.npz holds the reference's own VisionTransformer under float64 autograd (features at the CLS row,
    every parameter gradient and cv_emb's, all three seeds non-zero): the restatement agrees to 1e-12 relative"""
    name = vg.GOLDEN_CASE
    golden = np.load(vg.GOLDEN)
    cfg, img_hw, sd, imgs, cv, feats = vg.tower_case(name)
    for k, f in zip(("f_last", "f", "f_proj"), feats):
        assert tc.rel_l2(f, golden[k]) <= vg.GOLDEN_BOUND, k
    mine = vg.tower_grads(name)
    keys = set(sd) | {"cv_emb"}
    assert {k.split("_", 1)[1] for k in golden.files if k.startswith(("g_", "rows_"))} == keys
    for k in sorted(keys):
        assert vg.golden_deviation(k, mine[k].numpy(), golden) <= vg.GOLDEN_BOUND, k
