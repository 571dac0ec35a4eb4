"""Host-side checks of the MoE gradient seams: the closed forms the kernels implement against float64 autograd, the wrong
variants against their floor, the workspace queries and the refusals that need no device.  Cases: tests/moe_grad_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import moe_cases as mc
import moe_grad_cases as gc
from mpreid import _lib, ops


def test_mlp_backward_closed_forms_equal_autograd():
    """d_a and d_w of the routed MLP, slot by slot, against autograd through moe_cases.experts_f64 (float64: ~1e-15)"""
    rng = np.random.default_rng(3)
    width, E = 16, 4
    for K, rows in ((1, 37), (2, 41), (4, 19)):
        sel = np.stack([rng.permutation(E)[:K] for _ in range(rows)]).astype(np.int64)
        w = rng.uniform(0.1, 1.0, size=(rows, K))
        w /= w.sum(-1, keepdims=True)
        h = rng.standard_normal((rows, width))
        dy = rng.standard_normal((rows, width))
        wt = gc.mlp_weights(E, width, rng)
        a0, w0 = gc.mlp_backward_autograd(h, sel, w, *wt, dy)
        a1, w1 = gc.mlp_backward_closed(h, sel, w, *wt, dy)
        ra, rw = mc.rel_l2(a1, a0), mc.rel_l2(w1, w0)
        print("MLP backward closed form vs autograd, K %d: d_a %.2e d_w %.2e" % (K, ra, rw))
        assert ra <= 1e-12 and rw <= 1e-12


@pytest.mark.parametrize("E,K", gc.ROUTE_EK)
def test_route_backward_closed_forms_equal_autograd(E, K):
    """d_logits = w (d_w - c) on the selection plus the load-balancing term, and l_aux, against float64 autograd of
    sum(w * d_w) + coef * load_balancing_loss; K == 1 and coef == 0: exactly zero"""
    logits, d_w = gc.route_case(E, K, rows=300)
    for coef in (0.0, gc.AUX_COEF):
        want, l_aux, sel, w = gc.route_backward_autograd(logits, K, d_w, coef)
        got, l1 = gc.route_backward_closed(logits, sel, w, d_w, coef)
        dev = float((got - want).abs().max())
        scale = max(float(want.abs().max()), 1e-30)
        print("router closed form vs autograd E %d K %d coef %g: max abs %.2e (largest entry %.2e)" % (E, K, coef, dev, scale))
        assert dev <= 1e-13 * max(scale, 1.0)
        assert abs(float(l1 - l_aux)) <= 1e-13
        if coef == 0.0:
            off = torch.ones_like(got, dtype=torch.bool).scatter_(1, sel, False)
            assert float(got[off].abs().max() if off.any() else 0.0) == 0.0
            if K == 1:
                assert float(got.abs().max()) == 0.0


def test_load_balancing_loss_is_one_for_a_uniform_router():
    """E * sum_e f_e P_e with P uniform: sum_e f_e = K, so l_aux = K exactly (the reference's function sums the K choice ranks)"""
    for E, K in ((4, 2), (8, 1)):
        logits = torch.zeros((50, E), dtype=torch.float64)
        sel = mc.topk_lower_first(logits, K)
        assert abs(float(gc.load_balancing_loss(logits, sel)) - K) < 1e-12


def test_wrong_variants_clear_their_floor():
    """every wrong variant of the router gradient is farther than MUTANT_FLOOR from the right one on every case that can tell
    it apart; the figures are those of the comment in moe_grad_cases.py"""
    seen = {v: [] for v in gc.ROUTE_WRONG_VARIANTS}
    for E, K in gc.ROUTE_EK:
        logits, d_w = gc.route_case(E, K, rows=300)
        for v in gc.ROUTE_WRONG_VARIANTS:
            if not gc.variant_applies(v, E, K):
                continue   # the variant computes the same thing there
            seed = gc.variant_seed(v, d_w)
            want = gc.route_backward_autograd(logits, K, seed, gc.AUX_COEF)[0]
            seen[v].append((mc.rel_l2(gc.route_backward_autograd(logits, K, seed, gc.AUX_COEF, variant=v)[0], want), E, K))
    for v, figs in seen.items():
        print("router gradient variant %s: %s" % (v, ", ".join("%.2e (E %d K %d)" % f for f in figs)))
        assert figs and min(f[0] for f in figs) > gc.MUTANT_FLOOR, v


def test_workspace_queries_need_no_device():
    L = _lib.load()
    for rows, width, E, K in ((27, 128, 4, 2), (8256, 768, 4, 2), (1300, 128, 64, 8)):
        fwd = L.mpreid_moe_workspace_bytes(rows, width, E, K)
        grad = L.mpreid_moe_grad_workspace_bytes(rows, width, E, K)
        route = L.mpreid_moe_route_backward_workspace_bytes(rows, E)
        slots = ((rows * K + 127) // 128 + E) * 128
        assert fwd > 0 and grad >= fwd + slots * 16 * width and 0 < route <= grad - fwd, (rows, width, E, K, fwd, grad, route)
    # outside the limits of the forward: 0
    assert L.mpreid_moe_grad_workspace_bytes(10, 100, 4, 2) == 0 and L.mpreid_moe_grad_workspace_bytes(10, 128, 65, 2) == 0
    assert L.mpreid_moe_grad_workspace_bytes(10, 128, 4, 5) == 0 and L.mpreid_moe_grad_workspace_bytes((1 << 20) + 1, 128, 4, 2) == 0
    assert L.mpreid_moe_route_backward_workspace_bytes(0, 4) == 0 and L.mpreid_moe_route_backward_workspace_bytes(10, 65) == 0


def test_refusals_come_before_a_device_is_asked_for():
    """a request for the expert matrices' own gradients names what is missing; bad shapes and a short workspace return their
    codes without a launch (dummy pointers are never dereferenced)"""
    L = _lib.load()
    p = C.c_void_p(0x1000)
    layer = _lib.MoeLayer(None, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000)
    lt = _lib.MoeLayerT(0x1000, 0x1000)
    eg = _lib.MoeExpertGrads(fc_w=0x1000)

    def call(rows=10, width=128, E=4, K=2, experts=None, ws=None, nbytes=0, layer_t=lt):
        return L.mpreid_moe_mlp_backward(p, rows, width, p, p, E, K, C.byref(layer), C.byref(layer_t), p, p, p, 0,
                                         None if experts is None else C.byref(experts), ws, nbytes, None)
    assert call(experts=eg) == _lib.ERR_UNSUPPORTED
    assert "expert matrices' own gradients are not implemented" in L.mpreid_last_error().decode()
    assert call(experts=_lib.MoeExpertGrads()) == -2 and "workspace too small" in L.mpreid_last_error().decode()
    assert call(E=65) == _lib.ERR_UNSUPPORTED and call(K=9, E=16) == _lib.ERR_UNSUPPORTED and call(width=100) == _lib.ERR_UNSUPPORTED
    assert call(layer_t=_lib.MoeLayerT(0x1000, 0)) == _lib.ERR_ARG
    assert call(layer_t=_lib.MoeLayerT(0x1004, 0x1000)) == _lib.ERR_ARG
    assert call(ws=C.c_void_p(0x1010), nbytes=1 << 40) == _lib.ERR_ARG          # the workspace: 256-byte aligned
    r = lambda **kw: L.mpreid_moe_route_backward(kw.get("lg", p), kw.get("rows", 10), kw.get("E", 4), kw.get("K", 2), p, p, p,
                                                 kw.get("coef", 0.01), p, p, None, 0, None)
    assert r() == -2 and r(E=65) == _lib.ERR_UNSUPPORTED and r(K=5) == _lib.ERR_UNSUPPORTED and r(lg=None) == _lib.ERR_ARG
    assert r(coef=float("nan")) == _lib.ERR_ARG and r(rows=0) == _lib.ERR_ARG
    with pytest.raises(NotImplementedError, match="expert matrices' own gradients are not implemented"):
        ops.moe_mlp_backward(None, None, None, None, None, None, 4, d_experts={"fc_w": torch.zeros(1)})



# ---- the tower ---------------------------------------------------------------------------------------------------------------
def _vit_cfg_structs(cfg, hw, batch=3):
    c = _lib.VitCfg(hw[0], hw[1], cfg["patch"], cfg["stride"], cfg["h_res"], cfg["w_res"], cfg["width"], cfg["layers"], cfg["heads"],
                    cfg["out_dim"], 0, 1, _lib.VIT_SPLIT)
    n_moe = mc.resolved_moe_layers(cfg)
    layers = (_lib.MoeLayer * n_moe)()
    return c, _lib.VitMoe(cfg["num_experts"], cfg["top_k"], n_moe, C.cast(layers, C.POINTER(_lib.MoeLayer))), layers


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_tower_restatement_against_the_references_golden(name):
    """tower() and tower_grads() against the REFERENCE's own MoE VisionTransformer under float64 autograd
    (tests/golden/moe_grad.npz): f_last (the last block's OUTPUT), f, f_proj, the logits, l_aux, every stored gradient of the
    three seeds and every gradient of l_aux alone within 1e-12; the parameters the reference's autograd leaves without .grad are
    exactly those tower_grads leaves at None, and l_aux reaches the same parameters"""
    dev = gc.golden_deviations(name)
    worst = max((d, k) for k, d in dev.items())
    print("%s against the reference's golden: largest deviation %.2e (%s) of %d figures; l_aux %.2e"
          % (name, *worst, len(dev), dev["l_aux"]))
    assert len(dev) > 60 and "d " + ops.VitEncoder.GATE_KEY in dev and "d cv_emb" in dev and "d_aux " + ops.VitEncoder.GATE_KEY in dev
    for k, d in dev.items():
        assert d <= gc.GOLDEN_BOUND, (name, k, d)


def test_load_balancing_loss_func_against_the_references_recorded_value():
    """the model's load_balancing_loss_func on the reference's recorded logits (its flat order; the function does not depend on
    the order of the rows) against the value the reference's own function returned for them, nothing lifted (`l_aux`)"""
    from model import make_model_uniprompt as mu
    z = np.load(gc.GOLDEN)
    for name in gc.GOLDEN_CASES:
        K = gc.TOWER_CASES[name][0]["top_k"]
        got = float(mu.load_balancing_loss_func(torch.from_numpy(z[name + "_logits"]), K))
        want = float(z[name + "_l_aux"])
        print("%s: load_balancing_loss_func %.12f, the reference's %.12f" % (name, got, want))
        assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("name", list(gc.TOWER_CASES))
def test_tower_cases_hold_their_routing_margin(name):
    c = gc.tower_case(name)
    print("%s: seed %d, smallest K / K+1 logit gap %.2e, fp32 restatement's logit error %.2e" % (name, c["seed"], c["margin"], c["err"]))
    assert c["margin"] >= mc.MARGIN_RATIO * c["err"]
    assert all(float(np.abs(s).max()) > 0 for s in c["seeds"]) and float(np.abs(c["cv"]).max()) > 0


def test_tower_restatement_equals_the_forward_restatement_of_moe_cases():
    """the differentiable restatement computes what moe_cases.tower_f64 (checked against the reference's golden vectors) does"""
    for name in gc.TOWER_CASES:
        c = gc.tower_case(name)
        ref = mc.tower_f64(c["cfg"], c["sd"], c["imgs"], cv_emb=c["cv"])
        mine = c["f64"]
        dev = max(float((torch.cat([mine[1], mine[2]], 1) - ref["feat"]).abs().max()), float((mine[3] - ref["logits"]).abs().max()))
        print("%s: largest deviation from moe_cases.tower_f64 %.2e" % (name, dev))
        assert dev <= 1e-12


@pytest.mark.parametrize("variant", gc.TOWER_WRONG_VARIANTS)
def test_tower_wrong_variants_clear_their_floor(variant):
    use = gc.tower_variant_use(variant)
    right = gc.tower_grads(gc.TOWER_VARIANT_CASE, use=use)
    wrong = gc.tower_grads(gc.TOWER_VARIANT_CASE, use=use, variant=variant)
    figs = []
    for k in (ops.VitEncoder.GATE_KEY, "tokens"):
        w = wrong[k] if wrong[k] is not None else torch.zeros_like(right[k])
        figs.append(mc.rel_l2(w, right[k]))
    print("tower variant %s: gate.weight %.2e tokens %.2e" % (variant, *figs))
    assert min(figs) > gc.MUTANT_FLOOR


def test_later_gates_and_experts_get_no_gradient_under_autograd():
    g = gc.tower_grads("reduced")
    assert g["transformer.resblocks.1.gate.weight"] is None and g[ops.VitEncoder.GATE_KEY] is not None


def test_tower_workspace_queries_answer_without_a_device_and_exceed_the_dense_ones():
    L = _lib.load()
    for name in ("reduced", "full"):
        cfg, hw = gc.TOWER_CASES[name][0], gc.TOWER_CASES[name][1]
        c, moe, keep = _vit_cfg_structs(cfg, hw)
        dense_b = L.mpreid_vit_backward_workspace_bytes(C.byref(c), 3)
        moe_b = L.mpreid_vit_backward_moe_workspace_bytes(C.byref(c), C.byref(moe), 3)
        rows = 3 * (cfg["h_res"] * cfg["w_res"] + 1)
        assert dense_b > 0 and moe_b >= dense_b + L.mpreid_moe_grad_workspace_bytes(rows, cfg["width"], cfg["num_experts"], cfg["top_k"])
        fwd = L.mpreid_vit_workspace_bytes_moe(C.byref(c), C.byref(moe), 3)
        assert L.mpreid_vit_forward_train_moe_workspace_bytes(C.byref(c), C.byref(moe), 3) > fwd > 0
        none = _lib.VitMoe(cfg["num_experts"], cfg["top_k"], 0, None)
        assert L.mpreid_vit_backward_moe_workspace_bytes(C.byref(c), C.byref(none), 3) == 0


# mpreid_vit_backward_moe_workspace_bytes with (E, K, moe_layers) = (2, 1, 1) and (4, 2, 2), as the library answered before both
# sweeps took their shared regions (x_l, dx, dh, t, dqkv) through one definition.  "small" is SMALL of
# tests/test_gpu_tower_launches.py at 64 x 32, "full" ViT-B/16 at 256 x 128; both in the split precision
SMALL_VIT = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
BACKWARD_MOE_WORKSPACE_BYTES = {("small", 1): (5866240, 7047936), ("small", 3): (5977344, 7159552), ("small", 64): (18457088, 22022912),
                                ("full", 1): (46566400, 57190912), ("full", 3): (85973760, 103687424),
                                ("full", 64): (1302221312, 1536156928)}


@pytest.mark.parametrize("size,batch", sorted(BACKWARD_MOE_WORKSPACE_BYTES))
def test_tower_backward_workspace_bytes(size, batch):
    from mpreid import synth
    L = _lib.load()
    cfg, hw = (SMALL_VIT, (64, 32)) if size == "small" else (synth.VIT_B16, (256, 128))
    got = []
    for E, K, n_moe in ((2, 1, 1), (4, 2, 2)):
        c, moe, keep = _vit_cfg_structs(dict(cfg, num_experts=E, top_k=K, moe_layers=n_moe), hw)
        got.append(L.mpreid_vit_backward_moe_workspace_bytes(C.byref(c), C.byref(moe), batch))
    assert tuple(got) == BACKWARD_MOE_WORKSPACE_BYTES[(size, batch)]


def test_masters_of_an_moe_tower_and_the_host_refusals():
    """the masters are the dense parameters and block 0's gate: no later gate, no expert, no mlp.* of an MoE block; an expert
    that requires grad is refused by name; the model's opt-in refuses a dense tower"""
    enc = object.__new__(ops.VitEncoder)
    enc.cfg, enc.precision, enc.masters = dict(layers=3, width=128), "split", None
    enc.c_moe = _lib.VitMoe(4, 2, 2, None)
    keys = [k for k, _, _ in enc._param_fields()]
    assert ops.VitEncoder.GATE_KEY in keys and not any(".experts." in k for k in keys)
    assert not any(".gate." in k for k in keys if k != ops.VitEncoder.GATE_KEY)
    assert "transformer.resblocks.2.mlp.c_fc.weight" in keys and not any(k.startswith("transformer.resblocks.0.mlp.") or
                                                                        k.startswith("transformer.resblocks.1.mlp.") for k in keys)
    bad = {"image_encoder.transformer.resblocks.0.experts.0.c_fc.weight": torch.zeros(2, 2, requires_grad=True)}
    with pytest.raises(NotImplementedError, match="expert matrices' own gradients are not implemented"):
        enc.enable_training(bad)
    enc.c_moe = None
    assert len([k for k, _, _ in enc._param_fields()]) == 8 + 3 * 12
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["INPUT.SIZE_TRAIN", [32, 32], "INPUT.SIZE_TEST", [32, 32]])
    with pytest.raises(ValueError, match="no MoE block"):
        mu.make_model(cfg, num_class=3, camera_num=1, view_num=1).enable_stage2_moe_training()
    lg = torch.randn(40, 4, dtype=torch.float64)
    assert mu.LOAD_BALANCE_LOSS_COEFF == 0.01
