"""The MoE gradient seams on the GPU: the gradient through one routed MLP against float64 autograd with caller-made routing, on
exact integers, with NULL outputs and the accumulate flag; the router's gradient and the load-balancing loss against float64,
its exact zeros, the forward's tie rule; wrong variants; refusals.  Cases and references: tests/moe_grad_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import moe_cases as mc
import moe_grad_cases as gc
from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu
WIDTH = 128


# ---- 1. the gradient through one routed MLP ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mlp_cases():
    """kind -> dict of the inputs, the packed layers and the float64 gradients, computed once"""
    cache = {}

    def get(kind):
        if kind in cache:
            return cache[kind]
        sel, w = gc.mlp_routing(kind)
        rows, K = sel.shape
        rng = np.random.default_rng(11)
        h = rng.standard_normal((rows, WIDTH)).astype(np.float32)
        dy = rng.standard_normal((rows, WIDTH)).astype(np.float32)
        used = np.zeros(gc.MLP_E, bool)
        used[np.unique(sel)] = True
        wt = gc.mlp_weights(gc.MLP_E, WIDTH, rng, nan_unused=np.nonzero(~used)[0])
        want_a, want_w = gc.mlp_backward_autograd(h, sel, w, *wt, dy)
        layer, keep = ops.pack_moe_layer(*wt)
        layer_t, keep_t = ops.pack_moe_layer_t(wt[0], wt[2])
        cache[kind] = dict(sel=torch.from_numpy(sel).cuda(), w=torch.from_numpy(w).cuda(), rows=rows, K=K,
                           a=ops.split_pairs_f32(torch.from_numpy(h)), dy=torch.from_numpy(dy).cuda(), layer=layer, layer_t=layer_t,
                           keep=(keep, keep_t), want_a=want_a, want_w=want_w)
        return cache[kind]
    return get


def _run_mlp(c, **kw):
    return ops.moe_mlp_backward(c["a"], c["sel"], c["w"], c["layer"], c["layer_t"], c["dy"], gc.MLP_E, **kw)


@pytest.mark.parametrize("kind", gc.MLP_KINDS)
def test_mlp_backward_against_float64(mlp_cases, kind):
    """d_a and d_w within 2e-5 (relative L2) of float64 autograd; NaN weights of the empty experts reach nothing; guard rows of
    both outputs and guard bytes behind the workspace keep their contents; a second call gives the same bits"""
    c = mlp_cases(kind)
    rows, K = c["rows"], c["K"]
    need = _lib.load().mpreid_moe_grad_workspace_bytes(rows, WIDTH, gc.MLP_E, K)
    assert need > 0
    wsbuf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    d_a = torch.full((rows + 5, WIDTH), 7.0, device="cuda")
    d_w = torch.full((rows + 5, K), 7.0, device="cuda")
    _run_mlp(c, d_a=d_a, d_w=d_w, ws=wsbuf[:need])
    torch.cuda.synchronize()
    got_a, got_w = d_a[:rows].cpu(), d_w[:rows].cpu()
    assert bool(torch.isfinite(got_a).all()) and bool(torch.isfinite(got_w).all())
    assert bool((d_a[rows:] == 7.0).all()) and bool((d_w[rows:] == 7.0).all()) and bool((wsbuf[need:] == 0xA5).all())
    ra, rw = mc.rel_l2(got_a, c["want_a"]), mc.rel_l2(got_w, c["want_w"])
    print("routed MLP backward %s: d_a %.3e d_w %.3e" % (kind, ra, rw))
    assert ra <= gc.BOUND and rw <= gc.BOUND
    again_a, again_w = _run_mlp(c)
    assert torch.equal(again_a.cpu(), got_a) and torch.equal(again_w.cpu(), got_w)


def test_mlp_backward_null_outputs_and_accumulate(mlp_cases):
    """either output alone has the bits it has beside the other; the accumulate flag adds with one rounded add per entry"""
    c = mlp_cases("k2_hole")
    both_a, both_w = _run_mlp(c)
    only_a, none_w = _run_mlp(c, want_d_w=False)
    none_a, only_w = _run_mlp(c, want_d_a=False)
    assert none_w is None and none_a is None
    assert torch.equal(only_a, both_a) and torch.equal(only_w, both_w)
    base = torch.from_numpy(np.random.default_rng(2).standard_normal((c["rows"], c["K"])).astype(np.float32)).cuda()
    acc = base.clone()
    _run_mlp(c, d_w=acc, accumulate_d_w=True, want_d_a=False)
    assert torch.equal(acc, base + both_w)
    acc2 = base.clone()
    _run_mlp(c, d_w=acc2, accumulate_d_w=False, want_d_a=False)
    assert torch.equal(acc2, both_w)


def test_mlp_backward_on_exact_integers():
    """c_fc: zero weights, bias +32 on eight hidden units (QuickGELU = 32, slope exactly 1), -1024 on eight more (QuickGELU = -0 and
    slope exactly 0) and 0 elsewhere (slope 0.5, but c_proj is zero there); c_proj: integer weights in -4 .. 4 on those sixteen
    units; w in {0.25, 0.75}; dy small integers.  Then y, d_w = <dy, y> and dt = (w dy) . Wproj are exact in fp32.  d_w must
    equal the float64 result to the bit.  c_fc's weights are zero, so d_a must be exactly zero; with integer c_fc rows on the
    live units (second part) d_a must equal the float64 result to the bit as well."""
    E, K, rows = 4, 2, 200
    rng = np.random.default_rng(5)
    units = rng.choice(4 * WIDTH, 16, replace=False)
    on, off = units[:8], units[8:]
    sel = np.stack([rng.permutation(E).astype(np.int32)[:K] for _ in range(rows)])
    w = np.where(rng.random((rows, 1)) < 0.5, np.array([[0.25, 0.75]], np.float32), np.array([[0.75, 0.25]], np.float32)).astype(np.float32)
    dy = rng.integers(-3, 4, size=(rows, WIDTH)).astype(np.float32)
    for part in (0, 1):
        fc_w = np.zeros((E, 4 * WIDTH, WIDTH), np.float32)
        fc_b = np.zeros((E, 4 * WIDTH), np.float32)
        fc_b[:, on] = 32.0
        fc_b[:, off] = -1024.0
        h = rng.standard_normal((rows, WIDTH)).astype(np.float32)
        if part == 1:   # h = 0 keeps u = the bias whatever c_fc holds, so the slopes stay exactly 1 / 0
            h[:] = 0.0
            fc_w[:, units, :] = rng.integers(-4, 5, size=(E, 16, WIDTH)).astype(np.float32)
            fc_w[:, units[0], 0] = 4.0
        proj_w = np.zeros((E, WIDTH, 4 * WIDTH), np.float32)
        proj_w[:, :, units] = rng.integers(-4, 5, size=(E, WIDTH, 16)).astype(np.float32)
        proj_w[:, 0, units[0]] = 4.0   # the largest entry is 4 in every expert: exact power-of-two scales
        proj_b = rng.integers(-8, 9, size=(E, WIDTH)).astype(np.float32)
        want_a, want_w = gc.mlp_backward_autograd(h, sel, w, fc_w, fc_b, proj_w, proj_b, dy)
        layer, keep = ops.pack_moe_layer(fc_w, fc_b, proj_w, proj_b)
        layer_t, keep_t = ops.pack_moe_layer_t(fc_w, proj_w)
        d_a, d_w = ops.moe_mlp_backward(ops.split_pairs_f32(torch.from_numpy(h)), torch.from_numpy(sel).cuda(),
                                        torch.from_numpy(np.ascontiguousarray(w)).cuda(), layer, layer_t, torch.from_numpy(dy).cuda(), E)
        assert torch.equal(d_w.cpu().double(), want_w), part
        assert torch.equal(d_a.cpu().double(), want_a), part
        if part == 0:
            assert float(d_a.abs().max()) == 0.0
        else:
            assert float(want_a.abs().max()) > 0.0


# ---- 2. the router's gradient ---------------------------------------------------------------------------------------------
def _device_routing(logits, K):
    """sel / w / logits of the forward's router for given logits: h carries them in its first E columns and the gate is the
    first E rows of the identity, so every logit is reproduced exactly"""
    rows, E = logits.shape
    h = np.zeros((rows, WIDTH), np.float32)
    h[:, :E] = logits
    gate = np.eye(WIDTH, dtype=np.float32)[:E]
    sel, w, lg = ops.moe_route(torch.from_numpy(h), torch.from_numpy(gate), K, want_logits=True)
    assert torch.equal(lg.cpu(), torch.from_numpy(logits))
    return sel, w, lg


@pytest.mark.parametrize("E,K", gc.ROUTE_EK)
def test_route_backward_against_float64(E, K):
    """d_logits (routing term alone, load-balancing term alone, both) and l_aux within 2e-5 of float64 autograd at 1300 rows;
    coef == 0: entries off the selection are exactly zero, K == 1: all of them; coef changes no bit of l_aux; guard bytes behind
    the workspace keep their contents; a second call gives the same bits"""
    logits, d_w = gc.route_case(E, K)
    rows = logits.shape[0]
    sel, w, lg = _device_routing(logits, K)
    d_w_dev = torch.from_numpy(d_w).cuda()
    need = _lib.load().mpreid_moe_route_backward_workspace_bytes(rows, E)
    wsbuf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    l_aux_bits = None
    for what, seed, coef in (("routing", d_w_dev, 0.0), ("aux", None, gc.AUX_COEF), ("both", d_w_dev, gc.AUX_COEF)):
        want, want_l, want_sel, _ = gc.route_backward_autograd(logits, K, d_w if seed is not None else np.zeros_like(d_w), coef)
        assert torch.equal(sel.cpu().long(), want_sel)
        got, l_aux = ops.moe_route_backward(lg, sel, w, seed, coef, ws=wsbuf[:need])
        torch.cuda.synchronize()
        assert bool((wsbuf[need:] == 0xA5).all())
        g = got.cpu().double()
        if float(want.abs().max()) == 0.0 or (what == "routing" and K == 1):
            assert float(g.abs().max()) == 0.0, (what, "exact zeros")   # K == 1, or K == E for the load-balancing term: see below
        elif what == "aux" and K == E:
            # f_e = 1 for every e: g is uniform and p (g - sum p g) is rounding only; judged against the term's own scale
            assert float(g.abs().max()) <= 1e-6 * coef * E / rows
        else:
            rel = mc.rel_l2(g, want)
            print("router gradient E %d K %d %s: %.3e" % (E, K, what, rel))
            assert rel <= gc.BOUND, (what, rel)
        rl = abs(float(l_aux.cpu().double()) - float(want_l)) / float(want_l)
        assert rl <= gc.BOUND, (what, rl)
        if l_aux_bits is None:
            l_aux_bits = l_aux.clone()
        assert torch.equal(l_aux, l_aux_bits)
        if coef == 0.0:
            off = torch.ones_like(g, dtype=torch.bool).scatter_(1, want_sel, False)
            assert not off.any() or float(g[off].abs().max()) == 0.0
        again, l2 = ops.moe_route_backward(lg, sel, w, seed, coef)
        assert torch.equal(again, got) and torch.equal(l2, l_aux)
    only_l = ops.moe_route_backward(lg, sel, w, d_w_dev, gc.AUX_COEF, want_d_logits=False)
    assert only_l[0] is None and torch.equal(only_l[1], l_aux_bits)
    only_d = ops.moe_route_backward(lg, sel, w, d_w_dev, gc.AUX_COEF, want_l_aux=False)
    assert only_d[1] is None and torch.equal(only_d[0], got)


def test_route_backward_follows_the_forwards_tie_rule():
    """integer logits in -2 .. 2 over 8 experts: exact ties on most rows.  The device router's selection (lower index first)
    is the one the gradient is laid on: d_logits equals the float64 closed form for that selection, and entries of tied but
    unselected experts stay exactly zero with coef == 0"""
    E, K, rows = 8, 2, 257
    rng = np.random.default_rng(9)
    logits = rng.integers(-2, 3, size=(rows, E)).astype(np.float32)
    d_w = rng.standard_normal((rows, K)).astype(np.float32)
    sel, w, lg = _device_routing(logits, K)
    want_sel = mc.topk_lower_first(torch.from_numpy(logits).double(), K)
    assert torch.equal(sel.cpu().long(), want_sel)
    s = np.sort(logits, -1)[:, ::-1]
    assert int((s[:, K - 1] == s[:, K]).sum()) > rows // 4   # the tie at the selection's edge is common
    got, _ = ops.moe_route_backward(lg, sel, w, torch.from_numpy(d_w).cuda(), 0.0)
    want, _ = gc.route_backward_closed(logits, want_sel, w.cpu(), d_w, 0.0)
    assert mc.rel_l2(got.cpu(), want) <= gc.BOUND
    off = torch.ones((rows, E), dtype=torch.bool).scatter_(1, want_sel, False)
    assert float(got.cpu()[off].abs().max()) == 0.0


@pytest.mark.parametrize("variant", gc.ROUTE_WRONG_VARIANTS)
def test_wrong_variants_are_far_from_the_device_gradient(variant):
    far = []
    for E, K in gc.ROUTE_EK:
        if not gc.variant_applies(variant, E, K):
            continue
        logits, d_w = gc.route_case(E, K, rows=300)
        seed = gc.variant_seed(variant, d_w)
        sel, w, lg = _device_routing(logits, K)
        got, _ = ops.moe_route_backward(lg, sel, w, torch.from_numpy(seed).cuda(), gc.AUX_COEF)
        wrong = gc.route_backward_autograd(logits, K, seed, gc.AUX_COEF, variant=variant)[0]
        far.append(mc.rel_l2(got.cpu(), wrong) if float(wrong.abs().max()) > 0 else float(got.abs().max() > 0))
    print("device vs variant %s: %s" % (variant, ", ".join("%.2e" % f for f in far)))
    assert far and max(far) > gc.MUTANT_FLOOR


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------
def test_refused_calls_return_their_codes_and_leave_the_next_call_intact(mlp_cases):
    c = mlp_cases("k2_hole")
    L = _lib.load()
    good_a, good_w = _run_mlp(c)
    rows, K = c["rows"], c["K"]
    need = L.mpreid_moe_grad_workspace_bytes(rows, WIDTH, gc.MLP_E, K)
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    d_a, d_w = torch.zeros_like(good_a), torch.zeros_like(good_w)

    def call(ws_ptr=ws.data_ptr(), nbytes=need, E=gc.MLP_E, d_a_ptr=d_a.data_ptr(), experts=None):
        return L.mpreid_moe_mlp_backward(c["a"].data_ptr(), rows, WIDTH, c["sel"].data_ptr(), c["w"].data_ptr(), E, K,
                                         C.byref(c["layer"]), C.byref(c["layer_t"]), c["dy"].data_ptr(), d_a_ptr, d_w.data_ptr(), 0,
                                         experts, ws_ptr, nbytes, _lib.stream_ptr())
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(ws_ptr=ws.data_ptr() + 16) == _lib.ERR_ARG
    assert call(d_a_ptr=d_a.data_ptr() + 4) == _lib.ERR_ARG
    assert call(E=65) == _lib.ERR_UNSUPPORTED
    assert call(experts=C.byref(_lib.MoeExpertGrads(proj_w=d_a.data_ptr()))) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(d_a.abs().max()) == 0.0 and float(d_w.abs().max()) == 0.0   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(d_a, good_a) and torch.equal(d_w, good_w)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.moe_route_backward(torch.zeros((10, 4), device="cuda"), torch.zeros((10, 2), dtype=torch.int32, device="cuda"),
                               torch.zeros((10, 2), device="cuda"), None, 0.01, ws=torch.empty(256, dtype=torch.uint8, device="cuda")[:0])


# ---- 4. the tower -----------------------------------------------------------------------------------------------------------
GATE = ops.VitEncoder.GATE_KEY


@pytest.fixture(scope="module")
def towers():
    """name -> (case, encoder with masters, images and cv_emb on the device), built once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = gc.tower_case(name)
            enc = ops.VitEncoder(c["cfg"], c["sd"], c["hw"], ws_tag="moe_grad_" + name)
            enc.enable_training()
            cache[name] = (c, enc, torch.from_numpy(c["imgs"]).cuda(), torch.from_numpy(c["cv"]).cuda())
        return cache[name]
    return get


def _seeds(c, use=(True, True, True), scale=1.0):
    return [torch.from_numpy(d * np.float32(scale)).cuda() if u else None for d, u in zip(c["seeds"], use)]


def _all_names(enc):
    return [k for k, _, _ in enc._param_fields()] + ["cv_emb", "tokens"]


def _compare(out, want, what):
    """every tensor within the bound of float64; a tensor whose float64 gradient is exactly zero must be exactly zero"""
    worst = (0.0, None)
    for k, got in out.items():
        w = want[k]
        if w is None or float(w.abs().max()) == 0.0:   # (None: the function does not reach the tensor under these seeds)
            assert float(got.abs().max()) == 0.0, (what, k, "exact zero expected")
            continue
        rel = mc.rel_l2(got.reshape(w.shape), w)
        worst = max(worst, (rel, k))
        assert rel <= gc.BOUND, (what, k, rel)
    return worst


@pytest.mark.parametrize("name", list(gc.TOWER_CASES))
def test_tower_training_forward(towers, name):
    """f_last (the CLS row of the last block's OUTPUT), f, f_proj, the router logits and l_aux within 2e-5 of float64; f | f_proj
    carry the bits of forward(); the selection equals float64's on every token"""
    c, enc, imgs, cv = towers(name)
    f_last, f, f_proj, logits, l_aux = enc.forward_train(imgs, cv, want_router=True)
    want = c["f64"]
    rels = [mc.rel_l2(g, w) for g, w in zip((f_last, f, f_proj, logits), want[:4])]
    rl = abs(float(l_aux) - float(want[4])) / float(want[4])
    print("training forward %s: f_last %.2e f %.2e f_proj %.2e logits %.2e l_aux %.2e" % (name, *rels, rl))
    assert max(rels) <= gc.BOUND and rl <= gc.BOUND
    assert torch.equal(torch.cat([f, f_proj], 1), enc(imgs, cv))
    three = enc.forward_train(imgs, cv)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, (f_last, f, f_proj)))
    K = c["cfg"]["top_k"]
    assert torch.equal(mc.topk_lower_first(logits.cpu().double(), K).sort(-1).values, mc.topk_lower_first(want[3], K).sort(-1).values)


@pytest.mark.parametrize("name", list(gc.TOWER_CASES))
def test_tower_gradients_against_float64(towers, name):
    """every master (block 0's gate among them), cv_emb and tokens within 2e-5 per tensor of float64 autograd of
    sum(f_last o d1) + sum(f o d2) + sum(f_proj o d3) + 0.01 l_aux; fp32 autograd on the host beside it; a second call gives the
    same bits.  `aligned` (16 images, 144 token rows: every weight-gradient GEMM on the exact fp32 GEMM's fast staging), measured
    on an MI355X: device worst 8.6e-7 (block 0's gate), fp32 autograd on the host 2.0e-6"""
    c, enc, imgs, cv = towers(name)
    want = gc.tower_grads(name)
    out = enc.backward(imgs, cv, *_seeds(c), want=_all_names(enc), aux_coef=gc.AUX_COEF)
    worst = _compare(out, want, name)
    w32 = gc.tower_grads(name, dtype=torch.float32)
    host = max((mc.rel_l2(w32[k], want[k]), k) for k in out if float(want[k].abs().max()) > 0)
    print("tower gradients %s: device worst %.3e (%s); fp32 autograd on the host worst %.3e (%s)" % (name, *worst, *host))
    again = enc.backward(imgs, cv, *_seeds(c), want=_all_names(enc), aux_coef=gc.AUX_COEF)
    assert all(torch.equal(again[k], out[k]) for k in out)
    assert GATE in out and not any(".experts." in k or (".gate." in k and k != GATE) for k in enc.masters)


@pytest.mark.parametrize("use,coef", [((True, False, False), 0.0), ((False, True, False), 0.0), ((False, False, True), 0.0),
                                      ((False, False, False), gc.AUX_COEF)])
def test_tower_each_seed_alone_and_the_aux_term_alone(towers, use, coef):
    """each seed alone, then only aux_coef non-zero: within the bound wherever float64 is non-zero and exactly zero wherever it
    is -- with the aux term alone that is every tensor behind block 0's ln_2 (blocks 1 .., ln_post, proj)"""
    c, enc, imgs, cv = towers("reduced")
    want = gc.tower_grads("reduced", use=use, coef=coef)
    out = enc.backward(imgs, cv, *_seeds(c, use), want=_all_names(enc), aux_coef=coef)
    worst = _compare(out, want, (use, coef))
    print("tower gradients reduced, seeds %s coef %g: worst %.3e (%s)" % (use, coef, *worst))
    if not any(use):
        behind = [k for k in out if k.startswith(("transformer.resblocks.1.", "transformer.resblocks.2.", "ln_post", "proj"))]
        assert len(behind) > 20 and all(float(out[k].abs().max()) == 0.0 for k in behind)
        assert float(out[GATE].abs().max()) > 0.0 and float(out["tokens"].abs().max()) > 0.0


def test_tower_null_members_zero_seeds_and_homogeneity(towers):
    """asking for fewer gradients changes no bit of the others; all-zero seeds with coef == 0 give zeros; seeds scaled by 2^-40
    (coef == 0) scale every gradient by exactly 2^-40"""
    c, enc, imgs, cv = towers("reduced")
    names = _all_names(enc)
    full = enc.backward(imgs, cv, *_seeds(c), want=names, aux_coef=0.0)
    for sub in ([GATE], ["tokens"], ["cv_emb", "conv1.weight", "transformer.resblocks.0.ln_2.weight"],
                ["transformer.resblocks.2.mlp.c_fc.weight", "transformer.resblocks.1.attn.in_proj_weight"]):
        part = enc.backward(imgs, cv, *_seeds(c), want=sub, aux_coef=0.0)
        assert sorted(part) == sorted(sub) and all(torch.equal(part[k], full[k]) for k in sub), sub
    zero = enc.backward(imgs, cv, *[torch.zeros_like(s) for s in _seeds(c)], want=names, aux_coef=0.0)
    assert all(float(v.abs().max()) == 0.0 for v in zero.values())
    small = enc.backward(imgs, cv, *_seeds(c, scale=2.0 ** -40), want=names, aux_coef=0.0)
    assert all(torch.equal(small[k] * 2.0 ** 40, full[k]) for k in names)


def test_tower_single_expert_equals_the_dense_tower_bit_for_bit():
    """every block an MoE block whose single expert holds the dense MLP (moe_cases.dense_as_single_expert): f | f_proj of the
    training forward and every shared gradient equal the dense tower's BIT FOR BIT (seeds on f and f_proj: f_last differs by
    definition); d gate.weight is exactly zero"""
    cfg = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=3, heads=2, out_dim=64)
    sd = synth.vit_state_dict(cfg, seed=77, std=0.05, ln_jitter=0.1)
    moe_cfg = dict(cfg, num_experts=1, top_k=1, moe_layers=-1)
    imgs = torch.from_numpy(synth.synthetic_images(5, 64, 32, seed=78)).cuda()
    rng = np.random.default_rng(79)
    cv = torch.from_numpy((rng.standard_normal((5, 128)) * 0.05).astype(np.float32)).cuda()
    d_f = torch.from_numpy((rng.standard_normal((5, 128)) * 0.1).astype(np.float32)).cuda()
    d_fp = torch.from_numpy((rng.standard_normal((5, 64)) * 0.1).astype(np.float32)).cuda()
    dense = ops.VitEncoder(cfg, sd, (64, 32), ws_tag="moe_grad_dense")
    moe = ops.VitEncoder(moe_cfg, mc.dense_as_single_expert(sd, cfg["layers"]), (64, 32), ws_tag="moe_grad_e1")
    dense.enable_training(), moe.enable_training()
    fd, fm = dense.forward_train(imgs, cv), moe.forward_train(imgs, cv)
    assert torch.equal(fd[1], fm[1]) and torch.equal(fd[2], fm[2])
    shared = [k for k in _all_names(moe) if k != GATE]
    gd = dense.backward(imgs, cv, None, d_f, d_fp, want=shared)
    gm = moe.backward(imgs, cv, None, d_f, d_fp, want=shared + [GATE], aux_coef=gc.AUX_COEF)
    diff = [k for k in shared if not torch.equal(gd[k], gm[k])]
    assert not diff, diff
    assert float(gm[GATE].abs().max()) == 0.0
    # f_last differs from the dense tower's by definition (the last block's OUTPUT): it, and the gradients of its seed alone,
    # against float64 autograd of the MoE restatement
    moe_sd = mc.dense_as_single_expert(sd, cfg["layers"])
    g64 = {k: mc._t64(v).clone().requires_grad_(True) for k, v in moe_sd.items()}
    cv64 = cv.cpu().double().requires_grad_(True)
    taps = {}
    f_last64 = gc.tower(moe_cfg, g64, imgs.cpu().double(), cv64, taps)[0]
    assert mc.rel_l2(fm[0], f_last64) <= gc.BOUND and mc.rel_l2(fd[0], f_last64) > 100 * gc.BOUND
    d_fl = torch.from_numpy((rng.standard_normal((5, 128)) * 0.1).astype(np.float32)).cuda()
    (f_last64 * d_fl.cpu().double()).sum().backward()
    gl = moe.backward(imgs, cv, d_fl, None, None, want=["cv_emb", "tokens", "transformer.resblocks.2.ln_2.weight"])
    for k, w in (("cv_emb", cv64.grad), ("tokens", taps["tokens"].grad), ("transformer.resblocks.2.ln_2.weight",
                                                                           g64["transformer.resblocks.2.ln_2.weight"].grad)):
        assert mc.rel_l2(gl[k], w) <= gc.BOUND, k


def test_tower_an_image_has_the_same_gradient_bits_in_any_batch(towers):
    """image 7 alone and inside the 40-image batch (1320 token rows): the same cv_emb and tokens gradient bits (coef == 0: l_aux
    is a function of the whole batch)"""
    c, enc, imgs, cv = towers("rows1320")
    seeds = _seeds(c)
    big = enc.backward(imgs, cv, *seeds, want=["cv_emb", "tokens"], aux_coef=0.0)
    one = enc.backward(imgs[7:8], cv[7:8], *[s[7:8].contiguous() for s in seeds], want=["cv_emb", "tokens"], aux_coef=0.0)
    assert torch.equal(one["cv_emb"][0], big["cv_emb"][7]) and torch.equal(one["tokens"][0], big["tokens"][7])


@pytest.mark.parametrize("variant", gc.TOWER_WRONG_VARIANTS)
def test_tower_wrong_variants_are_far_from_the_device_gradients(towers, variant):
    c, enc, imgs, cv = towers(gc.TOWER_VARIANT_CASE)
    use = gc.tower_variant_use(variant)
    wrong = gc.tower_grads(gc.TOWER_VARIANT_CASE, use=use, variant=variant)
    out = enc.backward(imgs, cv, *_seeds(c, use), want=[GATE, "tokens"], aux_coef=gc.AUX_COEF)
    far = []
    for k in (GATE, "tokens"):
        w = wrong[k] if wrong[k] is not None else torch.zeros_like(out[k]).cpu().double()
        far.append(float((out[k].cpu().double() - w).norm() / out[k].cpu().double().norm()))
    print("device vs tower variant %s: gate %.2e tokens %.2e" % (variant, *far))
    assert max(far) > gc.MUTANT_FLOOR


def test_forward_grad_under_autograd_equals_backward(towers):
    """forward_grad's five outputs drive torch.autograd: the gradient that reaches l_aux is the coefficient, the logits are data;
    every master's .grad and cv_emb's equal backward()'s bits; later gates and experts are no masters"""
    c, enc, imgs, cv = towers("reduced")
    seeds = _seeds(c)
    cv_t = cv.clone().requires_grad_(True)
    f_last, f, f_proj, logits, l_aux = enc.forward_grad(imgs, cv_t)
    assert not logits.requires_grad and l_aux.requires_grad
    loss = (f_last * seeds[0]).sum() + (f * seeds[1]).sum() + (f_proj * seeds[2]).sum() + gc.AUX_COEF * l_aux.sum()
    loss.backward()
    names = [k for k, _, _ in enc._param_fields()]
    want = enc.backward(imgs, cv, *seeds, want=names + ["cv_emb"], aux_coef=gc.AUX_COEF)
    try:
        assert all(torch.equal(enc.masters[k].grad, want[k]) for k in names) and torch.equal(cv_t.grad, want["cv_emb"])
    finally:
        for k in names:
            enc.masters[k].grad = None


def test_tower_refusals(towers):
    """an expert that requires grad, an fp16 tower, a tower without an MoE block at the MoE entry points"""
    c, enc, imgs, cv = towers("reduced")
    key = "transformer.resblocks.0.experts.1.c_fc.weight"
    masters = dict(enc.masters)
    masters[key] = torch.zeros((4 * 128, 128), device="cuda", requires_grad=True)
    other = ops.VitEncoder(c["cfg"], c["sd"], c["hw"], ws_tag="moe_grad_refuse")
    with pytest.raises(NotImplementedError, match="expert matrices' own gradients are not implemented"):
        other.enable_training(masters)
    dense_cfg = {k: v for k, v in c["cfg"].items() if k not in ("num_experts", "top_k", "moe_layers")}
    sd = synth.vit_state_dict(dense_cfg, seed=3, std=0.05)
    with pytest.raises(NotImplementedError):
        ops.VitEncoder(dense_cfg, sd, c["hw"], precision="fp16", ws_tag="moe_grad_fp16").enable_training()
    L = _lib.load()
    none = _lib.VitMoe(4, 2, 0, None)
    assert L.mpreid_vit_backward_moe_workspace_bytes(C.byref(enc.c_cfg), C.byref(none), 3) == 0
    assert L.mpreid_vit_forward_train_moe_workspace_bytes(C.byref(enc.c_cfg), C.byref(none), 3) == 0
    good = enc.backward(imgs, cv, *_seeds(c), want=[GATE], aux_coef=0.0)
    assert bool(torch.isfinite(good[GATE]).all())


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,K", gc.E2E_EK)
def test_twenty_fused_steps_on_a_small_moe_model(E, K):
    """20 Stage2Trainer.steps (SGD) on the reduced tower with 2 of 3 blocks MoE against the same loop in float64: the loss falls on
    both; the reported loss is the head's + 0.01 * l_aux (step 1 within 2e-5 of float64, where the routing margin holds); the
    largest deviation over the curve is printed (a routing decision may flip once the parameters move: no bound is set on it);
    the experts and the later gates keep their bits, block 0's gate moves"""
    import stage1_cases as sc
    import stage2_head_cases as hc
    import stage2_train_cases as s2
    s, c = gc.e2e_setup(E, K), s2.TRAIN
    enc = ops.VitEncoder(s["cfg"], s["sd"], c["img_hw"], ws_tag="moe_e2e_%d" % E)
    masters = enc.enable_training()
    gate0 = masters[GATE].detach().clone()
    h = {k: torch.from_numpy(v).cuda() for k, v in s["head"].items() if v.dtype == np.float32}

    def bn(name):
        return dict(weight=h[name + ".weight"], bias=h[name + ".bias"], running_mean=h[name + ".running_mean"],
                    running_var=h[name + ".running_var"], num_batches_tracked=torch.zeros((), dtype=torch.long, device="cuda"))
    head = ops.Stage2Head(h["classifier.weight"], h["classifier_proj.weight"], bn("bottleneck"), bn("bottleneck_proj"))
    tensors = dict(masters)
    tensors.update({k: h[k] for k in hc.PARAMS})
    groups = [{"params": [t], "lr": c["sgd_lr"] * s2.group_of(k)[0], "weight_decay": s2.group_of(k)[1]} for k, t in tensors.items()]
    opt = ops.TensorOptimizer(groups, "SGD", betas=(sc.BETA1, sc.BETA2), eps=sc.EPS, momentum=c["sgd_mu"])
    tr = ops.Stage2Trainer(enc, head, opt, h["text"])
    assert tr.aux_coef == 0.01 and GATE in tr.grads and sorted(list(tr.grads) + list(s2.HEAD_BOUND)) == sorted(gc.e2e_trained_names(s))
    img, target = torch.from_numpy(s["imgs"]).cuda(), torch.from_numpy(s["head"]["target"]).cuda()
    # what the steps could move and must not: every device tensor the encoder holds that is no master -- the experts' fp16 pairs,
    # scales and biases and their fp32 transposed copies among them -- and the addresses the MoE structs point at.  The gates of
    # later blocks are not on the device at all: the encoder never reads them, and no tensor of the optimizer is one.
    mine = {t.data_ptr() for t in masters.values()}
    held = [t for t in enc._keep if torch.is_tensor(t) and t.data_ptr() not in mine]
    frozen = [t.detach().clone() for t in held]
    fields = ("fc_w", "fc_b", "proj_w", "proj_b", "fc_s", "proj_s")
    ptrs = [getattr(enc._moe_layers[i], f) for i in range(2) for f in fields] + \
           [getattr(enc._moe_layers_t[i], f) for i in range(2) for f in ("fc_t", "proj_t")]
    n_expert_bytes = sum(t.numel() * t.element_size() for t in held)
    assert n_expert_bytes >= 2 * E * (2 * 2 + 4) * 4 * 128 * 128   # pairs (2 x 2 bytes) and fp32 transposes of both matrices
    curve, aux = [], []
    for _ in range(gc.E2E_STEPS):
        st = tr.step(img, target)
        curve.append(st.loss.clone()), aux.append(st.aux_loss.clone())
    curve, aux = torch.cat(curve).cpu().numpy().astype(np.float64), torch.cat(aux).cpu().numpy().astype(np.float64)
    want = gc.e2e_f64(E, K)
    dev = np.abs(curve - want["losses"]) / np.abs(want["losses"])
    print("MoE E %d K %d: loss %.4f -> %.4f (float64 %.4f -> %.4f), largest deviation over %d steps %.2e, at step 1 %.2e; l_aux %.4f -> %.4f"
          % (E, K, curve[0], curve[-1], want["losses"][0], want["losses"][-1], gc.E2E_STEPS, dev.max(), dev[0], aux[0], aux[-1]))
    assert curve[-1] < curve[0] and want["losses"][-1] < want["losses"][0]
    assert dev[0] <= gc.BOUND and abs(aux[0] - want["aux"][0]) <= gc.BOUND * want["aux"][0]
    assert not torch.equal(masters[GATE], gate0)
    torch.cuda.synchronize()
    assert all(torch.equal(t, v) for t, v in zip(held, frozen))
    assert ptrs == [getattr(enc._moe_layers[i], f) for i in range(2) for f in fields] + \
                   [getattr(enc._moe_layers_t[i], f) for i in range(2) for f in ("fc_t", "proj_t")]
    assert not any(".experts." in k or (".gate." in k and k != GATE) for k in masters)
    bound = {id(p) for g in opt.param_groups for p in g["params"]}
    assert all(id(t) not in bound for t in held)


# ---- 6. the model and the loop ------------------------------------------------------------------------------------------------
def test_do_train_stage2_with_an_moe_model_on_both_paths(tmp_path, caplog):
    """the Uni-Prompt model with MODEL.MOE on (ViT-B/16 on 32 x 32 images, E 4, K 2, 2 MoE blocks) through do_train_stage2 for one
    epoch: the loop opts in by itself (and refuses, by name, a model whose experts were left trainable), on the fused path (TensorOptimizer) and on the autograd path (torch.optim.Adam); both log
    AuxLoss; the experts and the later gate keep their bits and block 0's gate moves; the checkpoint loads into a fresh model
    whose evaluation features carry the trained model's bits"""
    import logging
    from config import cfg_base
    from loss.make_loss import make_loss
    from model import make_model_uniprompt as mu
    from processor.processor_uniprompt_stage2 import do_train_stage2
    from solver.lr_scheduler import WarmupMultiStepLR
    from solver.make_optimizer_prompt import make_optimizer_2astage
    from test_gpu_stage2_train import _TrainLoader
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["INPUT.SIZE_TRAIN", [32, 32], "INPUT.SIZE_TEST", [32, 32], "MODEL.SIE_CAMERA", True,
                         "DATALOADER.SAMPLER", "softmax_triplet", "OUTPUT_DIR", str(tmp_path), "DATASETS.EXP_SETTING", "exp",
                         "MODEL.MOE.ENABLED", True, "MODEL.MOE.NUM_EXPERTS", 4, "MODEL.MOE.TOP_K", 2, "MODEL.MOE.MOE_LAYERS", 2])
    cfg.SOLVER.STAGE2.update(IMS_PER_BATCH=8, WARMUP_ITERS=0, BIAS_LR_FACTOR=2, WEIGHT_DECAY_BIAS=0.0)
    s2c = cfg.SOLVER.STAGE2
    m = mu.make_model(cfg, num_class=7, camera_num=3, view_num=1)
    with pytest.raises(NotImplementedError, match="enable_stage2_moe_training"):
        m.enable_stage2_training()
    loss_fn, center = make_loss(cfg, 7)
    gate = "image_encoder.transformer.resblocks.0.gate.weight"

    def run(opt, opt_center):
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.train"):
            do_train_stage2(cfg, m, center, _TrainLoader(), [], opt, opt_center,
                            WarmupMultiStepLR(opt, s2c.STEPS, s2c.GAMMA, s2c.WARMUP_FACTOR, s2c.WARMUP_ITERS, s2c.WARMUP_METHOD),
                            loss_fn, 0, 0, 1, 1, 1, 100)
        after = m.state_dict()
        assert "AuxLoss:" in caplog.text and "nan" not in caplog.text.lower()
        for k, v in before.items():
            if "expert" in k or (".gate." in k and k != gate):
                assert torch.equal(after[k], v), k
        assert not torch.equal(after[gate], before[gate])
        return caplog.text
    # the loop's own opt-in: the model is marked as the reference's 2a does and moved to the device by the caller (the optimizer
    # is built over device parameters), and has no training encoder yet.  With the experts left trainable the loop's opt-in is
    # the encoder's refusal, by name.
    m.to("cuda")
    for n, p in m.named_parameters():
        p.requires_grad = not ("text_encoder" in n or "expert" in n or "prompt_learner" in n)
    opt, opt_center = make_optimizer_2astage(cfg, m, center)
    assert isinstance(opt, ops.TensorOptimizer) and m._train_encoder is None
    held = {id(p) for g in opt.param_groups for p in g["params"]}
    named = dict(m.named_parameters())
    assert id(named[gate]) in held and not any(id(p) in held for n, p in named.items() if "expert" in n)   # the 2a selection
    for n, p in m.named_parameters():
        p.requires_grad = "prompt_learner" not in n and "text_encoder" not in n
    with pytest.raises(NotImplementedError, match="expert matrices' own gradients are not implemented"):
        run(opt, opt_center)
    assert m._train_encoder is None and not m._moe_training
    for n, p in m.named_parameters():
        p.requires_grad = not ("text_encoder" in n or "expert" in n or "prompt_learner" in n)
    assert "fused (mpreid.ops.Stage2Trainer)" in run(opt, opt_center)
    assert m._train_encoder is not None and m._moe_training
    assert not any(p.requires_grad for n, p in m.named_parameters() if "expert" in n) and dict(m.named_parameters())[gate].requires_grad
    trained = [p for n, p in m.named_parameters() if p.requires_grad]
    assert "autograd" in run(torch.optim.Adam(trained, lr=s2c.BASE_LR, foreach=False), torch.optim.SGD(center.parameters(), lr=0.5))
    m.train()
    out = m(x=_TrainLoader().img[:8].cuda(), label=torch.zeros(8, dtype=torch.long, device="cuda"),
            cam_label=torch.zeros(8, dtype=torch.long, device="cuda"))
    assert len(out) == 4 and tuple(out[3].shape) == (8 * 5, 4)
    m.eval()
    img = _TrainLoader().img[:8].cuda()
    cam = torch.zeros(8, dtype=torch.long, device="cuda")
    with torch.no_grad():
        feat = m(x=img, cam_label=cam).clone()
    fresh = mu.make_model(cfg, num_class=7, camera_num=3, view_num=1)
    fresh.load_param(str(tmp_path / "exp" / "ViT-B-16_1.pth"))
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh.to("cuda")(x=img, cam_label=cam), feat)
    dense_cfg = cfg.clone()
    dense_cfg.merge_from_list(["MODEL.MOE.ENABLED", False])
    with pytest.raises(ValueError, match="no MoE block"):
        mu.make_model(dense_cfg, num_class=7, camera_num=3, view_num=1).enable_stage2_moe_training()


def test_tower_entry_points_refuse_before_a_launch_and_the_next_call_is_intact(towers):
    """mpreid_vit_backward_moe and mpreid_vit_forward_train_moe through the C ABI: a short workspace, a misaligned pointer, a
    non-NULL MLP gradient member of an MoE block, a non-finite aux_coef and num_experts / top_k above the limits return their
    codes and write nothing; the next good call gives the bits of the call before"""
    c, enc, imgs, cv = towers("reduced")
    L = _lib.load()
    seeds = _seeds(c)
    good = enc.backward(imgs, cv, *seeds, want=[GATE, "tokens", "cv_emb"], aux_coef=gc.AUX_COEF)
    good = {k: v.clone() for k, v in good.items()}
    B, W = imgs.shape[0], 128
    desc = _lib.ImageIn(f32_dev=imgs.data_ptr())
    out = {k: torch.full_like(v, 7.0) for k, v in good.items()}
    need = L.mpreid_vit_backward_moe_workspace_bytes(C.byref(enc.c_cfg), C.byref(enc.c_moe), B)
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    lg = (_lib.VitLayerGrads * 3)()
    g = _lib.VitGrads()
    g.layers = C.cast(lg, C.POINTER(_lib.VitLayerGrads))
    g.cv_emb = out["cv_emb"].data_ptr()

    def call(ws_ptr=None, nbytes=need, tokens=None, coef=gc.AUX_COEF, moe=None):
        return L.mpreid_vit_backward_moe(C.byref(enc.c_cfg), C.byref(enc.c_w), C.byref(enc.c_wt), C.byref(moe or enc.c_moe),
                                         C.byref(enc.c_moe_t), C.byref(desc), B, cv.data_ptr(), seeds[0].data_ptr(),
                                         seeds[1].data_ptr(), seeds[2].data_ptr(), coef, C.byref(g), out[GATE].data_ptr(),
                                         tokens or out["tokens"].data_ptr(), None, ws_ptr or ws.data_ptr(), nbytes, _lib.stream_ptr())
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(ws_ptr=ws.data_ptr() + 16) == _lib.ERR_ARG
    assert call(tokens=out["tokens"].data_ptr() + 4) == _lib.ERR_ARG
    assert call(coef=float("nan")) == _lib.ERR_ARG and call(coef=float("inf")) == _lib.ERR_ARG
    lg[0].fc_w = out["tokens"].data_ptr()          # block 0 is an MoE block: it has no dense MLP to differentiate
    assert call() == _lib.ERR_ARG
    lg[0].fc_w = None
    for E, K in ((65, 2), (16, 9)):
        assert call(moe=_lib.VitMoe(E, K, 2, enc.c_moe.layers)) == _lib.ERR_UNSUPPORTED
    assert call(moe=_lib.VitMoe(4, 2, 0, enc.c_moe.layers)) == _lib.ERR_UNSUPPORTED
    f = [torch.full((B, n), 7.0, device="cuda") for n in (W, W, 64)]
    fneed = L.mpreid_vit_forward_train_moe_workspace_bytes(C.byref(enc.c_cfg), C.byref(enc.c_moe), B)

    def fwd(nbytes=fneed, f0=None, ws_off=0):
        return L.mpreid_vit_forward_train_moe(C.byref(enc.c_cfg), C.byref(enc.c_w), C.byref(enc.c_moe), C.byref(desc), B,
                                              cv.data_ptr(), f0 or f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), None, None,
                                              ws.data_ptr() + ws_off, nbytes, _lib.stream_ptr())
    assert fneed <= need and fwd(nbytes=fneed - 1) == _lib.ERR_WORKSPACE and fwd(ws_off=16) == _lib.ERR_ARG
    assert fwd(f0=f[0].data_ptr() + 2) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in list(out.values()) + f)      # nothing was launched
    assert call() == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], good[k]) for k in good)
    want_f = enc.forward_train(imgs, cv)
    assert all(torch.equal(a, b) for a, b in zip(f, want_f))
