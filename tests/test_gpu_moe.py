"""The MoE image encoder on the GPU: the router on exact integers and from the residual stream, the routed MLP alone against
float64 with caller-made routing, the combine's order and weights on exact data, the tower against the reference's golden
vectors and the float64 restatement, batch independence, E = 1 against the dense tower, views and uint8 input, wrong variants
of the restatement, limits and errors, the drop-in models.  Cases and references: tests/moe_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import moe_cases as mc
from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def towers():
    """name -> (golden case, encoder, images on the device, device features) of the reduced cases, built and run once"""
    out = {}
    for name in ("reduced", "reduced_all", "reduced_wide"):
        g = mc.golden_case(name)
        enc = ops.VitEncoder(g["cfg"], g["sd"], g["hw"], ws_tag="moe_" + name)
        imgs = torch.from_numpy(g["imgs"]).cuda()
        out[name] = (g, enc, imgs, enc(imgs).clone())
    return out


# ---- 1. the router on exact integers -------------------------------------------------------------------------------------
ROUTER_EK = [(E, K) for E in (1, 2, 3, 8, 64) for K in sorted({1, 2, E}) if K <= min(E, 8)]


@pytest.mark.parametrize("E,K", ROUTER_EK)
def test_router_on_exact_integers(E, K):
    """h and the gate hold small integers (8 non-zero entries of +-1 per row of h, gate entries in -2 .. 2), so every logit is
    an integer below 2^5 under any summation order; the last expert repeats expert 0's gate row (an exact tie on every row) and
    the integer range is small enough that other ties occur.  sel == a stable descending sort of the integer logits, w within
    1e-6 of the float64 softmax / renormalisation, K == 1: w == 1.0f, logits == the integers."""
    width = 128
    rng = np.random.default_rng(100 * E + K)
    gate = rng.integers(-2, 3, size=(E, width)).astype(np.float32)
    if E >= 2:
        gate[E - 1] = gate[0]
    for rows in (1, 63, 64, 65, 257):
        h = np.zeros((rows, width), np.float32)
        for r in range(rows):
            h[r, rng.choice(width, 8, replace=False)] = rng.choice([-1.0, 1.0], 8)
        want_logits = torch.from_numpy(h).double() @ torch.from_numpy(gate).double().T
        want_sel = mc.topk_lower_first(want_logits, K)   # on the integers themselves
        sel, w, logits = ops.moe_route(torch.from_numpy(h), torch.from_numpy(gate), K, want_logits=True)
        assert torch.equal(logits.cpu().double(), want_logits), (E, K, rows)
        assert torch.equal(sel.cpu().long(), want_sel), (E, K, rows)
        p = torch.softmax(want_logits, -1)
        ps = torch.gather(p, -1, want_sel)
        err = float((w.cpu().double() - ps / ps.sum(-1, keepdim=True)).abs().max())
        assert err <= 1e-6, (E, K, rows, err)
        if K == 1:
            assert bool((w.view(torch.int32) == 0x3F800000).all())
        if E >= 2 and K >= 2:   # the planted tie: wherever experts 0 and E - 1 are both selected, 0 comes first
            s = sel.cpu()
            both = (s == 0).any(-1) & (s == E - 1).any(-1)
            pos0 = (s == 0).float().argmax(-1)
            pos1 = (s == E - 1).float().argmax(-1)
            assert bool((pos0[both] < pos1[both]).all())


# ---- 2. the router from the residual stream ------------------------------------------------------------------------------
def test_router_from_the_residual_stream():
    """block 0's residual stream of `reduced` (from the float64 restatement, rounded to fp32) with ln_2's gamma / beta: the
    selection equals the golden's on every token, the logits agree with the reference's within 10 x the margin's denominator"""
    g = mc.golden_case("reduced")
    cfg, sd, f64 = g["cfg"], g["sd"], g["f64"]
    p = "transformer.resblocks.0."
    sel, w, logits = ops.moe_route(f64["x1"].float(), torch.from_numpy(sd[p + "gate.weight"]), cfg["top_k"],
                                   ln=(sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]), want_logits=True)
    ref_sel = mc.topk_lower_first(torch.from_numpy(g["ref_logits"]).double(), cfg["top_k"])
    assert torch.equal(sel.cpu().long().sort(-1).values, ref_sel.sort(-1).values)
    assert torch.equal(sel.cpu().long(), f64["sel"])
    _, err = mc.margin_figures(f64["logits"], g["ref_logits"], cfg["top_k"])
    dev = float((logits.cpu().double() - torch.from_numpy(g["ref_logits"]).double()).abs().max())
    print("router logits vs the reference: %.3e (reference's own fp32 error %.3e)" % (dev, err))
    assert dev <= 10.0 * err
    assert float((w.cpu().double() - f64["w"]).abs().max()) <= 1e-5


# ---- 3. the routed MLP alone ---------------------------------------------------------------------------------------------
def _sel_from_counts(counts, rng):
    """K = 1 routing with exactly counts[e] rows on expert e, shuffled"""
    sel = np.concatenate([np.full(c, e, np.int32) for e, c in enumerate(counts)])
    return rng.permutation(sel)[:, None]


def _mlp_case(kind):
    rng = np.random.default_rng(7)
    E = 4
    if kind.startswith("counts"):
        counts = {"counts_0_1_127_128": (0, 1, 127, 128), "counts_129_0_0_255": (129, 0, 0, 255),
                  "counts_one_expert_three_tiles": (0, 0, 300, 0)}[kind]
        sel = _sel_from_counts(counts, rng)
    elif kind == "k2_hole":      # two experts per row out of {0, 2, 3}: expert 1 stays empty between used ones
        rows = 193
        sel = np.stack([rng.permutation(np.array([0, 2, 3], np.int32))[:2] for _ in range(rows)])
    else:                        # k == E: every row on every expert, in a shuffled order
        rows = 130
        sel = np.stack([rng.permutation(E).astype(np.int32) for _ in range(rows)])
    w = rng.uniform(0.1, 1.0, size=sel.shape).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    return E, np.ascontiguousarray(sel), np.ascontiguousarray(w.astype(np.float32))


@pytest.mark.parametrize("kind", ["counts_0_1_127_128", "counts_129_0_0_255", "counts_one_expert_three_tiles", "k2_hole", "k_all"])
def test_routed_mlp_against_float64(kind):
    """mpreid_moe_mlp_split with routing chosen here, width 128, E = 4: segment sizes on both sides of the 128-row tile, an
    empty expert between used ones, K = 1, 2 and E, rows no multiple of the tile.  x[rows] - x0 against the float64 sum:
    relative L2 <= 2e-5; NaN weights of the empty experts reach nothing; guard rows of x and guard bytes behind the workspace
    keep their contents."""
    width = 128
    E, sel, w = _mlp_case(kind)
    rows, K = sel.shape
    rng = np.random.default_rng(11)
    h = rng.standard_normal((rows, width)).astype(np.float32)
    fc_w = (rng.standard_normal((E, 4 * width, width)) * width ** -0.5).astype(np.float32)
    fc_b = (rng.standard_normal((E, 4 * width)) * 0.1).astype(np.float32)
    proj_w = (rng.standard_normal((E, width, 4 * width)) * (4 * width) ** -0.5).astype(np.float32)
    proj_b = (rng.standard_normal((E, width)) * 0.1).astype(np.float32)
    used = np.zeros(E, bool)
    used[np.unique(sel)] = True
    for e in np.nonzero(~used)[0]:
        fc_w[e] = fc_b[e] = proj_w[e] = proj_b[e] = np.nan
    x0 = rng.standard_normal((rows + 5, width)).astype(np.float32)
    want = mc.experts_f64(torch.from_numpy(h).double(), torch.from_numpy(sel).long(), torch.from_numpy(w).double(),
                          *(torch.from_numpy(a).double() for a in (fc_w, fc_b, proj_w, proj_b)))
    layer, keep = ops.pack_moe_layer(fc_w, fc_b, proj_w, proj_b)
    need = _lib.load().mpreid_moe_workspace_bytes(rows, width, E, K)
    assert need > 0
    wsbuf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(x0).cuda()
    ops.moe_mlp(ops.split_pairs_f32(torch.from_numpy(h)), torch.from_numpy(sel).cuda(), torch.from_numpy(w).cuda(), layer, x, E,
                ws=wsbuf[:need])
    torch.cuda.synchronize()
    got = x.cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[rows:], torch.from_numpy(x0[rows:])) and bool((wsbuf[need:] == 0xA5).all())
    rel = mc.rel_l2(got[:rows].double() - torch.from_numpy(x0[:rows]).double(), want)
    print("routed MLP %s: %.3e" % (kind, rel))
    assert rel <= mc.BOUND_SPLIT


# ---- 4. combine order and weights on exact data ---------------------------------------------------------------------------
def test_combine_weights_and_bias_placement_exact():
    """c_fc: zero weights, bias 32 on eight hidden units and 0 elsewhere, so QuickGELU gives exactly 32 / 0; c_proj: integer
    weights in -4 .. 4 and integer biases, so every expert output is an integer below 2^11; w in {0.25, 0.75}: every product and
    sum is exact in fp32 and x must equal x0 + sum w * (y + b) to the bit"""
    width, E, K, rows = 128, 4, 2, 200
    rng = np.random.default_rng(5)
    fc_w = np.zeros((E, 4 * width, width), np.float32)
    fc_b = np.zeros((E, 4 * width), np.float32)
    units = rng.choice(4 * width, 8, replace=False)
    fc_b[:, units] = 32.0
    proj_w = np.zeros((E, width, 4 * width), np.float32)
    proj_w[:, :, units] = rng.integers(-4, 5, size=(E, width, 8)).astype(np.float32)
    proj_w[:, 0, units[0]] = 4.0   # the largest entry is 4 in every expert: one scale rule, exact powers of two
    proj_b = rng.integers(-8, 9, size=(E, width)).astype(np.float32)
    sel = np.stack([rng.permutation(E).astype(np.int32)[:K] for _ in range(rows)])
    w = np.where(rng.random((rows, 1)) < 0.5, np.array([[0.25, 0.75]], np.float32), np.array([[0.75, 0.25]], np.float32)).astype(np.float32)
    h = rng.standard_normal((rows, width)).astype(np.float32)
    x0 = rng.integers(-16, 17, size=(rows, width)).astype(np.float32)
    want = torch.from_numpy(x0).double() + mc.experts_f64(
        torch.from_numpy(h).double(), torch.from_numpy(sel).long(), torch.from_numpy(w).double(),
        *(torch.from_numpy(a).double() for a in (fc_w, fc_b, proj_w, proj_b)))
    layer, keep = ops.pack_moe_layer(fc_w, fc_b, proj_w, proj_b)
    x = torch.from_numpy(x0).cuda()
    ops.moe_mlp(ops.split_pairs_f32(torch.from_numpy(h)), torch.from_numpy(sel).cuda(), torch.from_numpy(np.ascontiguousarray(w)).cuda(),
                layer, x, E)
    assert torch.equal(x.cpu().double(), want)


# ---- 5. the tower against the goldens and float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reduced", "reduced_all", "reduced_wide"])
def test_tower_against_the_golden_and_float64(towers, name):
    g, enc, imgs, got = towers[name]
    a, b = mc.rel_l2(got, g["ref"]), mc.rel_l2(got, g["f64"]["feat"])
    print("MoE tower %s: %.3e vs the reference, %.3e vs float64" % (name, a, b))
    assert bool(torch.isfinite(got).all()) and a <= mc.BOUND_SPLIT and b <= mc.BOUND_SPLIT


def test_full_tower_with_and_without_cls_only_last():
    """ViT-B/16 at 256 x 128, E = 4, K = 2, two MoE blocks: both settings within 2e-5 of the reference and of float64, and equal
    to each other bit for bit (the last block is a dense block: the dense tower's own guarantee)"""
    g = mc.golden_case("full")
    imgs = torch.from_numpy(g["imgs"]).cuda()
    outs = []
    for cls_last in (True, False):
        enc = ops.VitEncoder(g["cfg"], g["sd"], g["hw"], cls_only_last=cls_last, ws_tag="moe_full_%d" % cls_last)
        got = enc(imgs).clone()
        a, b = mc.rel_l2(got, g["ref"]), mc.rel_l2(got, g["f64"]["feat"])
        print("MoE tower full (cls_only_last %s): %.3e vs the reference, %.3e vs float64" % (cls_last, a, b))
        assert a <= mc.BOUND_SPLIT and b <= mc.BOUND_SPLIT
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    ops.release_workspaces("moe_full_1_moe"), ops.release_workspaces("moe_full_0_moe")


# ---- 6. batch independence -----------------------------------------------------------------------------------------------
def test_an_image_has_the_same_bits_in_any_batch(towers):
    """alone, in the batch of 3, twice, and inside a batch of 130 images (1170 token rows: more than one 1024-row dispatch
    workgroup and many GEMM row tiles) at positions on both sides of those edges"""
    g, enc, imgs, got = towers["reduced"]
    assert torch.equal(enc(imgs), got)   # run to run
    for i in range(3):
        assert torch.equal(enc(imgs[i:i + 1])[0], got[i])
    big = torch.from_numpy(synth.synthetic_images(130, *g["hw"], seed=77)).cuda()
    for pos, i in ((0, 0), (113, 1), (114, 2), (129, 0), (56, 1)):   # row 1024 lies inside image 113 (9 tokens per image)
        big[pos] = imgs[i]
    out = enc(big)
    for pos, i in ((0, 0), (113, 1), (114, 2), (129, 0), (56, 1)):
        assert torch.equal(out[pos], got[i]), pos


def test_an_image_has_the_same_bits_across_the_encode_group_edge(towers):
    """the grouped pipeline of do_inference (mpreid.pipeline.EncodePipeline: loader batches cut at group boundaries, groups
    encoded by separate calls of different sizes on two alternating streams, each with its own workspace and its own dispatch
    tables): 14 images in loader batches of 4 with group = 5 give calls of 5, 5 and 4 images; the golden images sit on both
    sides of both edges and every feature has the bits of the single-call feature"""
    from mpreid.pipeline import EncodePipeline
    g, enc, imgs, got = towers["reduced"]
    allimgs = torch.from_numpy(synth.synthetic_images(14, *g["hw"], seed=78))
    where = {4: 0, 5: 1, 9: 2, 10: 0, 13: 1}   # last of call 1, first of call 2, last of call 2, first of call 3, last image
    for pos, i in where.items():
        allimgs[pos] = torch.from_numpy(g["imgs"][i])
    single = enc(allimgs.cuda()).clone()
    for pos, i in where.items():
        assert torch.equal(single[pos], got[i]), pos
    batches = [(allimgs[lo:lo + 4], tuple(range(lo, min(lo + 4, 14))), (0,) * min(4, 14 - lo), torch.zeros(min(4, 14 - lo), dtype=torch.int64),
                torch.zeros(min(4, 14 - lo), dtype=torch.int64), ("p",) * min(4, 14 - lo)) for lo in range(0, 14, 4)]
    pipe = EncodePipeline(lambda x, cam_label=None, view_label=None: enc(x), group=5, streams=2)
    feats = torch.cat([f for f, _ in pipe.run(batches)], dim=0)
    torch.cuda.synchronize()
    assert pipe.stats["groups"] == 3 and pipe.stats["images"] == 14
    assert torch.equal(feats, single)


# ---- 7. E = 1, K = 1 equals the dense tower -------------------------------------------------------------------------------
def test_single_expert_equals_the_dense_tower():
    """every block an MoE block whose single expert holds the dense MLP: the new kernels against mpreid_vit_forward"""
    cfg = dict(mc.CASES["reduced"][0], num_experts=0, top_k=0, moe_layers=0)
    sd = synth.vit_state_dict(cfg, seed=17, std=0.05, ln_jitter=0.1)
    imgs = torch.from_numpy(synth.synthetic_images(5, 64, 32, seed=9)).cuda()
    dense = ops.VitEncoder(cfg, sd, (64, 32), ws_tag="moe_dense")
    assert dense.c_moe is None
    # the dense request is today's path: a cfg without the MoE keys gives the same bits
    plain = ops.VitEncoder({k: v for k, v in cfg.items() if k not in ("num_experts", "top_k", "moe_layers")}, sd, (64, 32))
    assert torch.equal(plain(imgs), dense(imgs))
    moe = ops.VitEncoder(dict(cfg, num_experts=1, top_k=1, moe_layers=-1), mc.dense_as_single_expert(sd, cfg["layers"]), (64, 32),
                         ws_tag="moe_e1")
    assert moe.c_moe is not None and moe.c_moe.moe_layers == cfg["layers"]
    rel = mc.rel_l2(moe(imgs), dense(imgs))
    print("E = 1 MoE tower vs the dense tower: %.3e" % rel)
    assert rel <= mc.BOUND_SPLIT


# ---- 8. views and uint8 input ---------------------------------------------------------------------------------------------
def _view_of(x, v):
    return (x if v == 0 else torch.flip(x, [3]) if v == 1 else x.mean(dim=1, keepdim=True).repeat(1, 3, 1, 1) if v == 2
            else x[:, 0:1].repeat(1, 3, 1, 1))


@pytest.mark.parametrize("view", [0, 1, 2, 3])
def test_views_against_float64_of_the_materialised_view(towers, view):
    g, enc, imgs, _ = towers["reduced"]
    want = mc.tower_f64(g["cfg"], g["sd"], _view_of(torch.from_numpy(g["imgs"]), view).contiguous())["feat"]
    rel = mc.rel_l2(enc.forward_view(imgs, view), want)
    print("MoE tower view %d: %.3e" % (view, rel))
    assert rel <= mc.BOUND_SPLIT


def test_uint8_input_against_float64(towers):
    g, enc, _, _ = towers["reduced"]
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, size=(3,) + g["hw"] + (3,), dtype=np.uint8)
    x = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5
    rel = mc.rel_l2(enc.forward_u8(torch.from_numpy(u8)), mc.tower_f64(g["cfg"], g["sd"], x)["feat"])
    print("MoE tower uint8 input: %.3e" % rel)
    assert rel <= mc.BOUND_SPLIT


# ---- 9. discrimination ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", mc.WRONG_VARIANTS)
def test_wrong_variants_are_far_from_the_device_output(towers, variant):
    """each wrong variant of the float64 restatement is farther than MUTANT_FLOOR from the device output on at least one case"""
    figs = {}
    for name, (g, enc, imgs, got) in towers.items():
        figs[name] = mc.rel_l2(got, mc.tower_f64(g["cfg"], g["sd"], g["imgs"], variant=variant)["feat"])
    print("variant %s: %s" % (variant, {k: "%.2e" % v for k, v in figs.items()}))
    assert max(figs.values()) > mc.MUTANT_FLOOR


# ---- 10. limits and errors ------------------------------------------------------------------------------------------------
def test_refused_calls_return_their_codes_and_leave_the_next_call_intact(towers):
    L = _lib.load()
    g, enc, imgs, got = towers["reduced"]
    width, rows = 128, 16
    x = torch.randn(rows + 1, width, device="cuda")
    gate = torch.randn(80, width, device="cuda")
    sel = torch.full((rows, 16), -7, dtype=torch.int32, device="cuda")
    w = torch.full((rows, 16), -7.0, device="cuda")
    sp = _lib.stream_ptr()

    def route(xp, E, K):
        return L.mpreid_moe_route(xp, rows, width, None, None, gate.data_ptr(), E, K, sel.data_ptr(), w.data_ptr(), None, sp)
    assert route(x.data_ptr(), 4, 5) == _lib.ERR_UNSUPPORTED          # K > E
    assert route(x.data_ptr(), 65, 2) == _lib.ERR_UNSUPPORTED         # E > 64
    assert route(x.data_ptr(), 16, 9) == _lib.ERR_UNSUPPORTED         # K > 8
    assert route(x.data_ptr() + 4, 4, 2) == _lib.ERR_ARG              # a misaligned pointer
    assert L.mpreid_moe_workspace_bytes(rows, width, 65, 2) == 0 and L.mpreid_moe_workspace_bytes(rows, width, 4, 5) == 0
    # more token rows than MPREID_MOE_MAX_ROWS (refused on the sizes alone: nothing is read)
    assert L.mpreid_moe_workspace_bytes(2 ** 20, width, 4, 2) > 0 and L.mpreid_moe_workspace_bytes(2 ** 20 + 1, width, 4, 2) == 0
    assert L.mpreid_moe_route(x.data_ptr(), 2 ** 20 + 1, width, None, None, gate.data_ptr(), 4, 2, sel.data_ptr(), w.data_ptr(), None,
                              sp) == _lib.ERR_UNSUPPORTED
    # the routed MLP: a short workspace, a misaligned workspace
    layer, keep = ops.pack_moe_layer(*(np.zeros(s, np.float32) for s in ((4, 512, 128), (4, 512), (4, 128, 512), (4, 128))))
    a = torch.zeros((rows, 2 * width), dtype=torch.float16, device="cuda")
    need = L.mpreid_moe_workspace_bytes(rows, width, 4, 2)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    x_before = x.clone()

    def mlp(wsp, nbytes, E=4, K=2):
        return L.mpreid_moe_mlp_split(a.data_ptr(), rows, width, sel.data_ptr(), w.data_ptr(), E, K, C.byref(layer), x.data_ptr(),
                                      wsp, nbytes, sp)
    assert mlp(ws.data_ptr(), need - 1) == _lib.ERR_WORKSPACE
    assert mlp(ws.data_ptr() + 16, need) == _lib.ERR_ARG
    assert mlp(ws.data_ptr(), need, E=4, K=5) == _lib.ERR_UNSUPPORTED
    # the forward: fp16 precision, a short workspace
    cfg16 = _lib.VitCfg.from_buffer_copy(enc.c_cfg)
    cfg16.precision = _lib.VIT_F16
    desc = _lib.ImageIn(mean=(C.c_float * 3)(0.5, 0.5, 0.5), std=(C.c_float * 3)(0.5, 0.5, 0.5), view=0)
    desc.f32_dev = imgs.data_ptr()
    out = torch.full_like(got, -7.0)
    need_f = L.mpreid_vit_workspace_bytes_moe(C.byref(enc.c_cfg), C.byref(enc.c_moe), 3)
    wsf = torch.zeros(need_f, dtype=torch.uint8, device="cuda")

    def fwd(cfg, nbytes):
        return L.mpreid_vit_forward_moe(C.byref(cfg), C.byref(enc.c_w), C.byref(enc.c_moe), C.byref(desc), 3, None, out.data_ptr(),
                                        wsf.data_ptr(), nbytes, sp)
    assert L.mpreid_vit_workspace_bytes_moe(C.byref(cfg16), C.byref(enc.c_moe), 3) == 0
    assert fwd(cfg16, need_f) == _lib.ERR_UNSUPPORTED
    assert fwd(enc.c_cfg, need_f - 1) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it held
    assert bool((sel == -7).all()) and bool((w == -7.0).all()) and torch.equal(x, x_before) and bool((out == -7.0).all())
    # and the next good calls are intact
    assert fwd(enc.c_cfg, need_f) == 0
    assert torch.equal(out, got)
    assert mc.rel_l2(enc(imgs), g["f64"]["feat"]) <= mc.BOUND_SPLIT


# ---- 11. drop-in ----------------------------------------------------------------------------------------------------------
def _moe_cfg(extra=()):
    from config import cfg_base
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.MOE.ENABLED", True, "MODEL.MOE.NUM_EXPERTS", 2, "MODEL.MOE.TOP_K", 2, "MODEL.MOE.MOE_LAYERS", 1,
                         "DATASETS.SYNTH_QUERY", 16, "DATASETS.SYNTH_GALLERY", 48, "DATASETS.SYNTH_IDS", 8,
                         "TEST.IMS_PER_BATCH", 16] + list(extra))
    cfg.freeze()
    return cfg


@pytest.mark.parametrize("which", ["base", "uniprompt"])
def test_dropin_model_round_trip_and_inference(which, tmp_path, monkeypatch):
    """make_model with MODEL.MOE on: the state dict has the reference's expert / gate keys, a checkpoint with other weights loads
    through load_param, model(x) is within 2e-5 of the float64 restatement of that checkpoint, and the processor's own
    do_inference runs on a 64-image synthetic loader: processor.processor's with an encode group of 24 (calls of 24, 24 and 16
    images cut inside the loader's batches of 16: the evaluator's features have the bits of one 64-image call), the Uni-Prompt
    processor's do_inference and its TTA-view caller on the Uni-Prompt model"""
    from datasets.make_dataloader import make_dataloader
    if which == "uniprompt":
        from processor.processor_uniprompt_stage2 import do_inference, do_inference_ttpt_option_a
    else:
        from processor.processor import do_inference
        monkeypatch.setenv("MPREID_PIPELINE", "group=24")
    mm = __import__("model.make_model_uniprompt" if which == "uniprompt" else "model.make_model", fromlist=["make_model"])
    cfg = _moe_cfg(["TEST.TTA_ENABLED", True] if which == "uniprompt" else [])
    _, _, val_loader, num_query, num_classes, cam_num, view_num = make_dataloader(cfg)
    model = mm.make_model(cfg, num_class=num_classes, camera_num=cam_num, view_num=view_num)
    keys = set(model.state_dict().keys())
    b = "image_encoder.transformer.resblocks."
    assert b + "0.experts.1.c_proj.bias" in keys and b + "0.gate.weight" in keys and b + "0.mlp.c_fc.weight" not in keys
    assert b + "1.mlp.c_fc.weight" in keys and b + "1.gate.weight" not in keys
    vcfg = dict(synth.VIT_B16, num_experts=2, top_k=2, moe_layers=1)
    sd = synth.vit_moe_state_dict(vcfg, seed=91, std=0.02, ln_jitter=0.05, gate_std=0.3)
    path = str(tmp_path / "moe_ckpt.pth")
    torch.save({"image_encoder." + k: torch.from_numpy(v) for k, v in sd.items()}, path)
    model.load_param(path)
    imgs = synth.synthetic_images(2, 256, 128, seed=4)
    got = model(torch.from_numpy(imgs).cuda()) if which == "base" else model(x=torch.from_numpy(imgs).cuda())
    rel = mc.rel_l2(got, mc.tower_f64(vcfg, sd, imgs)["feat"])
    print("drop-in MoE model (%s): %.3e" % (which, rel))
    assert rel <= mc.BOUND_SPLIT
    r1, r5 = do_inference(cfg, model, val_loader, num_query)
    assert np.isfinite(float(r1)) and np.isfinite(float(r5)) and 0.0 <= float(r1) <= float(r5) <= 1.0
    if which == "base":
        assert do_inference.last_pipeline_stats["groups"] == 3 and do_inference.last_pipeline_stats["images"] == 64
        feats = torch.cat(do_inference.last_evaluator.feats, dim=0)
        one_call = model(torch.cat([b[0] for b in val_loader], dim=0).cuda())
        assert feats.shape == one_call.shape and torch.equal(feats.to(one_call.device), one_call)
    else:
        a1, a5 = do_inference_ttpt_option_a(cfg, model, val_loader, num_query)   # the four views of every query batch, averaged
        assert np.isfinite(float(a1)) and np.isfinite(float(a5)) and 0.0 <= float(a1) <= float(a5) <= 1.0
