"""The CLIP text tower on the GPU: the causal attention kernel against float64, its memory discipline and batch independence;
mpreid_text_forward against the reference's golden vectors and the float64 restatement; causality and row determinism of the
whole tower; limits and errors; the Uni-Prompt model's get_text branch.  Inputs and references: tests/text_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import text_cases as tc
from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def towers():
    """name -> (cfg, encoder, prompts on the device, eot, golden, float64) of the two stored configurations, built once"""
    out = {}
    for name in ("reduced", "full"):
        cfg, sd, prompts, eot, ref, f64 = tc.golden_case(name)
        out[name] = (cfg, ops.TextEncoder(cfg, sd, ws_tag="text_" + name), torch.from_numpy(prompts).cuda(), eot, ref, f64)
    return out


# ---- 1. the causal kernel against float64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", tc.ATT_TOKENS)
@pytest.mark.parametrize("width,heads", tc.ATT_SHAPES)
def test_causal_attention_against_float64(width, heads, tokens):
    """slab-relative error <= 2e-5, the split-mode bar.  Largest figure measured on an MI355X over the 28 cases: 6.5e-7
    ((512, 8), L = 80); the unmasked split kernel's committed figures are 7-8e-7"""
    qkv, want, scale = tc.attention_case(width, heads, tokens)
    out = ops.text_attention(qkv.cuda(), tc.ATT_BATCH, tokens, heads)
    assert bool(torch.isfinite(out).all())
    fig = tc.error_figure(tc.pairs_to_f64(out, tc.ATT_BATCH, tokens, heads), want, scale)
    print("causal attention (%d, %d) L = %d: %.3e" % (width, heads, tokens, fig))
    assert fig <= tc.BOUND_SPLIT


# ---- 2. poison -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [17, 77])
def test_causal_attention_reads_and_writes_only_its_rows(tokens):
    """qkv is followed by NaN guard rows in the same allocation, the output lies between sentinel guard rows: finite results
    (the partly filled last key tile multiplies zeros, not what lies behind row L - 1) and every guard byte untouched"""
    width, heads = 128, 2
    B, G = tc.ATT_BATCH, 32
    qkv, want, scale = tc.attention_case(width, heads, tokens)
    M = B * tokens
    buf = torch.full((M + G, 3 * width), float("nan"), dtype=torch.float32, device="cuda")
    buf[:M] = qkv.cuda()
    sentinel = 0x3A5C
    obuf = torch.full((G + M + G, 2 * width), sentinel, dtype=torch.int16, device="cuda")
    out = obuf[G:G + M].view(torch.float16)
    ops.text_attention(buf[:M], B, tokens, heads, out=out)
    torch.cuda.synchronize()
    assert bool((obuf[:G] == sentinel).all()) and bool((obuf[G + M:] == sentinel).all())
    assert bool(torch.isnan(buf[M:]).all())
    assert bool(torch.isfinite(out).all())
    assert tc.error_figure(tc.pairs_to_f64(out, B, tokens, heads), want, scale) <= tc.BOUND_SPLIT


# ---- 3. batch independence ----------------------------------------------------------------------------------------------
def test_causal_attention_rows_do_not_depend_on_the_batch():
    """one prompt repeated B times, B * heads > 4 x the CU count: every slab has the bits of a B = 1 call"""
    width, heads, tokens = 128, 2, 17
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = (4 * cus) // heads + 3
    one = tc.make_qkv(width, heads, 1, tokens).cuda()
    ref = ops.text_attention(one, 1, tokens, heads)
    got = ops.text_attention(one.repeat(B, 1).contiguous(), B, tokens, heads)
    assert B * heads > 4 * cus and bool((got.view(torch.int16).view(B, tokens, -1) == ref.view(torch.int16)[None]).all())


# ---- 4. the tower against the goldens and the float64 restatement ---------------------------------------------------------
@pytest.mark.parametrize("name", ["reduced", "full"])
def test_tower_against_the_golden_and_float64(towers, name):
    """relative L2 <= 2e-5 against the reference's encode_text and against the float64 restatement"""
    cfg, enc, prompts, eot, ref, f64 = towers[name]
    got = enc.forward(prompts, eot)
    assert got.shape == (len(eot), cfg["out_dim"]) and bool(torch.isfinite(got).all())
    e_ref, e_f64 = tc.rel_l2(got, ref), tc.rel_l2(got, f64)
    print("text tower %s: rel L2 %.3e against the golden, %.3e against float64" % (name, e_ref, e_f64))
    assert e_ref <= 2e-5 and e_f64 <= 2e-5


# ---- 5. causality end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reduced", "full"])
def test_rows_behind_the_eot_row_do_not_reach_the_features(towers, name):
    cfg, enc, prompts, eot, _, _ = towers[name]
    base = enc.forward(prompts, eot).clone()
    g = torch.Generator().manual_seed(77)
    fresh = (torch.randn(prompts.shape, generator=g) * 0.02).cuda()
    rows = torch.arange(cfg["tokens"], device="cuda")[None, :, None]
    e = torch.as_tensor(np.asarray(eot)).cuda().long()[:, None, None]
    behind = torch.where(rows > e, fresh, prompts)
    assert not torch.equal(behind, prompts)
    assert torch.equal(enc.forward(behind, eot), base)
    at = torch.where(rows == e, fresh, prompts)
    changed = enc.forward(at, eot)
    assert bool((changed != base).any(dim=1).all())


# ---- 6. row determinism of the tower ------------------------------------------------------------------------------------------
def test_a_prompt_has_the_same_bits_alone_in_a_batch_and_across_the_chunk_edge(towers):
    cfg, enc, prompts, eot, _, _ = towers["reduced"]
    assert enc.CHUNK == 512
    p, e = prompts[2:3], [int(eot[2])]
    alone = enc.forward(p, e).clone()
    assert torch.equal(enc.forward(prompts, eot)[2:3], alone)
    g = torch.Generator().manual_seed(5)
    big = (torch.randn((513, cfg["tokens"], cfg["width"]), generator=g) * 0.02).cuda()
    big_eot = np.full(513, 7, dtype=np.int64)
    for pos in (0, 300, 511, 512):        # first chunk (three places) and the one-prompt second chunk
        big[pos], big_eot[pos] = p[0], e[0]
    out = enc.forward(big, big_eot)
    for pos in (0, 300, 511, 512):
        assert torch.equal(out[pos:pos + 1], alone), pos
    assert bool(torch.isfinite(out).all())


# ---- 7. limits ----------------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_next_call_intact(towers):
    cfg, enc, prompts, eot, _, f64 = towers["reduced"]
    L = _lib.load()

    def good():
        assert tc.rel_l2(enc.forward(prompts, eot), f64) <= 2e-5

    # tokens = MPREID_TEXT_MAX_TOKENS works
    top = dict(tc.REDUCED, tokens=_lib.TEXT_MAX_TOKENS)
    sd = synth.text_state_dict(top, seed=41)
    p = tc.make_prompts(top, 2, 42)
    e = [_lib.TEXT_MAX_TOKENS - 1, 100]
    got = ops.TextEncoder(top, sd, ws_tag="text_top").forward(torch.from_numpy(p).cuda(), e)
    fig = tc.rel_l2(got, tc.tower_f64(top, sd, p, e))
    print("text tower at %d tokens: rel L2 %.3e against float64" % (_lib.TEXT_MAX_TOKENS, fig))
    assert fig <= 2e-5
    # one token more, a head dimension other than 64, another precision: MPREID_ERR_UNSUPPORTED
    over = dict(tc.REDUCED, tokens=_lib.TEXT_MAX_TOKENS + 1)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.TextEncoder(over, synth.text_state_dict(over, seed=41), ws_tag="text_over").forward(
            torch.zeros((1, over["tokens"], over["width"]), device="cuda"), [0])
    good()
    wide = dict(tc.REDUCED, heads=4)
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.TextEncoder(wide, synth.text_state_dict(wide, seed=41), ws_tag="text_wide").forward(prompts, eot)
    good()
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.TextEncoder(dict(tc.REDUCED, precision="fp16"), synth.text_state_dict(tc.REDUCED, seed=31))
    qkv = tc.make_qkv(128, 2, 1, 17).cuda()
    with pytest.raises(RuntimeError, match="code %d" % _lib.ERR_UNSUPPORTED):
        ops.text_attention(qkv.half(), 1, 17, 2)
    good()
    # a short workspace, a null pointer
    out = torch.empty((len(eot), cfg["out_dim"]), dtype=torch.float32, device="cuda")
    e_dev = torch.from_numpy(ops.check_eot(eot, len(eot), cfg["tokens"])).cuda()
    need = L.mpreid_text_workspace_bytes(ctypes.byref(enc.c_cfg), len(eot))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(prompts_ptr, ws_bytes):
        return L.mpreid_text_forward(ctypes.byref(enc.c_cfg), ctypes.byref(enc.c_w), prompts_ptr, e_dev.data_ptr(), len(eot),
                                     out.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    assert call(prompts.data_ptr(), need - 1) == _lib.ERR_WORKSPACE
    good()
    assert call(None, need) == _lib.ERR_ARG
    good()
    assert call(prompts.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert tc.rel_l2(out, f64) <= 2e-5
    with pytest.raises(ValueError):
        enc.forward(prompts, [0, 1, 2, 3, cfg["tokens"]])
    good()


# ---- 8. the model ---------------------------------------------------------------------------------------------------------------
def test_uniprompt_model_text_branch(tmp_path):
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    m = mu.make_model(cfg, num_class=7, camera_num=6, view_num=1)
    imgs = torch.from_numpy(synth.synthetic_images(2, 256, 128, seed=4)).cuda()
    img_feat = m(x=imgs).clone()
    label = torch.tensor([3, 0, 6, 6, 1]).cuda()
    view = torch.tensor([0, 6, 11, 12, 13]).cuda()

    def by_hand(stage, v):
        enc, pl = m.text_tower(), m.prompt_learner
        t = {k: getattr(pl, k).cpu() for k in mu.PROMPT_KEYS}
        prompts = tc.assemble_prompts(t, label.cpu(), stage, None if v is None else v.cpu())
        return enc.forward(prompts.cuda(), [cfg.MODEL.PROMPT_EOT_INDEX] * len(label)).clone()

    def check_branches():
        feats = []
        for stage, v in (("1a", None), ("1b", view), ("1b", None)):
            m.prompt_learner.set_training_stage(stage)
            got = m(label=label, get_text=True, view=v).clone()
            assert got.shape == (5, 512) and bool(torch.isfinite(got).all())
            assert torch.equal(got, by_hand(stage, v)), (stage, v is None)
            assert torch.equal(m(label=label, get_raw_text=True, view=v), got)
            feats.append(got)
        assert not torch.equal(feats[0], feats[1]) and not torch.equal(feats[1], feats[2])
        m.prompt_learner.set_training_stage("1a")
        return feats

    seeded = check_branches()
    assert torch.equal(m(x=imgs), img_feat)                         # the image branch is untouched by a get_text call
    # tokenized_prompts, when set, gives the read-out row
    tok = torch.zeros(1, 77, dtype=torch.long)
    tok[0, 30] = 49407
    m.prompt_learner.tokenized_prompts = tok
    moved = m(label=label, get_text=True)
    m.prompt_learner.tokenized_prompts = None
    assert not torch.equal(moved, seeded[0]) and torch.equal(m(label=label, get_text=True), seeded[0])
    # a complete synthetic checkpoint is picked up by load_param and changes the text features to the expected ones
    sd = synth.text_state_dict(mu.TEXT_CFG, seed=5)
    pt = tc.prompt_learner_tensors(7, 6)
    ck = {"module." + k: v.clone() for k, v in m.state_dict().items()}
    ck.update({"module.text_encoder." + k: torch.from_numpy(v) for k, v in sd.items()})
    ck.update({"module.prompt_learner." + k: v for k, v in pt.items()})
    ck["module.prompt_learner.visual_enhanced_net.linear1.weight"] = torch.zeros(32, 512)
    path = tmp_path / "uniprompt_text.pth"
    torch.save(ck, path)
    m.load_param(str(path))
    assert torch.equal(m(x=imgs), img_feat)
    loaded = check_branches()
    want = ops.TextEncoder(mu.TEXT_CFG, sd, ws_tag="text_want").forward(tc.assemble_prompts(pt, label.cpu(), "1a").cuda(), [19] * 5)
    assert torch.equal(loaded[0], want) and not torch.equal(loaded[0], seeded[0])
    assert torch.equal(m(x=imgs), img_feat)


def test_encode_tokens_equals_forward_on_the_gathered_rows(towers):
    cfg = tc.REDUCED
    sd = synth.text_state_dict(cfg, seed=31, vocab=40)
    enc = ops.TextEncoder(cfg, sd, ws_tag="text_vocab")
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 39, size=(4, cfg["tokens"]))
    eot = [1, 9, 20, 4]
    for b, e in enumerate(eot):
        ids[b, e] = 39                                   # the largest id of its row, once
    got = enc.encode_tokens(torch.from_numpy(ids))
    rows = torch.from_numpy(sd["token_embedding.weight"][ids]).cuda()
    assert torch.equal(got, enc.forward(rows, eot))
    assert torch.equal(got, towers["reduced"][1].forward(rows, eot))   # the same weights (seed 31) without the table
    with pytest.raises(ValueError):
        towers["reduced"][1].encode_tokens(torch.from_numpy(ids))   # no embedding table in that state dict
