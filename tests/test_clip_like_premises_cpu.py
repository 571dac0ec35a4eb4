"""Host-side premises of the stress cases of the gradient tests (clip_like_cases.py; the saturated attention slabs of
vit_grad_cases.py / text_grad_cases.py): the stress is real.  Everything here is checked on the float64 / float32 restatements;
no GPU.  Run with -s to see the figures."""
import pytest
import torch

import clip_like_cases as cl
import text_cases as tc
import text_grad_cases as tg
import vit_grad_cases as vg

BOUND = vg.BOUND


# ---- alignment: the fast staging of the exact fp32 GEMM (K % 16 == 0) ---------------------------------------------------------
def test_alignment_of_the_stress_cases():
    """align4(B L), align4(B) and B P are multiples of 16 on the aligned cases (every weight-gradient GEMM stages its operands
    with unconditional 16-byte loads), clip129 keeps the other staging.
    Every case of vg.TOWER_CASES whose gradients the GPU tests take has Mp4 % 16 != 0: t129 388, stride12 36, one_layer 20,
    t257 516, full 28, e2e 216 (two_layers, 16, is the golden pin's and the forward's case only)."""
    for name in ("aligned9", "aligned129", "clip9", "clip_full9"):
        mp4, bp4, bp = cl.alignment(name)
        print("%s: Mp4 %d Bp4 %d B P %d" % (name, mp4, bp4, bp))
        assert mp4 % 16 == 0 and bp4 % 16 == 0 and bp % 16 == 0, name
    assert cl.alignment("clip129")[0] % 16 != 0
    # the record: no tower-gradient case of vit_grad_cases that the GPU gradient tests run is aligned
    for name in ("t129", "stride12", "one_layer", "t257", "full", "e2e"):
        cfg, _, _, imgs, _, _ = vg.tower_case(name)
        rows = imgs.shape[0] * (cfg["h_res"] * cfg["w_res"] + 1)
        assert (rows + 3) // 4 * 4 % 16 != 0, name
    # the MoE tower: `aligned` is the one aligned case
    import moe_grad_cases as gc
    for name, (cfg, _, n, _, _) in gc.TOWER_CASES.items():
        rows, patches = n * (cfg["h_res"] * cfg["w_res"] + 1), n * cfg["h_res"] * cfg["w_res"]
        is_aligned = (rows + 3) // 4 * 4 % 16 == 0 and (n + 3) // 4 * 4 % 16 == 0 and patches % 16 == 0
        assert is_aligned == (name == "aligned"), name


# ---- the clip-like towers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cl.CLIP_LIKE)
def test_clip_like_towers_are_stressed(name):
    """on the float64 graph: ln_pre writes a massive channel (>= 500), FC1 pre-activations beyond +-52.13 (expf(1.702 |u|)
    overflows fp32), block 0's attention is peaked (median largest probability >= 0.15, largest >= 0.75).
    Measured: ln_pre's largest entry 812 / 816 / 1968, FC1 pre-activations -60.3 .. 60.3, median / largest probability
    clip9 0.59 / 1.00, clip129 0.56 / 1.00, clip_full9 0.40 / 0.99 (1 / L is 0.111, 0.008, 0.111)"""
    taps = cl.stress_taps(name)
    big = float(taps["ln_pre"].abs().max())
    pre = torch.cat([t.reshape(-1) for t in taps["fc1_pre"]])
    top = taps["probs"][0].amax(dim=-1).reshape(-1)
    med, largest = float(top.median()), float(top.max())
    L = taps["probs"][0].shape[-1]
    print("%s: ln_pre max %.0f, FC1 pre-activation %.1f .. %.1f, block 0 largest probability per row: median %.3f largest %.3f (1 / L = %.3f)"
          % (name, big, float(pre.min()), float(pre.max()), med, largest, 1.0 / L))
    assert big >= 500.0
    assert float(pre.max()) > cl.EXPF_OVERFLOW and float(pre.min()) < -cl.EXPF_OVERFLOW
    assert med >= 0.15 and largest >= 0.75
    cfg, _, sd, _, _, _ = cl.stress_case(name)
    assert all(u.size == 3 for u in cl.planted_units(sd, cfg)) and all(u.size == 3 for u in cl.planted_units(sd, cfg, 60.0))


@pytest.mark.parametrize("name", cl.CLIP_LIKE)
def test_fp32_autograd_misses_the_bound_on_clip_like_towers(name):
    """plain fp32 autograd of the restatement against float64, per tensor: at least one tensor above 2e-5 on each clip-like case
    (the device is granted 8 x these figures per tensor, never less than the bound).  Measured, worst tensor: clip9 3.4e-5,
    clip129 2.8e-5, clip_full9 1.6e-4, conv1.weight each time; 3, 1 and 10 tensors above the bound (the figures move with the
    host's BLAS and thread count: another host gave 9.3e-5, 2.8e-5, 1.3e-4)"""
    figs = cl.host_figures(name)
    for k, f in figs.items():
        print("%s fp32 autograd %s: %.3e" % (name, k, f))
    worst = max(figs, key=figs.get)
    above = sum(f > BOUND for f in figs.values())
    print("%s: worst %.3e (%s), %d of %d tensors above the bound" % (name, figs[worst], worst, above, len(figs)))
    assert figs[worst] > BOUND


@pytest.mark.parametrize("name", cl.ALIGNED)
def test_fp32_autograd_meets_the_bound_on_the_aligned_towers(name):
    """the aligned towers are benign: fp32 autograd itself is within the bound, so the bound is a fair one for the device"""
    figs = cl.host_figures(name)
    worst = max(figs, key=figs.get)
    print("%s: fp32 autograd worst %.3e (%s)" % (name, figs[worst], worst))
    assert figs[worst] <= BOUND


# ---- the saturated attention slabs --------------------------------------------------------------------------------------------
UNMASKED = [(w, h, t, False, False) for w, h in vg.ATT_SHAPES for t in vg.SAT_TOKENS] + [(128, 2, vg.TIED_TOKENS, True, False)]
CAUSAL = [(w, h, t, False, True) for w, h in tc.ATT_SHAPES for t in tg.SAT_TOKENS] + [(128, 2, tg.TIED_TOKENS, True, True)]


@pytest.mark.parametrize("width,heads,tokens,tied,causal", UNMASKED + CAUSAL)
def test_saturated_slabs(width, heads, tokens, tied, causal):
    """the kernels' own expressions in fp32 (clip_like_cases.formula_f32) are within BOUND / 2 of float64 on every case: the
    bound is reachable; plain fp32 autograd is at least 10 x BOUND on the saturated slab from 17 tokens on: a kernel that took
    r from another key than the strongest would fail; the strongest keys of the slab's rows are the construction's and visit
    key 0, 63, 64 and L - 1 wherever a row of the construction can see them; in the tied slab two keys hold the maximum of every
    pointed row to the bit.
    Measured (width 128): formula_f32 1.3e-6 .. 3.3e-6 unmasked, 7.4e-7 .. 5.2e-6 causal; fp32 autograd 1.3e-3 .. 0.96"""
    B = vg.ATT_BATCH
    if causal:
        qkv, d_o, want = tg.saturated_case(width, heads, tokens, tied)
        mask = tc.causal_mask(tokens)
    else:
        qkv, d_o, want = vg.saturated_case(width, heads, tokens, tied)
        mask = vg.all_keys(tokens)
    assert bool(torch.isfinite(want).all())
    formula = tg.grad_figure(cl.formula_f32(qkv, d_o, B, heads, mask), want, B, heads)
    plain = tg.attention_grad(qkv, d_o, B, heads, mask, dtype=torch.float32)
    on_slab = tg.grad_figure(tg.slab(plain, B, heads, 0, 0), tg.slab(want, B, heads, 0, 0), 1, 1)
    print("%s (%d, %d) L = %d%s: formula_f32 %.3e; fp32 autograd on slab (0, 0) %.3e"
          % ("causal" if causal else "unmasked", width, heads, tokens, " tied" if tied else "", formula, on_slab))
    assert formula <= BOUND / 2
    if tokens >= 17:
        assert on_slab >= 10 * BOUND
    q, k, _ = tc.split_heads(qkv, B, heads)
    s = (q @ k.transpose(2, 3) / 8.0).masked_fill(~mask, -float("inf"))
    strongest = s[0, 0].argmax(dim=-1)
    target = tg.strongest_keys(tokens, causal)
    assert torch.equal(strongest, target)
    seen = set(strongest.tolist())
    if not causal:   # 37 is prime to every count here: the rows' strongest keys are a permutation of the keys
        assert seen == set(range(tokens))
        assert {key for key in (0, 63, 64, tokens - 1) if key < tokens} <= seen
    else:
        # row i takes (37 i + 5) mod (i + 1) = i - 31 from row 32 on: key 63 is row 94's, key 64 row 95's, so the second lane half
        # holds a strongest key at 128 tokens only; key L - 1 is visible to the last row alone, which takes key L - 32 (the tied
        # slab points that row at key 0, whose copy is key L - 1)
        assert 0 in seen
        if tokens >= 96:
            assert {0, 63, 64} <= seen and max(seen) == tokens - 32
    if tied:
        for i, j in tg.tied_targets(tokens, causal).items():
            row = s[1, 0, i]
            top = float(row.max())
            holders = (row == top).nonzero().flatten().tolist()
            twin = {63: 64, 0: tokens - 1}[j]
            if mask[i, twin]:
                assert holders == sorted([j, twin]), (i, holders)
            else:
                assert holders == [j], (i, holders)
        tied_rows = [i for i, j in tg.tied_targets(tokens, causal).items() if mask[i, {63: 64, 0: tokens - 1}[j]]]
        first = {tg.tied_targets(tokens, causal)[i] for i in tied_rows}
        assert first == {0, 63} and len(tied_rows) >= 2
