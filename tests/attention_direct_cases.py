"""Inputs, the float64 reference and the per-call checks of the direct attention tests (test_gpu_attention_direct.py and
test_gpu_attention_direct_forms.py on the GPU, test_attention_direct_premises.py on the host).  q | k | v as [B * L][3 * width], head
h in columns h * 64 .. h * 64 + 63 of each third -- the layout mpreid_vit_attention reads; fp32 (the split mode, the all-fp32
seam) or the same values rounded to fp16 (the fp16 mode: the reference is computed from the ROUNDED values, so only the kernel's
arithmetic is measured).  Every function takes the token count; L = 129 below is the geometry of the first of the two GPU modules.

Data kinds
    plain        q, k ~ N(0, 2): the scaled scores q . k / 8 have a standard deviation of about 2; v ~ N(0, 1)
    spike<key>   the same with ONE key carrying about 0.4 of every row: channel 0 of every head is taken out of the noise (q = A for
                 every query, k = 0 for every key) and the spiked key is A on that channel and 0 elsewhere, so its score is
                 A * A / 8 = ln(0.4 / 0.6 * (L - 1) e^2) for every query against a sum of exp over the L - 1 others of about
                 (L - 1) e^2
    magnitude    plain, with v of (image b, head h) times 1 + (b * heads + h) / 64: every slab has a magnitude of its own

The error figure of a call is the largest, over its (image, head) slabs, of max |got - want| / max |v of the slab|: every output
row is a convex combination of the slab's v rows, so this is an error relative to the scale the slab's values live on."""
import functools
import math

import numpy as np
import torch

L = 129
SHAPES = [(128, 2), (768, 12)]                       # (width, heads)
SPIKE_KEYS = [128, 127, 112, 0]                      # 128: the key handled outside the matrix instructions
KINDS = ["plain"] + ["spike%d" % k for k in SPIKE_KEYS] + ["magnitude"]
SPIKE_SHARE = 0.4


def spike_a(tokens):
    """the value A of the spiked channel: A * A / 8 = ln(0.4 / 0.6 * (tokens - 1) e^2)"""
    return math.sqrt(8.0 * math.log(SPIKE_SHARE / (1.0 - SPIKE_SHARE) * (tokens - 1) * math.exp(2.0)))


SPIKE_A = spike_a(L)


def spike_keys(tokens):
    """[(name, key)] of the spiked keys of a token count, named relative to it, duplicates dropped (the first name stays):
    last = L - 1; last-1; tile = the first key of the last 16-key tile; 0; above 256 tokens block = the first key of the last
    64-key block of the streaming kernel and 64 = the first key of its second block.  4 <= L <= 32: last and 0; L <= 3: none"""
    if tokens <= 3:
        return []
    named = [("last", tokens - 1)]
    if tokens >= 33:
        named += [("last-1", tokens - 2), ("tile", 16 * ((tokens + 15) // 16 - 1))]
    named.append(("0", 0))
    if tokens > 256:
        named += [("block", 64 * ((tokens - 1) // 64)), ("64", 64)]
    seen, out = set(), []
    for name, key in named:
        if key not in seen:
            seen.add(key)
            out.append((name, key))
    return out


def kinds(tokens):
    """the data kinds of a token count: plain, spike<key> for every key of spike_keys, magnitude (L = 129: KINDS without
    spike112, the first key of the last tile the matrix instructions handle in attention_split_kernel<8,4,XKEY>)"""
    return ["plain"] + ["spike%d" % k for _, k in spike_keys(tokens)] + ["magnitude"]


@functools.lru_cache(maxsize=4)
def _plain(width, heads, batch, tokens=L):
    rng = np.random.default_rng(1000 * width + batch)
    qkv = rng.standard_normal((batch, tokens, 3, heads, 64), dtype=np.float32)
    qkv[:, :, :2] *= np.float32(math.sqrt(2.0))
    return torch.from_numpy(qkv)


def make_qkv(width, heads, batch, kind, tokens=L, dtype=torch.float32):
    """[batch * tokens, 3 * width] on the host: fp32, or the same tensor rounded to fp16"""
    assert width == 64 * heads and dtype in (torch.float32, torch.float16)
    assert kind in ("plain", "magnitude") or (kind.startswith("spike") and 0 <= int(kind[5:]) < tokens), kind
    t = _plain(width, heads, batch, tokens).clone()
    if kind.startswith("spike"):
        key = int(kind[5:])
        a = spike_a(tokens)
        if 33 <= tokens < 64:
            # The sum of exp over so few other keys is heavy-tailed enough for its median to fall well short of its mean,
            # (L - 1) e^2: at a score deviation of 2 the spiked key's median share sits AT 0.5, the edge of what check_premises
            # asks from 33 tokens on.  q times 1.05 -- a score deviation of 2.1 -- puts it near 0.45, as at the larger L
            t[:, :, 0] *= np.float32(1.05)
        t[:, :, 0, :, 0] = a
        t[:, :, 1, :, 0] = 0.0
        t[:, key, 1, :, :] = 0.0
        t[:, key, 1, :, 0] = a
    elif kind == "magnitude":
        pair = torch.arange(batch * heads, dtype=torch.float32).view(batch, 1, heads, 1)
        t[:, :, 2] *= 1.0 + pair / 64.0
    return t.reshape(batch * tokens, 3 * width).contiguous().to(dtype)


def split_heads(qkv, batch, heads):
    """[batch * tokens, 3 * width] -> q, k, v as float64 [batch, heads, tokens, 64]"""
    t = qkv.double().view(batch, qkv.shape[0] // batch, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def scores_f64(qkv, batch, heads):
    q, k, _ = split_heads(qkv, batch, heads)
    return q @ k.transpose(2, 3) / 8.0


def attention_f64(qkv, batch, heads, mutate=None):
    """float64 softmax(q k^T / 8) v of the inputs as they are -> [batch, tokens, heads, 64]; `mutate` maps the scores the softmax
    sees"""
    _, _, v = split_heads(qkv, batch, heads)
    sc = scores_f64(qkv, batch, heads)
    if mutate is not None:
        sc = mutate(sc)
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).contiguous()


def attention_host_f32(qkv, batch, heads):
    """the same formula in torch's fp32 on the CPU (of fp16 inputs: their values in fp32) -> float64 [batch, tokens, heads, 64]:
    what plain fp32 arithmetic makes of the case, printed beside the kernels' figures"""
    t = qkv.float().view(batch, qkv.shape[0] // batch, 3, heads, 64).permute(2, 0, 3, 1, 4)
    o = torch.softmax(t[0] @ t[1].transpose(2, 3) / 8.0, -1) @ t[2]
    return o.permute(0, 2, 1, 3).contiguous().double()


def slab_scale(qkv, batch, heads):
    """max |v| of every (image, head) slab -> float64 [batch, 1, heads, 1]"""
    _, _, v = split_heads(qkv, batch, heads)
    return v.abs().amax(dim=(2, 3)).view(batch, 1, heads, 1)


def error_figure(got, want, scale, rows=None):
    """got, want [batch, tokens, heads, 64] float64; the largest slab-relative error over rows [0, rows) of every image"""
    d = (got - want).abs() / scale
    if rows is not None:
        d = d[:, :rows]
    return float(d.max())


def check_premises(qkv, batch, heads, kind):
    """what the data is meant to be, in float64 on the host -> dict of figures (asserted here).  The token count is the input's.
    Spiked key, L >= 33: its share of the rows has a median in [0.3, 0.5], a 5th percentile >= 0.15 and a maximum <= 0.9;
    4 <= L <= 32 (few other keys: their sum of exp is noisier): median in [0.3, 0.6], 5th percentile >= 0.1.  Either way a
    kernel that drops the key, or hands its weight to a neighbouring row of v, is at least MUTANT_FLOOR away.  Spiked LAST key
    above 256 tokens: in at least half of the rows its score exceeds every earlier key's by >= 1, so the online softmax of the
    streaming kernel rescales in its last key block."""
    tokens = qkv.shape[0] // batch
    sc = scores_f64(qkv, batch, heads)
    fig = {"score_std": float(sc.std())}
    if kind in ("plain", "magnitude"):
        if tokens >= 33:
            assert 1.7 <= fig["score_std"] <= 2.3, fig
        else:
            # too few scores for their sample deviation to say much (L = 2, B = 1: eight): the premise is the operands', q, k of
            # variance 2, to five standard errors of a sample deviation, sqrt(2) / sqrt(2 n)
            q, k, _ = split_heads(qkv, batch, heads)
            for name, t in (("q_std", q), ("k_std", k)):
                fig[name] = float(t.std())
                assert abs(fig[name] / math.sqrt(2.0) - 1.0) <= 5.0 / math.sqrt(2.0 * t.numel()), fig
    if kind == "magnitude":
        # mean |v| of slab p is (1 + p / 64) * sqrt(2 / pi), within the sampling error of tokens * 64 values: 5 % at L = 129, and
        # five standard errors of the mean of |N(0, 1)| (deviation sqrt(1 - 2 / pi)) where that is more
        _, _, v = split_heads(qkv, batch, heads)
        mean = v.abs().mean(dim=(2, 3)).flatten()
        unit = mean / (1.0 + torch.arange(mean.numel(), dtype=torch.float64) / 64.0) / math.sqrt(2.0 / math.pi)
        fig["slab_unit_min"], fig["slab_unit_max"] = float(unit.min()), float(unit.max())
        tol = max(0.05, 5.0 * math.sqrt(1.0 - 2.0 / math.pi) / math.sqrt(2.0 / math.pi) / math.sqrt(64.0 * tokens))
        assert 1.0 - tol <= fig["slab_unit_min"] and fig["slab_unit_max"] <= 1.0 + tol, fig
    if kind.startswith("spike"):
        key = int(kind[5:])
        share = torch.softmax(sc, -1)[..., key]
        # (the sum over the other keys is heavy-tailed: a row with one large ordinary score gives the spike less)
        fig["share_median"], fig["share_p05"], fig["share_max"] = (float(share.median()), float(share.flatten().quantile(0.05)),
                                                                    float(share.max()))
        if tokens >= 33:
            assert 0.3 <= fig["share_median"] <= 0.5 and fig["share_p05"] >= 0.15 and fig["share_max"] <= 0.9, fig
        else:
            assert 0.3 <= fig["share_median"] <= 0.6 and fig["share_p05"] >= 0.1, fig
        want = attention_f64(qkv, batch, heads)
        scale = slab_scale(qkv, batch, heads)

        def drop(s):
            s = s.clone()
            s[..., key] = -float("inf")
            return s

        def move(s):   # the spiked key's score lands on a neighbouring key, i.e. another row of v gets its weight
            s = s.clone()
            other = key - 1 if key > 0 else 1
            s[..., [key, other]] = s[..., [other, key]]
            return s
        fig["mutant_drop"] = error_figure(attention_f64(qkv, batch, heads, drop), want, scale)
        fig["mutant_move"] = error_figure(attention_f64(qkv, batch, heads, move), want, scale)
        assert fig["mutant_drop"] >= MUTANT_FLOOR and fig["mutant_move"] >= MUTANT_FLOOR, fig
        if tokens > 256 and key == tokens - 1:
            lead = sc[..., key] - sc[..., :key].amax(-1)
            fig["rescale_rows"] = float((lead >= 1.0).double().mean())
            assert fig["rescale_rows"] >= 0.5, fig
    return fig


# a dropped or moved spiked key changes the float64 result by at least this (slab-relative): four orders of magnitude above
# the bounds of test_gpu_attention_direct.py, 25 times the loosest bound of test_gpu_attention_direct_forms.py
MUTANT_FLOOR = 5e-2


# ---- the cases of test_gpu_attention_direct_forms.py (the host module asserts the premises of every one) ------------------------
# both ends of every row of the dispatch table (test_gpu_attention_forms.py), the real geometries (99, 129, 211, 241, 257, 442),
# both sides of the streaming kernel's 64-key block edges (256 | 257, 258; 320 | 321) and the limit
FORMS_TOKENS = [2, 3, 17, 32, 33, 99, 128, 129, 130, 145, 160, 161, 192, 193, 211, 224, 225, 241, 256, 257, 258, 320, 321, 442, 1025]
# the all-fp32 seam: K / V resident up to 320 tokens, 128-key chunks above (384: three whole chunks, 385: one key more)
F32_TOKENS = [2, 17, 129, 256, 257, 320, 321, 384, 385, 1025]
# one token count per instantiation of the resident kernels (fp16 | split): <2,2>; <10,4,MASKALL> | <10,8>; <10,4,EXACT> | <8,4,XKEY>;
# <10,4,EXACT> | <10,8>; <14,8,MASKALL> | <14,8>; <14,8,EXACT> | <14,8>; <16,8,EXACT> | <16,8>
FORMS_ROWS = [17, 99, 129, 130, 177, 211, 241]
BOUND_SPLIT = 2e-5            # the project's slab-relative bar of a split attention kernel at its own seam (text_cases.BOUND_SPLIT)
BOUND_F32 = 2e-5              # BOUND["fp32"] of test_gpu_attention_forms.py
# fp16 operands, from the kernels' arithmetic: every output row is a convex combination of the slab's v rows; rounding P to fp16
# costs at most 2^-11 max|v| in the numerator and the same through the denominator, the fp16 store of O another 2^-11 max|v|;
# fp32 accumulation and the exponential's error sit orders of magnitude below; the fourth 2^-11 is slack for subnormal P
BOUND_F16 = 4.0 * 2.0 ** -11


def forms_shapes(tokens):
    """[(width, heads, batch)] of mpreid_vit_attention at a token count (the float64 reference of 12 heads above 257 tokens is
    not worth its time)"""
    if tokens <= 256:
        return [(w, h, b) for w, h in SHAPES for b in (1, 3)]
    return [(128, 2, 1), (128, 2, 3)] + ([(768, 12, 1)] if tokens == 257 else [])


def f32_shapes(tokens):
    return [(128, 2, 1), (128, 2, 3)] + ([(768, 12, 1)] if tokens in (129, 321) else [])


def q_tiles_of(tokens, kind):
    """the q_tiles a case runs.  T = ceil(L / 16) tiles.  plain and the spiked last key: 0, 1, 2 (L > 32: below that 2 tiles are
    all of them), T - 1 (>= 3: the largest partial call), T and T + 3 (all rows, asked for by number), and above 256 tokens 8 and
    9: the streaming launcher's one-group and two-group splits of a partial call.  Every other kind: 0 and 1"""
    if kind not in ("plain", "spike%d" % (tokens - 1)):
        return [0, 1]
    T = (tokens + 15) // 16
    qs = {0, 1, T, T + 3}
    if tokens > 32:
        qs.add(2)
    if T - 1 >= 3:
        qs.add(T - 1)
    if tokens > 256:
        qs |= {8, 9}
    return sorted(qs)


def premise_cases():
    """every (tokens, width, heads, kind) either seam's tests run -- B = 1 and 3 share the recipe: the premises are asserted at 3"""
    seen, out = set(), []
    rows_shapes = lambda tokens: [(128, 2, 8)]   # noqa: E731  (the wrapped persistent loop and the swapped-rows test)
    for tokens_list, shapes in ((FORMS_TOKENS, forms_shapes), (F32_TOKENS, f32_shapes), (FORMS_ROWS, rows_shapes)):
        for tokens in tokens_list:
            for w, h, _ in shapes(tokens):
                for kind in kinds(tokens):
                    if (tokens, w, h, kind) not in seen:
                        seen.add((tokens, w, h, kind))
                        out.append((tokens, w, h, kind))
    return out


# ---- one call on the GPU and everything about it that needs no reference ------------------------------------------------------
GUARD_ROWS = 8
NAN_BITS = 0x7E01          # an fp16 NaN
NAN_BITS_F32 = 0x7FC00A01  # an fp32 NaN


def written_rows(tokens, q_tiles):
    """the rows of every image a call writes (include/mpreid.h): min(16 q_tiles, tokens), all of them for q_tiles 0"""
    return tokens if q_tiles == 0 or 16 * q_tiles >= tokens else 16 * q_tiles


def guarded_call(qkv, batch, tokens, heads, q_tiles=0, f32=False):
    """one launch into a NaN-filled buffer with guard rows -> (out [batch * tokens, cols] (a view), its bits as integers); the
    guards are checked.  qkv fp16: mpreid_vit_attention in the fp16 mode, out fp16 [.., width]; fp32: the split mode, out fp16
    [.., 2 * width] = [hi | lo]; fp32 with f32 = True: mpreid_vit_attention_f32, out fp32 [.., width]"""
    from mpreid import ops
    width = 64 * heads
    rows = batch * tokens
    if f32:
        assert q_tiles == 0 and qkv.dtype == torch.float32
        buf = torch.empty((rows + 2 * GUARD_ROWS, width), dtype=torch.float32, device=qkv.device)
        bits, pattern = buf.view(torch.int32), NAN_BITS_F32
    else:
        cols = 2 * width if qkv.dtype == torch.float32 else width
        buf = torch.empty((rows + 2 * GUARD_ROWS, cols), dtype=torch.float16, device=qkv.device)
        bits, pattern = buf.view(torch.int16), NAN_BITS
    bits.fill_(pattern)
    out = buf[GUARD_ROWS:GUARD_ROWS + rows]
    if f32:
        ops.vit_attention_f32(qkv, batch, tokens, heads, out=out)
    else:
        ops.vit_attention(qkv, batch, tokens, heads, q_tiles=q_tiles, out=out)
    torch.cuda.synchronize()
    assert bool((bits[:GUARD_ROWS] == pattern).all()) and bool((bits[GUARD_ROWS + rows:] == pattern).all()), "guard rows written"
    return out, bits[GUARD_ROWS:GUARD_ROWS + rows]


def checked_call(qkv, batch, tokens, heads, q_tiles=0, f32=False, tag=()):
    """One call of the seam on a device tensor, with every check that needs no reference:
      * `out` lies between guard rows and is pre-filled with a NaN pattern: the guards and every row that must not be written
        (q_tiles n > 0: the rows from 16 n on of every image) hold the pattern afterwards, bit for bit;
      * every written row is finite;
      * a second identical call gives the same bits;
      * batch > 1: the rows of image i equal, bit for bit, a batch = 1 call on that image's slab.
    -> (values float64 [batch, tokens, heads, 64] on the host -- hi + lo in the split mode; rows that were not written are NaN --,
        the bits of the output [batch, tokens, cols] on the device)"""
    width = 64 * heads
    pattern = NAN_BITS_F32 if f32 else NAN_BITS
    written = written_rows(tokens, q_tiles)
    out, bits = guarded_call(qkv, batch, tokens, heads, q_tiles, f32)
    o3, b3 = out.view(batch, tokens, -1), bits.view(batch, tokens, -1)
    assert bool(torch.isfinite(o3[:, :written]).all()), (tag, q_tiles, "a written row is not finite")
    assert bool((b3[:, written:] == pattern).all()), (tag, q_tiles, "a row beyond the asked tiles was written")
    again = guarded_call(qkv, batch, tokens, heads, q_tiles, f32)[1].view(batch, tokens, -1)
    assert torch.equal(again, b3), (tag, q_tiles, "a second identical call gave other bits")
    if batch > 1:
        single = torch.empty_like(b3)
        for i in range(batch):
            single[i] = guarded_call(qkv[i * tokens:(i + 1) * tokens], 1, tokens, heads, q_tiles, f32)[1]
        same = (single[:, :written] == b3[:, :written]).all(-1).all(-1)
        assert bool(same.all()), (tag, q_tiles, "images that differ from their B = 1 call", (~same).nonzero()[:8].flatten().tolist())
    if o3.shape[2] == 2 * width:
        vals = o3[..., :width].double() + o3[..., width:].double()
    else:
        vals = o3.double()
    return vals.cpu().view(batch, tokens, heads, 64), b3
