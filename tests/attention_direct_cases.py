"""Inputs and the float64 reference of the direct attention tests (test_gpu_attention_direct.py on the GPU,
test_attention_direct_premises.py on the host).  Split precision, L = 129: q | k | v as fp32 [B * L][3 * width], head h in columns
h * 64 .. h * 64 + 63 of each third -- the layout mpreid_vit_attention reads.

Data kinds
    plain        q, k ~ N(0, 2): the scaled scores q . k / 8 have a standard deviation of about 2; v ~ N(0, 1)
    spike<key>   the same with ONE key carrying about 0.4 of every row: channel 0 of every head is taken out of the noise (q = A for
                 every query, k = 0 for every key) and the spiked key is A on that channel and 0 elsewhere, so its score is
                 A * A / 8 = ln(0.4 / 0.6 * 128 e^2) for every query against a sum of exp over the 128 others of about 128 e^2
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
SPIKE_A = math.sqrt(8.0 * math.log(SPIKE_SHARE / (1.0 - SPIKE_SHARE) * (L - 1) * math.exp(2.0)))


@functools.lru_cache(maxsize=2)
def _plain(width, heads, batch):
    rng = np.random.default_rng(1000 * width + batch)
    qkv = rng.standard_normal((batch, L, 3, heads, 64), dtype=np.float32)
    qkv[:, :, :2] *= np.float32(math.sqrt(2.0))
    return torch.from_numpy(qkv)


def make_qkv(width, heads, batch, kind):
    """fp32 [batch * L, 3 * width] on the host"""
    assert width == 64 * heads and kind in KINDS
    t = _plain(width, heads, batch).clone()
    if kind.startswith("spike"):
        key = int(kind[5:])
        t[:, :, 0, :, 0] = SPIKE_A
        t[:, :, 1, :, 0] = 0.0
        t[:, key, 1, :, :] = 0.0
        t[:, key, 1, :, 0] = SPIKE_A
    elif kind == "magnitude":
        pair = torch.arange(batch * heads, dtype=torch.float32).view(batch, 1, heads, 1)
        t[:, :, 2] *= 1.0 + pair / 64.0
    return t.reshape(batch * L, 3 * width).contiguous()


def split_heads(qkv, batch, heads):
    """[batch * L, 3 * width] -> q, k, v as float64 [batch, heads, L, 64]"""
    t = qkv.double().view(batch, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def scores_f64(qkv, batch, heads):
    q, k, _ = split_heads(qkv, batch, heads)
    return q @ k.transpose(2, 3) / 8.0


def attention_f64(qkv, batch, heads, mutate=None):
    """float64 softmax(q k^T / 8) v of the fp32 inputs -> [batch, L, heads, 64]; `mutate` maps the scores the softmax sees"""
    _, _, v = split_heads(qkv, batch, heads)
    sc = scores_f64(qkv, batch, heads)
    if mutate is not None:
        sc = mutate(sc)
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).contiguous()


def slab_scale(qkv, batch, heads):
    """max |v| of every (image, head) slab -> float64 [batch, 1, heads, 1]"""
    _, _, v = split_heads(qkv, batch, heads)
    return v.abs().amax(dim=(2, 3)).view(batch, 1, heads, 1)


def error_figure(got, want, scale, rows=None):
    """got, want [batch, L, heads, 64] float64; the largest slab-relative error over rows [0, rows) of every image"""
    d = (got - want).abs() / scale
    if rows is not None:
        d = d[:, :rows]
    return float(d.max())


def check_premises(qkv, batch, heads, kind):
    """what the data is meant to be, in float64 on the host -> dict of figures (asserted here)"""
    sc = scores_f64(qkv, batch, heads)
    fig = {"score_std": float(sc.std())}
    if kind in ("plain", "magnitude"):
        assert 1.7 <= fig["score_std"] <= 2.3, fig
    if kind == "magnitude":
        # mean |v| of slab p is (1 + p / 64) * sqrt(2 / pi), within the sampling error of 129 * 64 values
        _, _, v = split_heads(qkv, batch, heads)
        mean = v.abs().mean(dim=(2, 3)).flatten()
        unit = mean / (1.0 + torch.arange(mean.numel(), dtype=torch.float64) / 64.0) / math.sqrt(2.0 / math.pi)
        fig["slab_unit_min"], fig["slab_unit_max"] = float(unit.min()), float(unit.max())
        assert 0.95 <= fig["slab_unit_min"] and fig["slab_unit_max"] <= 1.05, fig
    if kind.startswith("spike"):
        key = int(kind[5:])
        share = torch.softmax(sc, -1)[..., key]
        # (the sum over the other 128 keys is heavy-tailed: a row with one large ordinary score gives the spike less)
        fig["share_median"], fig["share_p05"], fig["share_max"] = (float(share.median()), float(share.flatten().quantile(0.05)),
                                                                    float(share.max()))
        assert 0.3 <= fig["share_median"] <= 0.5 and fig["share_p05"] >= 0.15 and fig["share_max"] <= 0.9, fig
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
    return fig


# a dropped or moved spiked key changes the float64 result by at least this (slab-relative): four orders of magnitude above
# the bounds of test_gpu_attention_direct.py
MUTANT_FLOOR = 5e-2
