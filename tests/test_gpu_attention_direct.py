"""The split-precision attention kernel of L = 129 (attention_split_kernel<8,4,XKEY>) called directly through
mpreid_vit_attention, every written row against float64.  Through a whole encoder an error in a row other than CLS of the last
block is invisible, and the 2e-5 feature bound is far looser than the kernel's own accuracy.

Shapes: (width, heads) = (128, 2) and (768, 12); B = 1, 3, the smallest B with B * heads beyond the persistent grid (2 workgroups
per CU x the CU count: grid and heads are both even, so B * heads = grid + 1 cannot be had at these widths -- 2 and 4 workgroups
wrap; (64, 1) at B = grid + 1 is the case in which exactly ONE wraps) and a B about 20 % beyond the grid; q_tiles 0 and 1.
Data: attention_direct_cases.py (plain, one spiked key at 128 / 127 / 112 / 0, a magnitude per slab), premises asserted in float64
before the GPU is touched.

Checks, per case: hi + lo of every written row against float64 softmax(q k^T / 8) v of the same fp32 inputs; `out` pre-filled with a
NaN pattern, every row finite afterwards (q_tiles 1: rows 0 .. 15 finite, every other row untouched); guard rows before and after
`out` untouched; the rows of image i equal, bit for bit, a B = 1 call on that image's slab.

Bound: PARENT_MAX_ERR below is the largest slab-relative error (attention_direct_cases.error_figure) of the kernel as it stood
before its LDS / addressing rework, per data kind, over all the shapes here, measured on an MI355X and recorded in
profiles/attention_direct_parent.json.  Asserted with a factor 2: a kernel that keeps the order of every row's floating-point
operations reproduces the bits, the factor only keeps the test from encoding one device's last digit."""
import ctypes as C

import pytest
import torch

import attention_direct_cases as adc

pytestmark = pytest.mark.gpu

PARENT_MAX_ERR = {
    "plain": 7.453478467263816e-07,
    "spike128": 7.27453758846112e-07,
    "spike127": 7.429965811402355e-07,
    "spike112": 8.181035212057862e-07,
    "spike0": 8.007095706326771e-07,
    "magnitude": 7.38512629973661e-07,
}
GUARD_ROWS = 8
NAN_BITS = 0x7E01   # an fp16 NaN


def persistent_grid():
    from mpreid import _lib
    cus = C.c_int(0)
    _lib.require_gpu()
    _lib.check(_lib.load().mpreid_device_info(None, 0, C.byref(cus), None), "mpreid_device_info")
    assert cus.value > 0
    return 2 * cus.value


def batch_of(which, heads):
    if which in ("1", "3"):
        return int(which)
    grid = persistent_grid()
    if which == "wrap":          # the smallest B with B * heads > grid
        return grid // heads + 1
    assert which == "wrap20"
    return -(-(grid * 12 // 10) // heads)


def _call(qkv, batch, heads, q_tiles):
    """one launch into a NaN-filled buffer with guard rows -> fp16 [batch * L, 2 * width] (a view); the guards are checked"""
    from mpreid import ops
    width = 64 * heads
    rows = batch * adc.L
    buf = torch.empty((rows + 2 * GUARD_ROWS, 2 * width), dtype=torch.float16, device=qkv.device)
    buf.view(torch.int16).fill_(NAN_BITS)
    out = buf[GUARD_ROWS:GUARD_ROWS + rows]
    ops.vit_attention(qkv, batch, adc.L, heads, q_tiles=q_tiles, out=out)
    torch.cuda.synchronize()
    bits = buf.view(torch.int16)
    assert bool((bits[:GUARD_ROWS] == NAN_BITS).all()) and bool((bits[GUARD_ROWS + rows:] == NAN_BITS).all()), "guard rows written"
    return out


def measure(width, heads, batch, kind):
    """every check of one case but the error bound -> {q_tiles: error figure}"""
    host = adc.make_qkv(width, heads, batch, kind)
    prem = adc.check_premises(host[:3 * adc.L], min(batch, 3), heads, kind)
    want = adc.attention_f64(host, batch, heads)
    scale = adc.slab_scale(host, batch, heads)
    qkv = host.cuda()
    errs = {}
    for q_tiles in (0, 1):
        out = _call(qkv, batch, heads, q_tiles)
        o3 = out.view(batch, adc.L, 2 * width)
        written = adc.L if q_tiles == 0 else 16
        assert bool(torch.isfinite(o3[:, :written]).all()), (kind, q_tiles, "a written row is not finite")
        if q_tiles:
            assert bool((o3[:, written:].view(torch.int16) == NAN_BITS).all()), (kind, q_tiles, "a row beyond the tile was written")
        got = (o3[..., :width].double() + o3[..., width:].double()).cpu().view(batch, adc.L, heads, 64)
        errs[q_tiles] = adc.error_figure(got, want, scale, rows=written)
        # image i of the large call against a B = 1 call on its slab, bit for bit
        if batch > 1:
            single = torch.empty_like(o3)
            for i in range(batch):
                single[i] = _call(qkv[i * adc.L:(i + 1) * adc.L], 1, heads, q_tiles)
            same = (single.view(torch.int16)[:, :written] == o3.view(torch.int16)[:, :written]).all(-1).all(-1)
            assert bool(same.all()), (kind, q_tiles, "images that differ from their B = 1 call", (~same).nonzero()[:8].flatten().tolist())
    print("ATTDIRECT width=%d heads=%d B=%d kind=%s err q_tiles0=%.3e q_tiles1=%.3e premises %s"
          % (width, heads, batch, kind, errs[0], errs[1], prem))
    return errs


CASES = [(w, h, which) for w, h in adc.SHAPES for which in ("1", "3", "wrap", "wrap20")] + [(64, 1, "wrap")]


@pytest.mark.parametrize("kind", adc.KINDS)
@pytest.mark.parametrize("width,heads,which", CASES)
def test_attention_direct_vs_float64(width, heads, which, kind):
    batch = batch_of(which, heads)   # (heads 1: grid + 1)
    shape = (width, heads)
    errs = measure(width, heads, batch, kind)
    for q_tiles, err in errs.items():
        assert err <= 2.0 * PARENT_MAX_ERR[kind], (shape, batch, kind, q_tiles, err, PARENT_MAX_ERR[kind])
