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
`out` untouched; a second identical call gives the same bits; the rows of image i equal, bit for bit, a B = 1 call on that image's
slab (attention_direct_cases.checked_call, shared with test_gpu_attention_direct_forms.py).

Bound: PARENT_MAX_ERR below is the largest slab-relative error (attention_direct_cases.error_figure) of the kernel as it stood
before its LDS / addressing rework, per data kind, over all the shapes here, measured on an MI355X and recorded in
profiles/attention_direct_parent.json.  Asserted with a factor 2: a kernel that keeps the order of every row's floating-point
operations reproduces the bits, the factor only keeps the test from encoding one device's last digit."""
import ctypes as C

import pytest

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


def measure(width, heads, batch, kind):
    """every check of one case but the error bound (attention_direct_cases.checked_call) -> {q_tiles: error figure}"""
    host = adc.make_qkv(width, heads, batch, kind)
    prem = adc.check_premises(host[:3 * adc.L], min(batch, 3), heads, kind)
    want = adc.attention_f64(host, batch, heads)
    scale = adc.slab_scale(host, batch, heads)
    qkv = host.cuda()
    errs = {}
    for q_tiles in (0, 1):
        got, _ = adc.checked_call(qkv, batch, adc.L, heads, q_tiles, tag=kind)
        errs[q_tiles] = adc.error_figure(got, want, scale, rows=adc.written_rows(adc.L, q_tiles))
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
