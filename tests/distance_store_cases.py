"""The case matrix of the stored-distance kernels' STORE paths, on integer features: test infrastructure, not product.

euclidean_distance has three arithmetic modes; the two fp16 ones reach five kernel forms of csrc/gemm_f16.hip (128x128,
persistent 256x256 two-tensor / symmetric, two-workgroups-per-CU 256x128 symmetric / two-tensor), and each form picks its
store path per tile at run time: 16-byte stores when ldo % 4 == 0 and the output pointer is 16-byte aligned (`vec_ok`),
else one float per lane; an interior fast path without bounds; 4-packs that straddle n_valid (m_valid in a mirrored store)
degrade to 1-3 scalar stores; the symmetric forms store every off-diagonal tile a second time, transposed; tiles wholly
past the valid range store nothing.

Integer features make all of that a question of EQUALITY: every operand is an fp16 value, every product and every fp32
partial sum is an integer below 2^24, the 3-term split's per-row power-of-two scale leaves hi exact and lo == 0, so
GEMM_F16_FAST, GEMM_F16_SPLIT3 and GEMM_F32_EXACT must all return float32(|q|^2 + |g|^2 - 2 q.g) of plain integer
arithmetic (tests/test_distance_store_cases_cpu.py re-asserts the premise for every case below).  The row-dependent power of
two gives neighbouring rows different split exponents: a wrong rscale / cscale index is off by a factor of two.

The output is a block of a larger allocation filled with FILL: GUARD_ROWS rows below it and, where ldo > ng, columns left
and right of it.  After the call the block equals the expectation and EVERY other element still holds FILL.

Importable (tests/test_gpu_distance_stores.py runs the matrix in-process on the default dispatch) and runnable as a child
script -- MPREID_TUNE, which forces a kernel form, is latched per process:
    python tests/distance_store_cases.py fast split3
prints the device's CU count, one line per (case, mode) -- "CASE <id> <mode> ok", or the first mismatching index with both
values -- and exits non-zero if any case failed.
"""
import collections
import functools
import os
import sys

import numpy as np

FILL = -7.0
GUARD_ROWS = 8
NQ = 300                  # two tensors: 2 tile rows of 256 (3 of 128), the second ragged
D_VALUES = (40, 200)      # K padded to 64 (one 64-wide stage; split K = 192) and to 256 (split K = 768)
MODES = ("fast", "split3", "exact")

# (name, ng, ldo (None: ng), col_offset).  ng = 600 ... 603 pad to 768: 3 tiles of 256 / 6 of 128, the last column tile of
# 256 ragged, the fifth of 128 ragged (rows 512-639 hold 88 ... 91 valid), the sixth wholly past n_valid.
#   a   vec_ok, ng % 4 == 0: 16-byte stores, no partial 4-pack
#   b   ldo odd: not vec_ok, the scalar path
#   c*  vec_ok with ng % 4 == 1, 2, 3: partial 4-packs.  (A mirrored store runs along m, and a tile above the diagonal never
#       lies in the last tile row: with vec_ok its packs are always whole, what is ragged there is the row bound n < n_valid;
#       its one-to-four scalar stores run in b, d and e.)
#   d   ldo % 4 == 0 but the pointer is 4 bytes past a 16-byte boundary: not vec_ok
#   e   ldo odd inside a wider matrix
# Not covered: the fast paths' fall-back for ldo >= 2^24 (an interior tile there needs a 17 GB output).
GEOMETRIES = (
    ("a", 600, None, 0),
    ("b", 601, None, 0),
    ("c1", 601, 640, 16),
    ("c2", 602, 640, 16),
    ("c3", 603, 640, 16),
    ("d", 602, 640, 17),
    ("e", 603, 641, 16),
)
# two:   q [NQ, d] and g [ng, d]
# same:  one tensor [ng, d] passed twice -- the same pointer takes the symmetric forms
# clone: one tensor and its clone -- the full computation of the same matrix
OPERANDS = ("two", "same", "clone")

Case = collections.namedtuple("Case", "operands geom nq ng ldo col_offset d")


def _cases():
    out = []
    for operands in OPERANDS:
        for name, ng, ldo, off in GEOMETRIES:
            for d in D_VALUES:
                out.append(Case(operands, name, NQ if operands == "two" else ng, ng, ng if ldo is None else ldo, off, d))
    return tuple(out)


CASES = _cases()


def case_id(c: Case) -> str:
    return f"{c.operands}-{c.geom}-{c.nq}x{c.ng}x{c.d}-ldo{c.ldo}+{c.col_offset}"


# ---- the integer family ---------------------------------------------------------------------------------------------
def int_features(n: int, d: int, seed: int) -> np.ndarray:
    """int64 [n, d]: integers in -4 .. 4 times 2^(row % 5), column 0 shifted by row % 3 (no two rows alike), row 7 zero;
    |x| <= 66"""
    rng = np.random.default_rng(seed)
    row = np.arange(n)
    x = rng.integers(-4, 5, size=(n, d)).astype(np.int64) * (1 << (row % 5))[:, None]
    x[:, 0] += row % 3
    if n > 7:
        x[7] = 0
    return x


def expected_euclid(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """int64 [nq, ng] = |q|^2 + |g|^2 - 2 q.g.  The dot products go through a float64 matrix product (numpy's integer one
    is not a BLAS call): every partial sum is an integer far below 2^53, so it is exact and the conversion back loses
    nothing."""
    assert q.dtype == np.int64 and g.dtype == np.int64
    dot = q.astype(np.float64) @ g.astype(np.float64).T
    doti = dot.astype(np.int64)
    assert np.array_equal(doti.astype(np.float64), dot)
    return (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2 * doti


@functools.lru_cache(maxsize=None)
def operands_of(operands: str, nq: int, ng: int, d: int):
    """(q int64, g int64, expected int64) of a case; g is q for "same" and "clone".  Cached: the geometries share them."""
    g = int_features(ng, d, seed=1000 + ng + d)
    q = int_features(nq, d, seed=7 + d) if operands == "two" else g
    want = expected_euclid(q, g)
    for a in (q, g, want):
        a.setflags(write=False)
    return q, g, want


def split3_pack(x: np.ndarray):
    """csrc/gemm_f16.hip split3_pack_kernel on the host, Euclidean epilogue: (v = x * sc in float32, hi, lo in float16, sc)
    with sc = 2^(10 - ex), ex the binary exponent of the row's float32 norm (sc = 1 for a zero row)"""
    xf = x.astype(np.float32)
    sqn = (xf * xf).sum(1, dtype=np.float32)
    nrm = np.sqrt(sqn, dtype=np.float32)
    _, ex = np.frexp(nrm)
    sc = np.where(nrm > 0, np.ldexp(np.float32(1.0), 10 - ex), np.float32(1.0)).astype(np.float32)
    v = xf * sc[:, None]
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return v, hi, lo, sc


# ---- the cosine epilogue's features ---------------------------------------------------------------------------------
COS_NQ, COS_NG, COS_D = 130, 259, 100
COS_PLANT_Q, COS_PLANT_POS, COS_PLANT_NEG, COS_ZERO_G = 5, 3, 4, 200
COS_GEOMETRIES = (("a", None, 0), ("c", 640, 16), ("d", 640, 17))     # (name, ldo (None: ng), col_offset), as above


def cosine_features():
    """(q [130, 100], g [259, 100]) float32 Gaussian rows, not normalised, with g[3] = 2.5 q[5] (cosine 1), g[4] = -q[5]
    (cosine -1) and g[200] = 0 (a zero norm: the reference's 0 * (1 / 0) = NaN)"""
    rng = np.random.default_rng(2024)
    q = rng.standard_normal((COS_NQ, COS_D)).astype(np.float32)
    g = rng.standard_normal((COS_NG, COS_D)).astype(np.float32)
    g[COS_PLANT_POS] = np.float32(2.5) * q[COS_PLANT_Q]
    g[COS_PLANT_NEG] = -q[COS_PLANT_Q]
    g[COS_ZERO_G] = 0.0
    return q, g


def cosine_f64(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """the cosines themselves (before clip and arccos) in float64 on the float32 inputs; NaN in the zero row's column"""
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (q64 @ g64.T) * (1.0 / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(g64, axis=1)[None, :]))


# ---- running a case on the GPU --------------------------------------------------------------------------------------
def guarded_output(torch, nq: int, ldo: int):
    """([nq + GUARD_ROWS, ldo] filled with FILL, its first nq rows -- what a caller passes as `out`)"""
    alloc = torch.full((nq + GUARD_ROWS, ldo), FILL, dtype=torch.float32, device="cuda")
    return alloc, alloc[:nq]


def first_mismatch(got: np.ndarray, want: np.ndarray, nq: int, ng: int, col_offset: int):
    """None, or a sentence naming the first element (row-major) of the allocation where got != want bit for bit"""
    bad = got.view(np.uint32) != want.view(np.uint32)
    if not bad.any():
        return None
    r, c = (int(v) for v in np.argwhere(bad)[0])
    where = "block" if r < nq and col_offset <= c < col_offset + ng else "guard"
    return (f"{int(bad.sum())} elements differ, first at allocation [{r}, {c}] ({where}; block row {r}, block column "
            f"{c - col_offset}): got {got[r, c]!r}, want {want[r, c]!r}")


_device_features = {}


def _device(torch, x: np.ndarray):
    key = id(x)         # (operands_of caches its arrays for the life of the process)
    if key not in _device_features:
        _device_features[key] = (x, torch.from_numpy(x.astype(np.float32)).cuda())
    return _device_features[key][1]


def run_case(c: Case, mode: str):
    """None if the case passed in `mode`, else first_mismatch's sentence"""
    import torch
    from mpreid import ops
    q, g, want = operands_of(c.operands, c.nq, c.ng, c.d)
    qt = _device(torch, q)
    gt = qt if c.operands == "same" else qt.clone() if c.operands == "clone" else _device(torch, g)
    assert (gt.data_ptr() == qt.data_ptr()) == (c.operands == "same")
    alloc, out = guarded_output(torch, c.nq, c.ldo)
    m = {"fast": ops.GEMM_F16_FAST, "split3": ops.GEMM_F16_SPLIT3, "exact": ops.GEMM_F32_EXACT}[mode]
    ops.euclidean_distance(qt, gt, mode=m, out=out, col_offset=c.col_offset)
    full = np.full((c.nq + GUARD_ROWS, c.ldo), FILL, np.float32)
    full[:c.nq, c.col_offset:c.col_offset + c.ng] = want.astype(np.float32)
    return first_mismatch(alloc.cpu().numpy(), full, c.nq, c.ng, c.col_offset)


def run_matrix(modes, emit=print):
    """every case in every mode of `modes`; one line each through `emit`; -> the list of failed "<id> <mode>" """
    failed = []
    for mode in modes:
        for c in CASES:
            msg = run_case(c, mode)
            emit(f"CASE {case_id(c)} {mode} {'ok' if msg is None else 'MISMATCH: ' + msg}")
            if msg is not None:
                failed.append(f"{case_id(c)} {mode}")
    return failed


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "mp-reid_amd")]
    import ctypes as C
    from mpreid import _lib
    modes = argv or ["fast", "split3"]
    assert all(m in MODES for m in modes), modes
    _lib.require_gpu()
    cus = C.c_int(0)
    _lib.check(_lib.load().mpreid_device_info(None, 0, C.byref(cus), None), "mpreid_device_info")
    print("CUS", cus.value, flush=True)
    failed = run_matrix(modes, emit=lambda s: print(s, flush=True))
    print(f"DONE {len(CASES) * len(modes) - len(failed)} of {len(CASES) * len(modes)} passed", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
