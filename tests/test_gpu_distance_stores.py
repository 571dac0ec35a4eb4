"""Every store path of the stored-distance kernels, pinned bit for bit on integer features (tests/distance_store_cases.py:
the case matrix, why the expectation is exact, the guard rows and columns), and the cosine epilogue at its edges.

The fp16 modes reach five kernel forms (csrc/gemm_f16.hip); MPREID_TUNE, which forces one, is latched per process, so the
matrix runs once per forced form in a fresh child process -- one at a time -- with verbose=1, and the launcher's
"[mpreid] gemm epi 5: ..." lines (one per distinct kernel, tile grid and launch grid of the process) must be EXACTLY the ones
the case list implies: a case that quietly took another kernel fails.  The default dispatch and the exact fp32 kernel run
the same matrix in-process."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distance_store_cases as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "distance_store_cases.py")
EPI_EUCLID = 5                      # csrc/gemm_f16.h GE_EUCLID

# Padded sizes of the matrix: rows 300 -> 512, 600 ... 603 -> 768 (both operands are padded to 256).
# tune -> what launch_one must have said for the Euclidean epilogue, given the device's CU count
P2_GRID = "grid {p2}"               # the two-workgroups-per-CU kernel: max(8, 2 * CUs rounded down to 8) workgroups
FORMS = {
    "gemm_big=0": (
        "128x128, 4x6 tiles, grid 24",                                                # two tensors
        "128x128, 6x6 tiles, grid 36",                                                # one tensor twice, tensor and clone
    ),
    "gemm_big=2,dist_sym_p2=0": (
        "persistent 256x256, walk strided, 2x3 tiles, grid 6",                        # two tensors
        "persistent 256x256, walk strided, 3x3 tiles, grid 9",                        # tensor and clone
        "persistent 256x256 (symmetric), walk strided, 3x3 tiles, grid 9",            # one tensor twice
    ),
    # dist_sym_p2=3: the symmetric form for the 3-term split operands as well (2 would leave them on the persistent kernel)
    "gemm_big=2,dist_sym_p2=3,dist_p2_full=2": (
        "two workgroups per CU 256x128 (two tensors), 2x6 tiles, " + P2_GRID,
        "two workgroups per CU 256x128 (two tensors), 3x6 tiles, " + P2_GRID,
        "two workgroups per CU 256x128 (symmetric), 3x6 tiles, " + P2_GRID,
    ),
}


def test_forms_table_matches_the_case_list():
    """the tile counts above are those of the case list (a shape edited there must be edited here)"""
    pad = lambda n: (n + 255) // 256 * 256
    assert {(pad(c.nq), pad(c.ng)) for c in S.CASES if c.operands == "two"} == {(512, 768)}
    assert {(pad(c.nq), pad(c.ng)) for c in S.CASES if c.operands != "two"} == {(768, 768)}


@pytest.mark.parametrize("tune", list(FORMS))
def test_store_paths_on_a_forced_kernel_form(tune):
    """GEMM_F16_FAST and GEMM_F16_SPLIT3 over the whole matrix on one forced kernel form (a child process)"""
    env = dict(os.environ, MPREID_TUNE=tune + ",verbose=1")
    r = subprocess.run([sys.executable, SCRIPT, "fast", "split3"], env=env, capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    cases = [ln for ln in lines if ln.startswith("CASE ")]
    print("\n".join(ln for ln in lines if not ln.endswith(" ok")))
    said = sorted(ln for ln in r.stderr.splitlines() if ln.startswith(f"[mpreid] gemm epi {EPI_EUCLID}: "))
    print("\n".join(said))
    bad = [ln for ln in cases if not ln.endswith(" ok")]
    assert r.returncode == 0 and not bad, (tune, bad[:10], r.stdout[-1500:], r.stderr[-3000:])
    want_cases = [f"CASE {S.case_id(c)} {mode} ok" for mode in ("fast", "split3") for c in S.CASES]
    assert cases == want_cases, (tune, len(cases), len(want_cases))
    cus = int([ln for ln in lines if ln.startswith("CUS ")][0].split()[1])
    p2 = max(8, (2 * cus) & ~7)
    want = sorted(f"[mpreid] gemm epi {EPI_EUCLID}: " + form.format(p2=p2) for form in FORMS[tune])
    assert said == want, (tune, said, want)


def _default_dispatch():
    assert "gemm_big" not in os.environ.get("MPREID_TUNE", ""), "these cases test the default dispatch"


@pytest.mark.parametrize("mode", ["fast", "split3"])
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_store_paths_default_dispatch(c, mode):
    """the kernel the production dispatch picks for these sizes, in-process"""
    _default_dispatch()
    msg = S.run_case(c, mode)
    assert msg is None, (S.case_id(c), mode, msg)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_store_paths_exact_mode(c):
    """GEMM_F32_EXACT (csrc/distance.hip): two tensors, and `q is g` -- the upper-triangular tiles with mirrored stores"""
    msg = S.run_case(c, "exact")
    assert msg is None, (S.case_id(c), msg)


# ---- the cosine epilogue ---------------------------------------------------------------------------------------------
CLIP_HI = np.float32(1.0 - 0.00001)          # utils/metrics.py: np.clip of a float32 matrix at 1 - epsilon
FAST_DOT = 1.5e-4                            # half the one-pass fp16 mode's stated 3e-4 on unit rows, which is 2 |delta(q.g)|


@pytest.fixture(scope="module")
def cosine_refs():
    q, g = S.cosine_features()
    c64 = S.cosine_f64(q, g)
    with np.errstate(invalid="ignore"):
        ref64 = np.arccos(np.clip(c64, -np.float64(CLIP_HI), np.float64(CLIP_HI)))
    want_orc = orc.cosine_similarity(q, g)
    for a in (q, g, c64, ref64, want_orc):
        a.setflags(write=False)
    return q, g, c64, ref64, want_orc


def _ulps(x, n):
    return n * float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("mode", ["exact", "split3", "fast"])
@pytest.mark.parametrize("geom,ldo,col_offset", S.COS_GEOMETRIES, ids=[g[0] for g in S.COS_GEOMETRIES])
def test_cosine_epilogue(cosine_refs, mode, geom, ldo, col_offset):
    """arccos(clip(q.g / (|q||g|))) on unnormalised rows with a cosine of +1, one of -1 and a zero-norm gallery row, written
    into a guarded block: EXACT within 2e-6 of the oracle, SPLIT3 within 1e-5 of a float64 evaluation, FAST within
    1.5e-4 / sqrt(1 - c^2) + 1e-6 of it (d arccos / dc times the mode's dot-product bar).  The zero row's column is NaN, as
    in the reference (0 * (1 / 0)), and nothing else is.  EXACT / SPLIT3 clip the planted entries: arccos(float32(1 - 1e-5))
    and pi minus it, within 4 ulp.  FAST rounds the operands before the dot but not the norms, so its planted cosines may
    stay below the clip: finite, within [arccos(hi), arccos(hi - 1.5e-4)] (mirrored about pi / 2 for -1), the ends taken
    with the same 4 ulp of float32 arccos.  Measured (MI355X): EXACT 2.4e-7 from the oracle, SPLIT3 2.3e-7 from float64,
    FAST 1.47e-4 at most and 0.96 of its per-entry bound at worst (the operands' fp16 rounding alone gives a 4.2-sigma
    entry of 33 670 about 1.7e-4 here: the bound has no slack to spare, and the result is deterministic); the planted
    entries reach the clip in all three modes."""
    from mpreid import ops
    q, g, c64, ref64, want_orc = cosine_refs
    nq, ng = q.shape[0], g.shape[0]
    ldo = ng if ldo is None else ldo
    alloc, out = S.guarded_output(torch, nq, ldo)
    m = {"fast": ops.GEMM_F16_FAST, "split3": ops.GEMM_F16_SPLIT3, "exact": ops.GEMM_F32_EXACT}[mode]
    ops.cosine_similarity(torch.tensor(q), torch.tensor(g), mode=m, out=out, col_offset=col_offset)
    full = alloc.cpu().numpy()
    got = full[:nq, col_offset:col_offset + ng]
    outside = np.ones(full.shape, bool)
    outside[:nq, col_offset:col_offset + ng] = False
    assert (full[outside] == S.FILL).all(), np.argwhere(outside & (full != S.FILL))[:5]
    zero = np.zeros(got.shape, bool)
    zero[:, S.COS_ZERO_G] = True
    assert np.array_equal(np.isnan(want_orc), zero)                      # the oracle keeps the reference's NaN
    assert np.array_equal(np.isnan(got), zero), np.argwhere(np.isnan(got) != zero)[:5]
    plants = [(S.COS_PLANT_Q, S.COS_PLANT_POS, False), (S.COS_PLANT_Q, S.COS_PLANT_NEG, True)]
    rest = ~zero
    for i, j, _ in plants:
        rest[i, j] = False
    err = np.abs(got.astype(np.float64) - ref64)
    a_hi = math.acos(float(CLIP_HI))
    if mode == "exact":
        bound = np.full(got.shape, 2e-6)
        worst = float(np.abs(got[~zero] - want_orc[~zero]).max())
        print(f"cosine {mode} {geom}: max |got - oracle| {worst:.3e}")
        assert worst <= 2e-6, worst
    elif mode == "split3":
        bound = np.full(got.shape, 1e-5)
    else:
        bound = FAST_DOT / np.sqrt(1.0 - np.where(rest, c64, 0.0) ** 2) + 1e-6
    if mode != "exact":
        print(f"cosine {mode} {geom}: max |got - float64| {float(err[rest].max()):.3e}, largest share of the bound "
              f"{float((err[rest] / bound[rest]).max()):.3f}")
        assert (err[rest] <= bound[rest]).all(), (float(err[rest].max()), np.argwhere(rest & (err > bound))[:5])
    for i, j, neg in plants:
        v = float(got[i, j])
        v = math.pi - v if neg else v
        print(f"cosine {mode} {geom}: planted {'-1' if neg else '+1'} -> {float(got[i, j])!r}")
        assert math.isfinite(v)
        slack = _ulps(math.pi if neg else a_hi, 4)
        if mode == "fast":
            assert a_hi - slack <= v <= math.acos(float(CLIP_HI) - FAST_DOT) + slack, (i, j, float(got[i, j]))
        else:
            assert abs(v - a_hi) <= slack, (i, j, float(got[i, j]), a_hi)
