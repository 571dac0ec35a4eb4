"""The fp16 GEMM launcher's plan (csrc/gemm_plan.h: which kernel, which walk, which grid, the verbose line) without a GPU.

plan_gemm is a pure function, so tests/gemm_plan_main.cpp -- a program with its own main, compiled here for the host only, run
as a child and never loaded into Python -- prints the plan's `MPREID_TUNE=verbose=1` line for "epi M N K kseg sym same_operand
has_out cus tune" lines.  The expectations are NOT produced by the code under test:
  * the FORMS table of tests/test_gpu_distance_stores.py and BIG_CASES + FORCED_CASES of tests/test_gpu_rn50_split_layers.py are
    imported: the GPU tests assert those very lines on what launch_one says on the device;
  * the cases no GPU test reaches are worked out below from the launcher's rule, the arithmetic beside each;
  * a second build with -DMPREID_ABLATION prints which timing-ablation instance MPREID_GEMM_DBG selects per epilogue, against a
    table written out from the precedence the launcher documents.
"""
import os
import subprocess

import pytest

import distance_store_cases as S
import test_gpu_distance_stores as D
import test_gpu_rn50_split_layers as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_plan_main.cpp")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(default build, -DMPREID_ABLATION build) of the host program, compiled side by side"""
    out = tmp_path_factory.mktemp("gemm_plan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exes, procs = [], []
    for name, extra in (("gemm_plan_main", []), ("gemm_plan_main_abl", ["-DMPREID_ABLATION"])):
        exes.append(str(out / name))
        procs.append(subprocess.Popen([hipcc, "--offload-arch=gfx950", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall",
                                       "-Wno-unused-function"] + extra + [SRC, "-o", exes[-1]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text
    return exes


def _run(exe, mode, lines):
    r = subprocess.run([exe, mode], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(lines), (len(got), len(lines), r.stdout[-2000:])
    return got


def _line(epi, M, N, K, kseg=0, sym=0, same=0, has_out=1, cus=256, tune="-"):
    return f"{epi} {M} {N} {K} {kseg} {sym} {same} {has_out} {cus} {tune}"


# ---- the stored-distance kernels' five forms: FORMS of the GPU test, at the shapes of its case list --------------------------
@pytest.mark.parametrize("cus", [256, 80])
@pytest.mark.parametrize("tune", list(D.FORMS))
def test_distance_forms_table(programs, tune, cus):
    """the lines test_store_paths_on_a_forced_kernel_form asserts on the device, from the arguments mpreid_distance_f16_fast /
    _split3 hand the launcher: M, N padded to 256; K = d padded to 64, three times that for the 3-term split; sym when one
    tensor is passed twice, and then A == W in the one-pass mode only (the split packs its two operands separately)"""
    pad = lambda n, m: (n + m - 1) // m * m
    lines = []
    for mode in ("fast", "split3"):
        for c in S.CASES:
            same = c.operands == "same"
            K = pad(c.d, 64) * (3 if mode == "split3" else 1)
            lines.append(_line(D.EPI_EUCLID, pad(c.nq, 256), pad(c.ng, 256), K, sym=int(same), same=int(same and mode == "fast"),
                               cus=cus, tune=tune))
    said = sorted(set(_run(programs[0], "plan", lines)))
    p2 = max(8, (2 * cus) & ~7)
    want = sorted(f"gemm epi {D.EPI_EUCLID}: " + form.format(p2=p2) for form in D.FORMS[tune])
    assert said == want, (tune, said, want)


# ---- the split RN50 1x1 layers on the persistent kernel: kernel, walk name, tiles and grid of the GPU test's cases ------------
def test_rn50_split_layer_cases(programs):
    """test_split_layer_persistent_kernel_and_walks_ran's lines at 256 CUs, from conv_split's arguments (csrc/rn50_f32.hip:
    M = Mp, N = npad, K = 2 kseg): BIG_CASES on the default dispatch, FORCED_CASES under gemm_big=2"""
    cus = 256
    lines, want = [], []
    for c in R.BIG_CASES + R.FORCED_CASES:
        npad, kseg = (c.cout + 127) // 128 * 128, (c.cin + 63) // 64 * 64
        epi = R.EPI_OF[c.form]
        lines.append(_line(epi, c.Mp, npad, 2 * kseg, kseg=kseg, cus=cus, tune="-" if c in R.BIG_CASES else "gemm_big=2"))
        tm, tn = c.Mp // 256, npad // 256
        want.append(f"gemm epi {epi}: persistent 256x256, walk {c.walk}, {tm}x{tn} tiles, grid {min(tm * tn, cus)}")
    assert _run(programs[0], "plan", lines) == want
    # and the same shapes with gemm_big=0 (the digests' reference child): the 128x128 kernel, one workgroup per tile
    lines = [ln.rsplit(" ", 1)[0] + " gemm_big=0" for ln in lines]
    want = [f"gemm epi {R.EPI_OF[c.form]}: 128x128, {c.Mp // 128}x{(c.cout + 127) // 128} tiles, grid {c.Mp // 128 * ((c.cout + 127) // 128)}"
            for c in R.BIG_CASES + R.FORCED_CASES]
    assert _run(programs[0], "plan", lines) == want


# ---- what no GPU test reaches, from the launcher's rule ----------------------------------------------------------------------
# The rule (csrc/gemm_plan.h, unchanged from launch_one's): persistent when M % 256 == N % 256 == 0 and tiles >= 128 (gemm_big=1);
# walk = column-fastest (1) only for tiles_n <= 4 and 2 K >= 8192; |= 8 when tiles_m % 64 != 0 and tiles_m % 32 == 0; |= 16 with
# gemm_ragged=0; grid = min(tiles, CUs).  Walk name: GR = 4 with bit 8 else 8; groups = ceil(tiles_m / GR);
# owned = grid % 8 == 0 and (tiles_m % (8 GR) == 0 or (groups >= 24 and not bit 16 and not sym)), "ragged-" when tiles_m % (8 GR) != 0;
# else blocked = grid % 64 == 0 and tiles >= grid; else strided.
HAND_CASES = [
    # tiles_m = 224: 224 % 64 = 32, 224 % 32 = 0 -> walk 8, GR = 4; 224 x 1 = 224 tiles < 256 CUs -> grid 224 = 8 * 28; 224 % 32 == 0 -> owned
    (_line(0, 224 * 256, 256, 64), "gemm epi 0: persistent 256x256, walk owned GR=4 row-fastest, 224x1 tiles, grid 224"),
    # ... x 2 tile columns: 448 tiles -> grid 256
    (_line(0, 224 * 256, 512, 64), "gemm epi 0: persistent 256x256, walk owned GR=4 row-fastest, 224x2 tiles, grid 256"),
    # ... 2 K = 8192 and tiles_n = 2 <= 4: column-fastest
    (_line(0, 224 * 256, 512, 4096), "gemm epi 0: persistent 256x256, walk owned GR=4 column-fastest, 224x2 tiles, grid 256"),
    # gemm_walk=3: groups of 4 by the switch (walk 3, no bit 8): GR = 4, 224 % 32 == 0 -> owned
    (_line(0, 224 * 256, 512, 64, tune="gemm_walk=3"), "gemm epi 0: persistent 256x256, walk owned GR=4 row-fastest, 224x2 tiles, grid 256"),
    # 127 tiles of 256x256: below the threshold -> 128x128, 254 x 2 = 508 tiles
    (_line(0, 127 * 256, 256, 64), "gemm epi 0: 128x128, 254x2 tiles, grid 508"),
    # 128 tiles: at the threshold; 128 % 64 == 0 -> walk 0, GR = 8, grid 128 = 8 * 16, 128 % 64 == 0 -> owned
    (_line(0, 128 * 256, 256, 64), "gemm epi 0: persistent 256x256, walk owned GR=8 row-fastest, 128x1 tiles, grid 128"),
    # 64 x 2 = 128 tiles as well, but N % 256 != 0 never takes it: 128 x 3 tiles of 128 columns
    (_line(0, 64 * 256, 384, 64), "gemm epi 0: 128x128, 128x3 tiles, grid 384"),
    # gemm_ragged=0 on the ragged-owned shape of BIG_CASES (185 x 2 tiles, 24 groups of 8): bit 16 -> not owned; grid 256 = 4 * 64
    # and 370 tiles >= 256 -> blocked
    (_line(11, 185 * 256, 512, 128, kseg=64, tune="gemm_ragged=0"), "gemm epi 11: persistent 256x256, walk blocked, 185x2 tiles, grid 256"),
    # 130 x 1 tiles (strided on 256 CUs in BIG_CASES).  128 CUs, fewer than the tiles: grid 128 = 2 * 64, 17 groups < 24 -> blocked
    (_line(10, 130 * 256, 256, 128, kseg=64, cus=128), "gemm epi 10: persistent 256x256, walk blocked, 130x1 tiles, grid 128"),
    # 304 CUs, more than the tiles: grid 130, no multiple of 8 -> strided
    (_line(10, 130 * 256, 256, 128, kseg=64, cus=304), "gemm epi 10: persistent 256x256, walk strided, 130x1 tiles, grid 130"),
    # gemm_grid=64 on 256 CUs: 64 workgroups, 130 tiles >= 64 -> blocked; gemm_grid above the CU count changes nothing
    (_line(10, 130 * 256, 256, 128, kseg=64, tune="gemm_grid=64"), "gemm epi 10: persistent 256x256, walk blocked, 130x1 tiles, grid 64"),
    (_line(10, 130 * 256, 256, 128, kseg=64, tune="gemm_grid=300"), "gemm epi 10: persistent 256x256, walk strided, 130x1 tiles, grid 130"),
    # the candidate epilogue always takes the persistent kernel, even 2 x 2 tiles with gemm_big=0; grid 4 -> strided
    (_line(9, 512, 512, 64, sym=1, same=1, has_out=0, tune="gemm_big=0"), "gemm epi 9: persistent 256x256, walk strided, 2x2 tiles, grid 4"),
    # ... 64 x 64 tiles, symmetric: grid 256, 64 % 64 == 0 -> owned (exact division: allowed for a symmetric problem)
    (_line(9, 16384, 16384, 64, sym=1, same=1, has_out=0), "gemm epi 9: persistent 256x256, walk owned GR=8 row-fastest, 64x64 tiles, grid 256"),
    # ... 65 x 65 tiles, symmetric: 9 groups -> not owned; grid 256, 4225 tiles -> blocked, the symmetric problem's compacted list
    (_line(9, 16640, 16640, 64, sym=1, same=1, has_out=0), "gemm epi 9: persistent 256x256, walk blocked compacted, 65x65 tiles, grid 256"),
    # the cosine epilogue has no persistent instance
    (_line(6, 128 * 256, 256, 64, tune="gemm_big=2"), "gemm epi 6: 128x128, 256x2 tiles, grid 512"),
    # stored distances, one tensor twice, default switches: two workgroups per CU from 16 tile rows of 256 (16 x 32 tiles of 256x128) ...
    (_line(5, 4096, 4096, 64, sym=1, same=1), "gemm epi 5: two workgroups per CU 256x128 (symmetric), 16x32 tiles, grid 512"),
    # ... the 3-term split's operands (A != W) stay on the persistent kernel's symmetric instance: 16 x 16 = 256 tiles, 16 % 64 != 0,
    # 2 groups -> not owned; grid 256 -> blocked compacted
    (_line(5, 4096, 4096, 192, sym=1, same=0), "gemm epi 5: persistent 256x256 (symmetric), walk blocked compacted, 16x16 tiles, grid 256"),
    # ... 15 tile rows: 225 tiles >= 128 -> persistent, symmetric instance; grid 225, no multiple of 8 -> strided
    (_line(5, 3840, 3840, 64, sym=1, same=1), "gemm epi 5: persistent 256x256 (symmetric), walk strided, 15x15 tiles, grid 225"),
    # dist_p2_full=1: two tensors from 16 x 32 tiles of 256x128; N = 31 * 128 is neither that nor a multiple of 256 -> 128x128
    (_line(5, 4096, 4096, 64, tune="dist_p2_full=1"), "gemm epi 5: two workgroups per CU 256x128 (two tensors), 16x32 tiles, grid 512"),
    (_line(5, 4096, 3968, 64, tune="dist_p2_full=1"), "gemm epi 5: 128x128, 32x31 tiles, grid 992"),
    # ... and only with an output to store
    (_line(5, 4096, 4096, 64, has_out=0, tune="dist_p2_full=1"), "gemm epi 5: persistent 256x256, walk blocked, 16x16 tiles, grid 256"),
    # dist_sym_p2_grid: that kernel's grid by the switch
    (_line(5, 4096, 4096, 64, sym=1, same=1, tune="dist_sym_p2_grid=96"), "gemm epi 5: two workgroups per CU 256x128 (symmetric), 16x32 tiles, grid 96"),
    # the two shape checks that live in the plan
    (_line(10, 256, 256, 192, kseg=64), "ERROR gemm_f16: split epilogue 10 needs K == 2 * kseg, kseg a multiple of 64 (K=192 kseg=64)"),
    (_line(12, 256, 256, 64, kseg=32), "ERROR gemm_f16: split epilogue 12 needs K == 2 * kseg, kseg a multiple of 64 (K=64 kseg=32)"),
    (_line(9, 384, 512, 64, sym=1, same=1, has_out=0), "ERROR gemm_f16: the candidate epilogue needs M, N multiples of 256"),
]


def test_hand_worked_cases(programs):
    got = _run(programs[0], "plan", [ln for ln, _ in HAND_CASES])
    bad = [(ln, g, w) for (ln, w), g in zip(HAND_CASES, got) if g != w]
    assert not bad, bad


def test_ablation_build_plans_the_same(programs):
    """-DMPREID_ABLATION changes which instance runs, never the plan"""
    lines = [ln for ln, _ in HAND_CASES]
    assert _run(programs[1], "plan", lines) == [w for _, w in HAND_CASES]


# ---- timing-ablation instances (MPREID_ABLATION builds) ----------------------------------------------------------------------
# MPREID_GEMM_DBG -> the DBG instance of gemm_f16_big_kernel, in the launcher's order of precedence:
#   1. 64 on the split epilogues (10 .. 15)
#   2. 32 on every epilogue with a persistent instance other than GE_EUCLID (5) / GE_BIAS_GELU (3), with the stamps buffer
#   3. GE_BIAS_F16 (1): 1 2 3 4 5 7 8 9 15 16 24
#   4. GE_EUCLID / GE_BIAS_GELU: 800 and 32 with the stamps buffer, F * 128 for F = 1 .. 6, 16
#   anything else, and every epilogue without a persistent instance (GE_COSINE, 6): the plain instance
PLAIN, STAMPS = 0, 1
DBG_TABLE = {
    0: {32: STAMPS}, 2: {32: STAMPS}, 4: {32: STAMPS}, 7: {32: STAMPS}, 8: {32: STAMPS}, 9: {32: STAMPS},
    1: {32: STAMPS, 1: PLAIN, 2: PLAIN, 3: PLAIN, 4: PLAIN, 5: PLAIN, 7: PLAIN, 8: PLAIN, 9: PLAIN, 15: PLAIN, 16: PLAIN, 24: PLAIN},
    3: {800: STAMPS, 32: STAMPS, 128: PLAIN, 256: PLAIN, 384: PLAIN, 512: PLAIN, 640: PLAIN, 768: PLAIN, 16: PLAIN},
    5: {800: STAMPS, 32: STAMPS, 128: PLAIN, 256: PLAIN, 384: PLAIN, 512: PLAIN, 640: PLAIN, 768: PLAIN, 16: PLAIN},
    6: {},
    10: {64: PLAIN, 32: STAMPS}, 11: {64: PLAIN, 32: STAMPS}, 12: {64: PLAIN, 32: STAMPS}, 13: {64: PLAIN, 32: STAMPS},
    14: {64: PLAIN, 32: STAMPS}, 15: {64: PLAIN, 32: STAMPS},
    -1: {v: PLAIN for v in (1, 2, 3, 4, 8, 9, 16, 24, 32, 33)},      # dist_sym_p2_kernel<abl>, MPREID_TUNE=dist_sym_p2_abl
}
DBG_VALUES = sorted(set(range(-1, 40)) | {63, 64, 65, 96, 127, 128, 129, 192, 256, 384, 512, 640, 768, 769, 800, 801, 896, 1024})


def test_ablation_instances(programs):
    assert sorted(DBG_TABLE) == list(range(-1, 16))
    pairs = [(epi, dbg) for epi in sorted(DBG_TABLE) for dbg in DBG_VALUES]
    got = _run(programs[1], "dbg", [f"{e} {d}" for e, d in pairs])
    want = [f"{e} {d} {d if d in DBG_TABLE[e] else 0} {DBG_TABLE[e].get(d, 0)}" for e, d in pairs]
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad[:10]
    # 29 + 19 + 10: the instances of a default build's persistent kernel that no shipped path could launch, the ones an
    # ablation build had on top of them, and dist_sym_p2_kernel's
    assert sum(len(v) for v in DBG_TABLE.values()) == 58
