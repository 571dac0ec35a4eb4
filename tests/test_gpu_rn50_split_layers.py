"""One convolution of the split-precision RN50 tower (mpreid_rn50_conv_split_layer: the tower's own layer routine behind a
C entry point) against float64, in every operand / output form the tower uses, at the smallest shapes at which each
mechanism can fail.  Two data sets per shape:

EXACT  activations p * (1 + q 2^-12) and folded weights r * (1 + s 2^-12) with p, q, r, s in {-1, 0, 1}, integer biases and
       destinations.  An fp16 pair of such a value is hi = +-1, lo = +-2^-12, so the three products the kernels run
       (hi.hi', lo.hi', hi.lo') are multiples of 2^-12 and never above 1: every partial sum, in ANY order, is exact in fp32
       while the sum of the |terms| stays below 2^24 grid steps -- asserted on the host for the data of each case, not
       assumed.  The reference -- those three products (and NOT lo.lo') summed in float64 from the pair operands the device
       holds, * oscale + bias, then the ReLU / += / max(dst, 0) + of the form -- must be met bit for bit; a mismatch is
       reported at its (image, y, x, channel).
       (A value with p = 0 but q != 0 is the pair hi = q 2^-12, lo = 0: its product with a weight's lo' is a multiple of
       2^-24 only, the sums would need 36 bits and the precondition could not hold.  So q = 0 where p = 0 and s = 0 where
       r = 0: zeros stay in the data -- padding must still multiply to nothing -- but there are no lone small values.)
RANDOM randn activations, weights randn * sqrt(2 / (taps * cin)) under a jittered folded BatchNorm; reference: F.conv2d +
       BatchNorm (+ residual, ReLU) in float64 on the fp32 inputs; bounds: the split GEMM's own (test_gpu_vit.py,
       test_split_gemm_kernels_agree_bitwise_and_are_fp32_grade, derived for k <= 3072; here taps * cin <= 1152): relative
       L2 <= 6e-7, max |d| <= 4e-6 * max(1, max |ref|); a pair output is compared as hi + lo with the representation's own
       allowance on top of max |d| (test_split_pack_is_exact_pair): 2^-22 |ref| + 2^-25 per element.

Every call is made twice, into buffers pre-filled with NaN and with large finite values: every element the header documents
as written (rows < M; all npad fp32 columns -- the one 64-wide tile for a 3x3 convolution with cout <= 64 -- and all
2 * pair_c pair columns) must not depend on what was there, and nothing behind a pair output is written.

The 1x1 path has TWO kernels (csrc/gemm_f16.hip, launch_one): CASES reach the 128x128 one only; the persistent 256x256 one --
separate epilogues: the residual forms' LDS-DMA prefetch of the destination waited for with counted vmcnt, the pair form's
column mask and ring-aliased patches -- takes every conv3, downsample and most conv1 of a production batch.  So "the smallest
shapes at which each mechanism can fail" holds for that kernel as well:
BIG_CASES     the production dispatch (>= 128 tiles of 256x256) at kseg = 64 / 128 / 512, i.e. 6- / 12- / 144-stage pipelines, in
              every tile walk of the kernel (on 256 CUs): owned 128x1 and 64x2 tiles, ragged-owned 185x2, strided 185x1 (fewer
              tiles than CUs, a grid that is no multiple of 8) and 130x1, blocked 132x2; both data sets, every call three
              times with the same bits; rows [M, Mp) of a residual destination as the header states them
FORCED_CASES  the padded forms (cout < npad, pair_c < npad, M < Mp, ld_in > cin), which production never hands that kernel:
              MPREID_TUNE=gemm_big=2 in a child process
and for all of them the RANDOM outputs carry the bits of the 128x128 kernel (a child with gemm_big=0: the same image gives the
same bits in any batch), and the launcher itself says (MPREID_TUNE=verbose=1) that the persistent kernel and the named walk
ran."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STEP = 2.0 ** -12


class Case:
    def __init__(self, name, taps, B, H, W, cin, cout, form="f32", pair_c=0, relu_in=False, ld_in=None, scales=None, live_rows=0,
                 walk=None, tail_rows=False):
        self.name, self.taps, self.B, self.H, self.W, self.cin, self.cout = name, taps, B, H, W, cin, cout
        self.form, self.pair_c, self.relu_in, self.ld_in, self.scales = form, pair_c, relu_in, ld_in or cin, scales
        # live_rows > cout: the weight and bias rows [cout, live_rows) hold VALUES instead of the documented zeros, so the
        # zeros of the pair columns [cout, pair_c) must come from the epilogue's own column mask
        self.live_rows = live_rows
        # the persistent kernel's cases: the tile walk the shape is meant to land in on a 256-CU device (the library names the one
        # it took, test_split_layer_persistent_kernel_and_walks_ran); tail_rows: rows [M, Mp) of a residual destination hold data
        # too, and what the call leaves there is checked against the header's statement
        self.walk, self.tail_rows = walk, tail_rows
        self.M = B * H * W
        self.Mp = (self.M + 255) // 256 * 256
        # fp32 columns a call writes (include/mpreid.h): all npad, but one 64-wide tile for a 3x3 with cout <= 64
        self.ncols = 64 if taps == 9 and cout <= 64 else (cout + 127) // 128 * 128

    def __repr__(self):
        return self.name


# forms: f32 (fp32 out), pair (ReLU-ed pairs, no fp32 tensor), res1 (+=), res2 (max(dst, 0) +), res_pair (+= and the pair copy)
CASES = [
    # ---- 3x3 (conv_f16.hip, pair form) ----
    # M = 35 < one tile, every border kind, cin < kseg, the 64-wide tile variant, cout < npad
    Case("3x3_5x7_c8_n24", 9, 1, 5, 7, 8, 24),
    Case("3x3_5x7_c8_n24_relu", 9, 1, 5, 7, 8, 24, relu_in=True),
    # one column: left / right taps are always padding; two 64-channel blocks per tap (the second mostly zero padding); two
    # N tiles (the second mostly masked)
    Case("3x3_3x1_c72_n136", 9, 3, 3, 1, 72, 136),
    Case("3x3_3x1_c72_n136_relu", 9, 3, 3, 1, 72, 136, relu_in=True),
    Case("3x3_1x9_c64_n64", 9, 2, 1, 9, 64, 64),                     # a single row
    # M = 384: three M tiles, image boundaries inside a tile, an image straddling two tiles; RANDOM: neighbouring images of
    # very different magnitudes
    Case("3x3_16x8_c64_n128_b3", 9, 3, 16, 8, 64, 128, scales=(1.0, 256.0, 16.0)),
    Case("3x3_16x8_c64_n64_pairs", 9, 2, 16, 8, 64, 64, form="pair", pair_c=64, relu_in=True),   # production layer1's conv2 -> conv3
    Case("3x3_8x8_c128_n16_pairs", 9, 4, 8, 8, 128, 16, form="pair", pair_c=64),   # columns [16, 64) of both halves exactly zero
    Case("3x3_8x8_c128_n16_pairs_live_rows", 9, 4, 8, 8, 128, 16, form="pair", pair_c=64, live_rows=64),   # ... by the mask itself
    # ---- 1x1 (gemm_f16.hip, GE_S_*) ----
    Case("1x1_m35_c16_ld128_n64", 1, 1, 5, 7, 16, 64, ld_in=128),       # channels [16, 128) hold NaN: never read; Mp = 256
    Case("1x1_m256_c64_n16_pairs", 1, 1, 16, 16, 64, 16, form="pair", pair_c=64, relu_in=True),   # GE_S_BIAS_RELU_PAIR
    Case("1x1_m512_c256_n128_res1", 1, 2, 16, 16, 256, 128, form="res1", relu_in=True),
    Case("1x1_m512_c256_n128_res2", 1, 2, 16, 16, 256, 128, form="res2", relu_in=True),
    Case("1x1_m512_c256_n128_res_pair", 1, 2, 16, 16, 256, 128, form="res_pair", pair_c=128, relu_in=True),
]


# ---- 1x1 on the PERSISTENT 256x256 kernel (gemm_f16_big_kernel), in the launcher's production dispatch ----
# launch_one (csrc/gemm_f16.hip; its plan: csrc/gemm_plan.h) takes that kernel when Mp % 256 == 0, npad % 256 == 0 and there are at least 128 tiles of
# 256x256; its grid is min(tiles, CU count).  kseg = 64 / 128 give the 6- and 12-stage pipelines of RN50's layer1 / layer2.
# `walk`: what the kernel's rule gives on 256 CUs (owned: the grid is a multiple of 8 and the tile rows divide into 8 XCDs x
# groups of 8, or -- ragged -- there are at least 24 groups; blocked: a full grid of a multiple of 64 workgroups; else strided).
OWNED, RAGGED, STRIDED, BLOCKED = "owned GR=8 row-fastest", "ragged-owned GR=8 row-fastest", "strided", "blocked"
BIG_CASES = [
    # 128 x 1 tiles (layer1 conv3 / downsample): every epilogue behind a 6-stage pipeline
    Case("big_m32768_c64_n256_f32", 1, 8, 1, 4096, 64, 256, walk=OWNED),
    Case("big_m32768_c64_n256_pairs", 1, 8, 1, 4096, 64, 256, form="pair", pair_c=256, walk=OWNED),
    Case("big_m32768_c64_n256_res1", 1, 8, 1, 4096, 64, 256, form="res1", walk=OWNED),
    Case("big_m32768_c64_n256_res2", 1, 8, 1, 4096, 64, 256, form="res2", walk=OWNED),
    Case("big_m32768_c64_n256_res_pair", 1, 8, 1, 4096, 64, 256, form="res_pair", pair_c=256, walk=OWNED),
    # 64 x 2 tiles (layer2 conv3): two tile columns
    Case("big_m16384_c128_n512_res_pair", 1, 8, 1, 2048, 128, 512, form="res_pair", pair_c=512, walk=OWNED),
    Case("big_m16384_c128_n512_pairs", 1, 8, 1, 2048, 128, 512, form="pair", pair_c=512, walk=OWNED),
    # 185 tile rows, M = 47323 = 37 x 1279 < Mp = 47360: rows [M, Mp) written as documented.  185 x 1 tiles are fewer than the
    # 256 CUs: the grid is 185 workgroups, no multiple of 8 -- the STRIDED walk.  185 x 2 tiles fill the chip: 23 groups of 8
    # tile rows and a last group of one, the ragged owned walk
    Case("big_m47323_c64_n256_res2", 1, 37, 1, 1279, 64, 256, form="res2", walk=STRIDED, tail_rows=True),
    Case("big_m47323_c64_n512_res2", 1, 37, 1, 1279, 64, 512, form="res2", walk=RAGGED, tail_rows=True),
    Case("big_m33280_c64_n256_res_pair", 1, 8, 1, 4160, 64, 256, form="res_pair", pair_c=256, walk=STRIDED),   # 130 x 1 tiles
    # 132 x 2 = 264 tiles on 256 CUs, 17 groups: blocked, with unused slots in the edge blocks
    Case("big_m33792_c64_n512_res1", 1, 8, 1, 4224, 64, 512, form="res1", walk=BLOCKED),
    Case("big_m33792_c64_n512_pairs", 1, 8, 1, 4224, 64, 512, form="pair", pair_c=512, walk=BLOCKED),
    # layer3 block-1 conv1: 48 k-blocks, 144 stages
    Case("big_m32768_c512_n256_pairs_relu", 1, 8, 1, 4096, 512, 256, form="pair", pair_c=256, relu_in=True, walk=OWNED),
]
# ---- the padded forms the entry point documents, which production never hands the persistent kernel: forced onto it with
# MPREID_TUNE=gemm_big=2 in a child process (every shape here is below 128 tiles: the strided walk) ----
FORCED_CASES = [
    Case("forced_m35_c16_ld128_n200_f32", 1, 1, 5, 7, 16, 200, ld_in=128, walk=STRIDED),      # one tile; channels [16, 128) NaN
    # wave column 3 of the tile (columns [192, 256)) masked; columns [136, 192) exactly zero in both halves
    Case("forced_m512_c64_n136_pairs192", 1, 2, 1, 256, 64, 136, form="pair", pair_c=192, relu_in=True, walk=STRIDED),
    Case("forced_m512_c64_n136_pairs256", 1, 2, 1, 256, 64, 136, form="pair", pair_c=256, relu_in=True, walk=STRIDED),
    Case("forced_m768_c256_n256_res1", 1, 3, 1, 256, 256, 256, form="res1", walk=STRIDED),     # 3 tile rows
    Case("forced_m768_c256_n256_res2", 1, 3, 1, 256, 256, 256, form="res2", walk=STRIDED),
    Case("forced_m768_c256_n256_res_pair", 1, 3, 1, 256, 256, 256, form="res_pair", pair_c=256, walk=STRIDED),
    Case("forced_m512_c128_n512_res_pair", 1, 2, 1, 256, 128, 512, form="res_pair", pair_c=512, walk=STRIDED),   # two tile columns
]
EPI_OF = {"f32": 10, "pair": 14, "res1": 11, "res2": 11, "res_pair": 15}      # GemmEpi (csrc/gemm_f16.h)


def _pairs_np(v):
    """fp32 array -> (hi, lo) fp16 arrays: hi = fp16(v), lo = fp16(v - hi), round to nearest even (include/mpreid.h)"""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def _where(c, row, col):
    b, r = divmod(int(row), c.H * c.W)
    return f"image {b} y {r // c.W} x {r % c.W} channel {int(col)}"


def _assert_same(c, what, got, want):
    """bit for bit: the raw bit patterns are compared (-0.0 is not +0.0), and nothing may be NaN or infinite; the first
    element that differs is reported"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in (np.float16, np.float32), (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    bad = ~np.isfinite(got) | (got.view(bits) != want.view(bits))
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise AssertionError(f"{c.name} {what}: {int(bad.sum())} of {bad.size} elements differ, first at row {r} = "
                             f"{_where(c, r, col)}: got {float(got[r, col])!r}, want {float(want[r, col])!r}")


def _make(c, exact, with_ref=True):
    """host data of a case: x [M][ld_in] fp32 (channels >= cin NaN), folded weights [cout][cin][k][k] + bias in float64, the
    initial destination [Mp][npad] for the residual forms, and for RANDOM the float64 reference of the layer's output (None
    with with_ref=False: the same operands for a caller that only compares bits)"""
    rng = np.random.default_rng(sum(map(ord, c.name)) * 2 + int(exact))
    k = 3 if c.taps == 9 else 1
    npad = (c.cout + 127) // 128 * 128
    cg = max(c.cout, c.live_rows)     # weight / bias rows generated
    x = np.full((c.M, c.ld_in), np.nan, np.float32)
    if exact:
        p = rng.integers(-1, 2, (c.M, c.cin))
        q = rng.integers(-1, 2, (c.M, c.cin))
        x[:, :c.cin] = (p * (1.0 + q * STEP)).astype(np.float32)
        r = rng.integers(-1, 2, (cg, c.cin, k, k))
        s = rng.integers(-1, 2, (cg, c.cin, k, k))
        w = r * (1.0 + s * STEP)
        bias = rng.integers(-3, 4, cg).astype(np.float64)
        bias[c.cout:] = np.abs(bias[c.cout:]) + 1      # (live rows: a positive bias survives the ReLU)
        dst = rng.integers(-4, 5, (c.Mp, npad)).astype(np.float32)
        return x, w, bias, dst, None
    xr = rng.standard_normal((c.M, c.cin))
    if c.scales:
        xr *= np.repeat(np.asarray(c.scales), c.H * c.W)[:, None]
    x[:, :c.cin] = xr.astype(np.float32)
    w = (rng.standard_normal((cg, c.cin, k, k)) * np.sqrt(2.0 / (c.taps * c.cin))).astype(np.float32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(cg)).astype(np.float32), (0.1 * rng.standard_normal(cg)).astype(np.float32)
    mean, var = (0.1 * rng.standard_normal(cg)).astype(np.float32), (0.5 + rng.random(cg)).astype(np.float32)
    dst = rng.standard_normal((c.Mp, npad)).astype(np.float32)
    # folded in float64 as Rn50Encoder does (mpreid/ops.py: fold)
    sc = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)
    wf, bf = w.astype(np.float64) * sc[:, None, None, None], beta.astype(np.float64) - mean.astype(np.float64) * sc
    if not with_ref:
        return x, wf, bf, dst, None
    # the float64 reference on the fp32 inputs: conv + BatchNorm (eval), then the form's residual / ReLU
    xin = torch.from_numpy(x[:, :c.cin].astype(np.float64)).reshape(c.B, c.H, c.W, c.cin).permute(0, 3, 1, 2)
    if c.relu_in:
        xin = F.relu(xin)
    y = F.conv2d(xin, torch.from_numpy(w.astype(np.float64)), None, padding=k // 2)
    y = F.batch_norm(y, torch.from_numpy(mean.astype(np.float64)), torch.from_numpy(var.astype(np.float64)),
                     torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), training=False, eps=1e-5)
    ref = y.permute(0, 2, 3, 1).reshape(c.M, cg).numpy()[:, :c.cout]
    return x, wf, bf, dst, ref


def _conv_of(c, w, bias, dev):
    """the weights the way the product builds them (mpreid.ops.pairs_of / pairs_of_3x3) -> (struct, tensors to keep,
    W_hi, W_lo float64 [npad][taps][kseg] read back from the device: the scaled pair operand the kernels multiply)"""
    from mpreid import ops
    if c.taps == 9:
        conv, keep = ops.pairs_of_3x3(w, bias, dev)
        slab = keep[0].cpu().numpy().astype(np.float64).reshape(conv.npad, 9, conv.kseg // 64, 2, 64)
        whi, wlo = slab[:, :, :, 0].reshape(conv.npad, 9, conv.kseg), slab[:, :, :, 1].reshape(conv.npad, 9, conv.kseg)
    else:
        conv, keep = ops.pairs_of(w.reshape(w.shape[0], c.cin), bias, c.cin, 1, dev)
        pair = keep[0].cpu().numpy().astype(np.float64)
        whi, wlo = pair[:, None, :conv.kseg], pair[:, None, conv.kseg:]
    assert conv.kseg == (c.cin + 63) // 64 * 64 and conv.npad == (c.cout + 127) // 128 * 128 and conv.taps == c.taps
    assert conv.cout == max(c.cout, c.live_rows)
    conv.cout = c.cout
    return conv, keep, whi, wlo


def _conv64(c, a, wt):
    """sum over (tap, channel) of a[pixel + tap][channel] * wt[n][tap][channel] in float64: a [M][kseg], wt [npad][taps][kseg]
    -> [M][npad]"""
    kseg = a.shape[1]
    if c.taps == 1:
        return a @ wt[:, 0, :].T
    xin = torch.from_numpy(np.ascontiguousarray(a)).reshape(c.B, c.H, c.W, kseg).permute(0, 3, 1, 2)
    w4 = torch.from_numpy(np.ascontiguousarray(wt)).reshape(-1, 3, 3, kseg).permute(0, 3, 1, 2)
    return F.conv2d(xin, w4, None, padding=1).permute(0, 2, 3, 1).reshape(c.M, -1).numpy()


def _host_pairs(c, x, kseg):
    """the pair operand pack_pairs_kernel must produce: [Mp][hi(kseg) | lo(kseg)], ReLU on read, zeros past cin and past M"""
    v = x[:, :c.cin]
    if c.relu_in:
        v = np.where(v < 0, np.float32(0), v)
    hi, lo = _pairs_np(v)
    full = np.zeros((c.Mp, 2 * kseg), np.float16)
    full[:c.M, :c.cin], full[:c.M, kseg:kseg + c.cin] = hi, lo
    return full


def _garbage(shape, dtype, which, dev):
    """0: NaN, 1: large finite values (different in every element)"""
    n = int(np.prod(shape))
    if which == 0:
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)
    big = 3.0e4 if dtype == torch.float16 else 1.0e30
    return (torch.linspace(0.5, 1.0, n, device=dev, dtype=torch.float32) * big).to(dtype).reshape(shape)


GUARD = 4096      # fp16 elements behind a pair output: a store past 2 * pair_c columns of the last rows would land there


def _run(c, conv, x_dev, dst, dev, which, in_pairs=None, form=None):
    """one call into garbage-filled buffers -> (fp32 out [Mp][npad] or None, pairs [Mp][2 pair_c] or None, pair scratch)"""
    from mpreid import ops
    form = form or c.form
    res = {"f32": 0, "pair": 0, "res1": 1, "res2": 2, "res_pair": 1}[form]
    pair_c = c.pair_c if form in ("pair", "res_pair") else 0
    out = None
    if form != "pair":
        out = _garbage((c.Mp, conv.npad), torch.float32, which, dev)
        if res:
            rows = c.Mp if c.tail_rows else c.M      # (tail_rows: the padding rows of the destination hold data as well)
            out[:rows] = torch.from_numpy(dst[:rows]).to(dev)
    pout = flat = None
    if pair_c:      # the pair output ends where its buffer ends: the elements behind it must come back untouched
        flat = _garbage((c.Mp * 2 * pair_c + GUARD,), torch.float16, which, dev)
        pout, guard = flat[:c.Mp * 2 * pair_c].view(c.Mp, 2 * pair_c), flat[c.Mp * 2 * pair_c:].clone()
    scratch = _garbage((c.Mp, 2 * conv.kseg), torch.float16, which, dev) if in_pairs is None else None
    out, pout = ops.conv_split_layer(conv, c.B, c.H, c.W, x=x_dev if in_pairs is None else None, relu_in=c.relu_in, in_pairs=in_pairs,
                                     res=res, out=out, pair_c=pair_c, pair_out=pout, scratch=scratch)
    torch.cuda.synchronize()
    if pair_c:
        assert torch.equal(flat[c.Mp * 2 * pair_c:].view(torch.int16), guard.view(torch.int16)), (c.name, "written past the pair output")
    return (None if out is None else out.cpu().numpy(), None if pout is None else pout.cpu().numpy(),
            None if scratch is None else scratch.cpu().numpy())


def _run_twice(c, conv, x_dev, dst, dev, reps=2, **kw):
    """NaN-filled and large-value-filled buffers: every element documented as written agrees between the two calls (reps = 3:
    and a third call, value-filled again -- the persistent kernel's determinism screen)"""
    a = _run(c, conv, x_dev, dst, dev, 0, **kw)
    for rep in range(1, reps):
        b = _run(c, conv, x_dev, dst, dev, 1, **kw)
        tag = f"(NaN-filled vs value-filled buffers, call {rep + 1})" if reps > 2 else "(NaN-filled vs value-filled buffers)"
        if a[0] is not None:
            _assert_same(c, "fp32 out " + tag, a[0][:c.M, :c.ncols], b[0][:c.M, :c.ncols])
        if a[1] is not None:
            _assert_same(c, "pair out " + tag, a[1][:c.M], b[1][:c.M])
        if a[2] is not None:   # the pack writes all Mp rows of the scratch operand
            _assert_same(c, "pair scratch " + tag, a[2], b[2])
    return a


def _tail_rows_want(c, conv, dst, bias):
    """rows [M, Mp) of a residual destination after the call (include/mpreid.h): y of the zero operand rows is the bias, so
    res 2 leaves max(dst, 0) + bias and res 1 dst + bias there -- one fp32 addition, as in the epilogue"""
    bp = np.zeros(conv.npad, np.float32)
    bp[:c.cout] = bias[:c.cout]          # (the bias as the device holds it: mpreid.ops.pairs_of)
    d = dst[c.M:]
    if c.form == "res2":
        d = np.where(d < 0, np.float32(0), d)
    return d + bp[None, :]


def _check_exact(c, dev, reps=2):
    """the EXACT set of one case -> (fp32 out, pair out)"""
    x, w, bias, dst, _ = _make(c, True)
    conv, keep, whi, wlo = _conv_of(c, w, bias, dev)
    ahl = _host_pairs(c, x, conv.kseg)
    ahi, alo = ahl[:c.M, :conv.kseg].astype(np.float64), ahl[:c.M, conv.kseg:].astype(np.float64)
    # ---- the precondition of exactness, checked on this case's own operands ----
    # activations: hi an integer, lo a multiple of 2^-12; weights (scaled by 2^e = 1 / oscale): hi' a multiple of 2^e, lo' of
    # 2^(e-12): every product hi.hi', lo.hi', hi.lo' is a multiple of g = 2^(e-12) ...
    assert (alo != 0).any() and (wlo != 0).any()       # (the lo halves are in play)
    scale = 1.0 / conv.oscale
    assert scale == 2.0 ** round(np.log2(scale))
    g = scale * STEP
    assert (ahi == np.round(ahi)).all() and (alo / STEP == np.round(alo / STEP)).all()
    assert (whi / scale == np.round(whi / scale)).all() and (wlo / g == np.round(wlo / g)).all()
    # ... and for every output the sum of the |terms| is below 2^24 such steps: no partial sum in any order needs more than
    # the 24 bits of an fp32 accumulator
    tot = _conv64(c, np.abs(ahi) + np.abs(alo), np.abs(whi)) + _conv64(c, np.abs(ahi), np.abs(wlo))
    assert tot.max() / g < 2.0 ** 24, tot.max() / g
    assert c.taps * c.cin <= 4096
    # ---- the reference: hi.hi' + lo.hi' + hi.lo' (no lo.lo') in float64, * oscale + bias, then the form ----
    acc = _conv64(c, ahi + alo, whi) + _conv64(c, ahi, wlo)
    bias_pad = np.zeros(conv.npad)
    bias_pad[:c.cout] = bias[:c.cout]
    if c.live_rows:
        acc[:, c.cout:] = 0.0      # columns >= cout are not outputs: zero whatever the rows there hold
    y = acc * conv.oscale + bias_pad
    if c.form in ("res1", "res_pair"):
        y = dst[:c.M].astype(np.float64) + y
    elif c.form == "res2":
        assert (dst[:c.M] < 0).any()
        y = np.maximum(dst[:c.M].astype(np.float64), 0.0) + y
    assert (y.astype(np.float32).astype(np.float64) == y).all()     # (the epilogue's fma and sum are exact as well)
    y = y.astype(np.float32)
    x_dev = torch.from_numpy(x).to(dev)
    out, pout, scratch = _run_twice(c, conv, x_dev, dst, dev, reps)
    # the pack (ReLU on read, channels >= cin and rows >= M zero; the NaN in the unused input channels is never read)
    _assert_same(c, "pair operand written by the pack", scratch, ahl)
    if out is not None:
        _assert_same(c, "fp32 out", out[:c.M, :c.ncols], y[:, :c.ncols])
    if c.tail_rows:
        assert c.Mp > c.M and (dst[c.M:] < 0).any()
        _assert_same(c, "fp32 out, rows [M, Mp)", out[c.M:], _tail_rows_want(c, conv, dst, bias))
    if pout is not None:
        v = np.maximum(y[:, :c.pair_c], np.float32(0))
        hi, lo = _pairs_np(v)
        assert c.cout == c.pair_c or (not hi[:, c.cout:].any() and not lo[:, c.cout:].any())   # columns [cout, pair_c): zero
        assert (lo != 0).any()
        _assert_same(c, "pair out", pout[:c.M], np.concatenate([hi, lo], axis=1))
    if c.form == "res_pair":   # the fp32 result of the fused form == the plain residual call's
        plain = _run(c, conv, x_dev, dst, dev, 1, form="res1")[0]
        _assert_same(c, "fp32 out of the residual + pair form vs the plain residual form", out[:c.M], plain[:c.M])
    del keep
    return out, pout


def _check_random(c, dev, reps=2):
    """the RANDOM set of one case -> (fp32 out, pair out)"""
    x, w, bias, dst, ref = _make(c, False)
    conv, keep, _, _ = _conv_of(c, w, bias, dev)
    if c.form in ("res1", "res_pair"):
        ref = dst[:c.M, :c.cout].astype(np.float64) + ref
    elif c.form == "res2":
        assert (dst[:c.M] < 0).any()
        ref = np.maximum(dst[:c.M, :c.cout].astype(np.float64), 0.0) + ref
    x_dev = torch.from_numpy(x).to(dev)
    out, pout, scratch = _run_twice(c, conv, x_dev, dst, dev, reps)
    _assert_same(c, "pair operand written by the pack", scratch, _host_pairs(c, x, conv.kseg))

    def grade(what, got, want, pair):
        d = np.abs(got - want)
        allow = (2.0 ** -22 * np.abs(want) + 2.0 ** -25) if pair else np.zeros_like(want)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        bound = 4e-6 * max(1.0, float(np.abs(want).max()))
        print(f"split layer {c.name} {what}: rel-L2 vs float64 {rel:.2e} (bound 6e-7), max |d| {d.max():.2e} "
              f"(bound {bound:.2e}{' + pair allowance' if pair else ''}), max |ref| {np.abs(want).max():.3g}", flush=True)
        assert np.isfinite(got).all()
        assert rel <= 6e-7, (what, rel)
        over = d - allow - bound
        assert over.max() <= 0, (what, _where(c, *np.unravel_index(np.argmax(over), over.shape)), float(d.max()), bound)

    if out is not None:
        got = out[:c.M].astype(np.float64)
        grade("fp32 out", got[:, :c.cout], ref, False)
        if c.scales:   # image by image: a large neighbour must not hide what bleeds into a small image, nor the reverse
            hw = c.H * c.W
            for b in range(c.B):
                grade(f"fp32 out, image {b} (x {c.scales[b]:g})", got[b * hw:(b + 1) * hw, :c.cout], ref[b * hw:(b + 1) * hw], False)
        if c.form == "f32":   # columns [cout, npad): zero weight rows and zero bias
            assert not out[:c.M, c.cout:c.ncols].any()
    if c.tail_rows:
        assert c.Mp > c.M and (dst[c.M:] < 0).any()
        _assert_same(c, "fp32 out, rows [M, Mp)", out[c.M:], _tail_rows_want(c, conv, dst, bias))
    if pout is not None:
        want = np.maximum(ref, 0.0)
        hi, lo = pout[:c.M, :c.pair_c].astype(np.float64), pout[:c.M, c.pair_c:].astype(np.float64)
        grade("pair out (hi + lo)", (hi + lo)[:, :c.cout], want, True)
        assert not hi[:, c.cout:].any() and not lo[:, c.cout:].any()
        # a well-formed pair: hi is the fp16 rounding of the value the pair stands for, lo the fp16 rounding of the rest
        if out is not None:
            eh, el = _pairs_np(np.maximum(out[:c.M, :c.pair_c], np.float32(0)))
            _assert_same(c, "pair copy of relu(fp32 out)", pout[:c.M], np.concatenate([eh, el], axis=1))
    if c.form == "res_pair":
        plain = _run(c, conv, x_dev, dst, dev, 1, form="res1")[0]
        _assert_same(c, "fp32 out of the residual + pair form vs the plain residual form", out[:c.M], plain[:c.M])
    del keep
    return out, pout


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_split_layer_exact_set_is_bit_exact(c):
    from mpreid import _lib
    _check_exact(c, _lib.require_gpu())


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_split_layer_random_set_is_fp32_grade(c):
    from mpreid import _lib
    _check_random(c, _lib.require_gpu())


@pytest.mark.parametrize("name", ["3x3_5x7_c8_n24_relu", "3x3_16x8_c64_n64_pairs", "1x1_m35_c16_ld128_n64", "1x1_m512_c256_n128_res2"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_split_layer_prepacked_operand_gives_the_same_bits(name, exact):
    """the operand delivered as pairs by the caller (what a producer's pair epilogue writes: `prepacked` for 1x1, `act_pairs`
    for 3x3) == the operand packed inside the call, bit for bit"""
    from mpreid import _lib
    c = next(k for k in CASES if k.name == name)
    dev = _lib.require_gpu()
    x, w, bias, dst, _ = _make(c, exact)
    conv, keep, _, _ = _conv_of(c, w, bias, dev)
    x_dev = torch.from_numpy(x).to(dev)
    out, pout, scratch = _run_twice(c, conv, x_dev, dst, dev)
    pairs = torch.from_numpy(scratch).to(dev)
    out2, pout2, _ = _run_twice(c, conv, None, dst, dev, in_pairs=pairs)
    for what, u, v in (("fp32 out", out, out2), ("pair out", pout, pout2)):
        assert (u is None) == (v is None)
        if u is not None:
            n = c.ncols if what == "fp32 out" else u.shape[1]
            _assert_same(c, what + " (operand packed inside the call vs delivered as pairs)", v[:c.M, :n], u[:c.M, :n])
    del keep


def test_split_layer_argument_checks():
    """conv_split's / the implicit GEMM's argument checks come back as MPREID_ERR_ARG (a RuntimeError here); those on the pair output's shape before any kernel is launched"""
    from mpreid import _lib, ops
    dev = _lib.require_gpu()
    c = CASES[0]
    x, w, bias, dst, _ = _make(c, True)
    conv3, keep3, _, _ = _conv_of(c, w, bias, dev)
    c1 = next(k for k in CASES if k.name == "1x1_m256_c64_n16_pairs")
    x1, w1, b1, _, _ = _make(c1, True)
    conv1, keep1, _, _ = _conv_of(c1, w1, b1, dev)
    xd, x1d = torch.from_numpy(x).to(dev), torch.from_numpy(x1).to(dev)
    bad = [
        lambda: ops.conv_split_layer(conv3, c.B, c.H, c.W, x=xd, res=1, out=torch.zeros((c.Mp, conv3.npad), device=dev)),   # 3x3 + residual
        lambda: ops.conv_split_layer(conv3, c.B, c.H, c.W, x=xd, pair_c=96),                       # pair_c % 64
        lambda: ops.conv_split_layer(conv3, c.B, c.H, c.W, x=xd, pair_c=128),                      # columns no tile covers
        lambda: ops.conv_split_layer(conv1, c1.B, c1.H, c1.W, x=x1d, pair_c=256),                  # pair_c > npad
        lambda: ops.conv_split_layer(conv1, c1.B, c1.H, c1.W, x=x1d, res=1, pair_c=64,             # res + pairs: pair_c == npad
                                     out=torch.zeros((c1.Mp, conv1.npad), device=dev)),
        lambda: ops.conv_split_layer(conv1, c1.B, c1.H, c1.W, x=x1d[:, :32].contiguous()),         # ld_in < cin
        lambda: ops.conv_split_layer(conv1, c1.B, c1.H, c1.W, x=x1d, res=3, out=torch.zeros((c1.Mp, conv1.npad), device=dev)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError, match="bad argument"):
            f()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()
    del keep3, keep1


# ---- the persistent 256x256 kernel -----------------------------------------------------------------------------------------
def _assert_production_dispatch_takes_the_big_kernel(c):
    """plan_gemm (csrc/gemm_plan.h, launch_one's plan): use_big = M % 256 == 0 && N % 256 == 0 && (M / 256) * (N / 256) >= 128, with gemm_big at
    its default -- M = Mp, N = npad here (conv_split, csrc/rn50_f32.hip)"""
    npad = (c.cout + 127) // 128 * 128
    assert "gemm_big" not in os.environ.get("MPREID_TUNE", ""), "these cases test the default dispatch"
    assert c.taps == 1 and c.Mp % 256 == 0 and npad % 256 == 0 and (c.Mp // 256) * (npad // 256) >= 128, c.name


def _digests(c, out, pout):
    """[(what, [sha-256 (first 8 hex digits) of each block of 256 rows below M])]: all fp32 columns, all pair columns"""
    res = []
    for what, t in (("fp32", out), ("pairs", pout)):
        if t is not None:
            t = np.ascontiguousarray(t[:c.M])
            res.append((what, [hashlib.sha256(t[r:r + 256].tobytes()).hexdigest()[:8] for r in range(0, c.M, 256)]))
    return res


def _worker(mode, names):
    """the body of a child process (the tuning string is latched per process), one line "OK <case>" per finished case:
    check   EXACT and RANDOM of every named case, each call three times; DIGEST lines of the RANDOM outputs
    digest  the RANDOM operands through one call; DIGEST lines
    probe   one call on zero operands (for the launcher's MPREID_TUNE=verbose=1 lines)"""
    import ctypes as C
    from mpreid import _lib
    dev = _lib.require_gpu()
    cus = C.c_int(0)
    _lib.check(_lib.load().mpreid_device_info(None, 0, C.byref(cus), None), "mpreid_device_info")
    print("CUS", cus.value, flush=True)
    for c in BIG_CASES + FORCED_CASES:
        if c.name not in names:
            continue
        if mode == "check":
            _check_exact(c, dev, 3)
            out, pout = _check_random(c, dev, 3)
        else:
            x, w, bias, dst, _ = _make(c, False, with_ref=False)
            if mode == "probe":
                x, w, bias, dst = np.zeros_like(x[:, :c.cin]), np.zeros_like(w), np.zeros_like(bias), np.zeros_like(dst)
                c = Case(c.name, 1, c.B, c.H, c.W, c.cin, c.cout, form=c.form, pair_c=c.pair_c)
            conv, keep, _, _ = _conv_of(c, w, bias, dev)
            out, pout, _ = _run(c, conv, torch.from_numpy(x).to(dev), dst, dev, 1)
            del keep
        if mode != "probe":
            for what, d in _digests(c, out, pout):
                print("DIGEST", c.name, what, ",".join(d), flush=True)
        print("OK", c.name, flush=True)


WORKER = """
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, "mp-reid_amd"), os.path.join({root!r}, "tests")]
import test_gpu_rn50_split_layers as T
T._worker(sys.argv[1], sys.argv[2:])
"""


def _child(tmp, tune, mode, cases):
    """-> (the child's stdout lines, its stderr); the child has run every case to its OK line"""
    script = tmp / "split_layer_worker.py"
    script.write_text(WORKER.format(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    env = dict(os.environ)
    env.pop("MPREID_TUNE", None)
    if tune:
        env["MPREID_TUNE"] = tune
    r = subprocess.run([sys.executable, str(script), mode] + [c.name for c in cases], env=env, capture_output=True, text=True, timeout=900)
    lines = r.stdout.splitlines()
    done = [ln.split()[1] for ln in lines if ln.startswith("OK ")]
    assert r.returncode == 0 and done == [c.name for c in cases], (tune, mode, done, r.stdout[-1500:], r.stderr[-3000:])
    return lines, r.stderr


def _digest_table(lines):
    return {(ln.split()[1], ln.split()[2]): ln.split()[3].split(",") for ln in lines if ln.startswith("DIGEST ")}


@pytest.fixture(scope="module")
def small_kernel_digests(tmp_path_factory):
    """the RANDOM outputs of every persistent-kernel case from the 128x128 kernel (MPREID_TUNE=gemm_big=0), computed once"""
    lines, _ = _child(tmp_path_factory.mktemp("small_kernel"), "gemm_big=0", "digest", BIG_CASES + FORCED_CASES)
    return _digest_table(lines)


@pytest.fixture(scope="module")
def forced_child(tmp_path_factory):
    """the padded forms on the persistent kernel, all in ONE child (gemm_big=2: whenever the shape is divisible; verbose=1: the
    launcher names what it launches)"""
    return _child(tmp_path_factory.mktemp("forced"), "gemm_big=2,verbose=1", "check", FORCED_CASES)


def _assert_same_digests(c, got, small):
    """the project's invariant -- the same image gives the same bits in any batch, so through either kernel: every block of
    256 rows of the persistent kernel's output has the digest of the 128x128 kernel's"""
    assert got, c.name
    for what, d in got:
        want = small[(c.name, what)]
        bad = [i for i in range(max(len(d), len(want))) if i >= len(d) or i >= len(want) or d[i] != want[i]]
        assert not bad, f"{c.name} {what}: {len(bad)} of {len(want)} blocks of 256 rows differ from the 128x128 kernel's, first tile row {bad[0]}"


@pytest.mark.parametrize("c", BIG_CASES, ids=repr)
def test_split_layer_persistent_exact_set_is_bit_exact(c):
    """EXACT on the persistent kernel in its production dispatch; every call three times with the same bits (the residual
    epilogues wait for their LDS-DMA prefetch with counted vmcnt: a wrong count is a race)"""
    from mpreid import _lib
    _assert_production_dispatch_takes_the_big_kernel(c)
    _check_exact(c, _lib.require_gpu(), 3)


@pytest.mark.parametrize("c", BIG_CASES, ids=repr)
def test_split_layer_persistent_random_set_is_fp32_grade_and_the_small_kernels_bits(c, small_kernel_digests):
    """RANDOM on the persistent kernel: the module's bounds against float64, three calls with the same bits, and the bits of
    the 128x128 kernel"""
    from mpreid import _lib
    _assert_production_dispatch_takes_the_big_kernel(c)
    out, pout = _check_random(c, _lib.require_gpu(), 3)
    _assert_same_digests(c, _digests(c, out, pout), small_kernel_digests)


@pytest.mark.parametrize("c", FORCED_CASES, ids=repr)
def test_split_layer_forced_persistent_padded_forms(c, forced_child, small_kernel_digests):
    """cout < npad, pair_c < npad, M < Mp, ld_in > cin on the persistent kernel: EXACT and RANDOM passed in the child, and its
    RANDOM outputs have the 128x128 kernel's bits"""
    lines, _ = forced_child
    print("\n".join(ln for ln in lines if ln.startswith(f"split layer {c.name} ")))      # (the child's RANDOM figures)
    assert "OK " + c.name in lines
    table = _digest_table(lines)
    _assert_same_digests(c, [(what, d) for (name, what), d in table.items() if name == c.name], small_kernel_digests)


def test_split_layer_persistent_kernel_and_walks_ran(tmp_path, forced_child):
    """MPREID_TUNE=verbose=1: launch_one names kernel, walk, tiles and grid of each distinct launch on stderr.  Every shape of
    BIG_CASES (a child on the default dispatch, one call each on zero operands) and of FORCED_CASES reached the persistent
    kernel, in the walk its case names (the walks depend on the grid: asserted on a 256-CU device)"""
    lines, err = _child(tmp_path, "verbose=1", "probe", BIG_CASES)
    cus = int([ln for ln in lines if ln.startswith("CUS ")][0].split()[1])
    said = [ln for ln in (err + "\n" + forced_child[1]).splitlines() if ln.startswith("[mpreid] gemm epi")]
    print("\n".join(said))
    if cus != 256:
        print(f"the device has {cus} CUs, not 256: the walk names are not asserted, only that the persistent kernel ran")
    for c in BIG_CASES + FORCED_CASES:
        tm, tn = c.Mp // 256, (c.cout + 127) // 128 * 128 // 256
        head, tiles = f"[mpreid] gemm epi {EPI_OF[c.form]}: persistent 256x256, walk ", f", {tm}x{tn} tiles, grid {min(tm * tn, cus)}"
        hits = [ln for ln in said if ln.startswith(head) and ln.endswith(tiles)]
        assert len(hits) == 1, (c.name, head, tiles, said)
        if cus == 256:
            assert hits[0] == head + c.walk + tiles, (c.name, hits[0], c.walk)
    assert not [ln for ln in said if "persistent" not in ln], said      # no GEMM of these children ran another kernel
    if cus == 256:
        assert {c.walk for c in BIG_CASES} == {OWNED, RAGGED, STRIDED, BLOCKED}
