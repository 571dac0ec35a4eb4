"""Inputs and numpy restatements for the training input path (tests/test_train_input_cpu.py, tests/test_gpu_train_input.py,
tests/golden/make_goldens_train_input.py): Pillow's 8-bit two-pass resample with the bilinear and bicubic filters,
Philox4x32-10 with the Box-Muller pairing of include/mpreid.h, and the augmentation kernel's pixel rule in float32.
Nothing here touches the GPU or the library."""
import math
import zlib

import numpy as np

RS_BITS = 22

# (name, (in_h, in_w), (out_h, out_w), seed): the shapes of the golden.  1x1 and 3x3 sources (every tap clipped at the border),
# a strong two-axis downscale, same size (identity), an exact 2x upscale, odd sizes both ways, an extreme one-axis downscale
RESIZE_CASES = [("one_px", (1, 1), (4, 4), 1), ("three_px", (3, 3), (16, 8), 2), ("down_600x401", (600, 401), (256, 128), 3),
                ("same_size", (256, 128), (256, 128), 4), ("up_2x", (128, 64), (256, 128), 5), ("odd_down", (97, 53), (32, 32), 6),
                ("mixed", (200, 99), (64, 32), 7), ("wide_strip", (17, 300), (16, 8), 8), ("tiny_down", (5, 7), (3, 2), 9)]
RAGGED_SIZES = [(128, 64), (96, 51), (199, 99), (33, 70), (150, 48)]   # one call, every image its own (h, w)
RAGGED_OUT = (64, 32)
RAGGED_SEED = 40


def make_image(h, w, seed):
    """uint8 [h, w, 3]: noise with planted hard edges (blocks of 0 next to blocks of 255), where the bicubic lobes overshoot"""
    rng = np.random.default_rng([20, int(seed)])
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if h >= 8 and w >= 8:
        img[: h // 3, : w // 2] = 255
        img[: h // 3, w // 2:] = 0
        img[h // 3: h // 2, ::2] = 0
        img[h // 3: h // 2, 1::2] = 255
        img[h - h // 4:, w // 4: w // 2] = np.array([255, 0, 255], np.uint8)
    return img


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ---------------------------------------------------------------- Pillow's resample (src/libImaging/Resample.c)
def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_coeffs(in_size, out_size, filt):
    """per output position (lo, int coefficients): precompute_coeffs + normalize_coeffs_8bpc, in IEEE double"""
    f, base = (_bicubic, 2.0) if filt == "bicubic" else (_bilinear, 1.0)
    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support = base * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        ws = [f((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        ww = 0.0
        for w in ws:
            ww += w
        ks = []
        for w in ws:
            if ww != 0.0:
                w = w / ww
            ks.append(int(-0.5 + w * (1 << RS_BITS)) if w < 0 else int(0.5 + w * (1 << RS_BITS)))
        out.append((lo, np.array(ks, dtype=np.int64)))
    return out


def _pass(img, out_size, filt, axis):
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    for xx, (lo, ks) in enumerate(resample_coeffs(img.shape[0], out_size, filt)):
        acc = (1 << (RS_BITS - 1)) + np.tensordot(ks, img[lo:lo + len(ks)], axes=(0, 0))
        out[xx] = np.clip(acc >> RS_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def np_resize(img, out_hw, filt):
    """PIL.Image.resize((out_w, out_h), BILINEAR | BICUBIC) of a uint8 [h, w, 3] image: horizontal pass into 8 bits, then vertical"""
    return _pass(_pass(np.asarray(img, np.uint8), int(out_hw[1]), filt, 1), int(out_hw[0]), filt, 0)


# ---------------------------------------------------------------- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# Random123's known-answer vectors for philox4x32 with 10 rounds: (counter, key, output)
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
               (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(ctr, key):
    """numpy form: ctr uint32 [..., 4], key (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def philox4x32_10_scalar(ctr, key):
    """a second, independently written form: Python integers, the round written as the paper's S-P network (multiply the two
    even words, swap the halves into place, fold the odd words and the round key in), the key schedule precomputed"""
    keys = [((key[0] + r * W0) & MASK, (key[1] + r * W1) & MASK) for r in range(10)]
    x = [int(v) & MASK for v in ctr]
    for ka, kb in keys:
        prod_a, prod_b = divmod(x[0] * M0, 1 << 32), divmod(x[2] * M1, 1 << 32)   # (high, low)
        x = [prod_b[0] ^ x[1] ^ ka, prod_b[1], prod_a[0] ^ x[3] ^ kb, prod_a[1]]
    return tuple(x)


def erase_words(seed, sample_id, n):
    """the uint32 words of elements 0 .. n-1 of an image's erase box, [n]"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    sid = np.uint64(int(sample_id) & 0xFFFFFFFFFFFFFFFF)
    ctr = np.stack([q & np.uint64(MASK), q >> np.uint64(32), np.full_like(q, sid & np.uint64(MASK)),
                    np.full_like(q, sid >> np.uint64(32))], axis=-1).astype(np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(ctr, (seed & MASK, seed >> 32)).reshape(-1)[: 4 * ((n + 3) // 4)]


def erase_noise_f64(seed, sample_id, eh, ew):
    """float64 [3, eh, ew]: the Box-Muller values of include/mpreid.h from the same Philox words"""
    n = 3 * eh * ew
    w = erase_words(seed, sample_id, n).reshape(-1, 2)
    u1 = ((w[:, 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2.0 * math.pi * u2), r * np.sin(2.0 * math.pi * u2)], axis=-1).reshape(-1)
    return z[:n].reshape(3, eh, ew)


# ---------------------------------------------------------------- the augmentation kernel's rule
def np_augment(img, row, pad, mean, std, seed, sample_id):
    """(float32 [3, H, W] with the box left at 0, bool [H, W] box mask, float64 [3, eh, ew] noise or None) of one resized
    uint8 [H, W, 3] image and its table row"""
    H, W = img.shape[:2]
    flip, top, left, e_top, e_left, eh, ew = (int(v) for v in row[:7])
    src = img[:, ::-1] if flip else img
    padded = np.zeros((H + 2 * pad, W + 2 * pad, 3), np.uint8)
    padded[pad:pad + H, pad:pad + W] = src
    crop = padded[top:top + H, left:left + W]
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    out = ((crop.astype(np.float32) / np.float32(255.0) - m) / s).astype(np.float32).transpose(2, 0, 1).copy()
    mask = np.zeros((H, W), bool)
    noise = None
    if eh > 0:
        mask[e_top:e_top + eh, e_left:e_left + ew] = True
        out[:, mask] = 0.0
        noise = erase_noise_f64(seed, sample_id, eh, ew)
    return out, mask, noise


def row_is_valid(r, H, W, pad):
    """the kernel's validity rules for one table row"""
    return (r[0] in (0, 1) and 0 <= r[1] <= 2 * pad and 0 <= r[2] <= 2 * pad and 0 <= r[5] < H and 0 <= r[6] < W
            and (r[5] == 0) == (r[6] == 0) and 0 <= r[3] <= H - r[5] and 0 <= r[4] <= W - r[6] and r[7] == 0)


# explicit tables at H x W = 16 x 8, B = 6: {flip, crop_top, crop_left, erase_top, erase_left, erase_h, erase_w, 0}
AUG_HW = (16, 8)


def aug_tables(pad):
    H, W = AUG_HW
    p2 = 2 * pad
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    a = [[0, pad, pad, 0, 0, 0, 0, 0],            # no-op: the centre crop of the padded image
         [1, pad, pad, 0, 0, 0, 0, 0],            # flip only
         [0, 0, 0, 0, 0, 0, 0, 0],                # crop at (0, 0)
         [0, p2, p2, 0, 0, 0, 0, 0],              # crop at (2 pad, 2 pad)
         [0, pad, pad, 1, 1, H - 1, W - 1, 0],    # the largest box, at (1, 1)
         [1, p2, 0, 3, 2, 5, 4, 0]]               # a box with flip and crop
    b = [[0, pad, pad, y, x, 1, 1, 0] for y, x in corners] + [[1, 0, p2, 0, 0, H - 1, W - 1, 0], [1, pad, 0, 15, 0, 1, 7, 0]]
    return np.array(a, np.int32), np.array(b, np.int32)


# ---------------------------------------------------------------- the sampler's list
SAMPLER_BATCH, SAMPLER_K, SAMPLER_SEEDS = 8, 4, (0, 1234)


def sampler_list():
    """40 images of 7 identities (labels not contiguous, first appearance not sorted), counts 1 .. 11: below, at and above K"""
    counts = {31: 11, 4: 1, 17: 4, 9: 3, 50: 9, 2: 6, 23: 6}
    rng = np.random.default_rng(77)
    pids = rng.permutation(np.repeat(list(counts), list(counts.values())))
    return [(f"img_{i:03d}.jpg", int(p), int(i % 6), 0) for i, p in enumerate(pids)]


def sampler_len(data, k):
    n = {}
    for item in data:
        n[item[1]] = n.get(item[1], 0) + 1
    return sum(max(c, k) - max(c, k) % k for c in n.values())
