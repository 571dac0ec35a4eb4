// train_aug.hip — the random part of the reference's train_transforms (datasets/make_dataloader_uniprompt.py:55-60) behind the
// bicubic Resize of preprocess.hip, in ONE kernel on the resized uint8 batch:
//   RandomHorizontalFlip -> Pad(pad) -> RandomCrop(H x W) -> ToTensor -> Normalize -> timm RandomErasing(mode='pixel', max_count=1)
// The random DECISIONS (flip, crop corner, erase box) are taken on the host in the reference's order of draws
// (mpreid.ops.TrainAugment.draw) and arrive as an int32 [B][8] table; the kernel is a pure function of (image, row, seed,
// sample id).  The table travels BY VALUE in the kernel arguments, MPREID_AUG_IMAGES_PER_LAUNCH images per launch, as the
// descriptors of mpreid_optim_step_multi_f32 do (optim.hip): no upload, no workspace, nothing to keep alive after the call.
//
// HBM-bound byte work: 3 bytes read and 12 written per output pixel.  One thread per output pixel (y, x): it reads the three
// bytes of its HWC source pixel and writes one fp32 to each of the three planes, so a wave writes 256 contiguous bytes per plane.
// The noise of the erase box is Philox4x32-10 (Salmon et al., SC'11; the published multipliers and Weyl constants) keyed by the
// call's seed and counted by (element index in the box >> 2, sample id): an element's value does not depend on the batch it
// sits in.  include/mpreid.h states the definition; tests/train_input_cases.py restates it in numpy.
#include "common.h"
#include "image_in.h"

namespace {

constexpr int AUG_MAX_B = MPREID_AUG_IMAGES_PER_LAUNCH;

struct AugTable {
    int32_t p[AUG_MAX_B][8];      // {flip, crop_top, crop_left, erase_top, erase_left, erase_h, erase_w, 0}
    int64_t sample_id[AUG_MAX_B];
};
static_assert(sizeof(AugTable) <= 3072, "the table is a kernel argument");

struct AugNorm {
    float mean[3], std[3];
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// element e of the (3, erase_h, erase_w) box of the image with this sample id: one value of a Box-Muller pair
__device__ __forceinline__ float erase_noise(uint64_t e, uint64_t sample_id, uint32_t k0, uint32_t k1) {
    const uint64_t q = e >> 2;
    uint32_t w[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)sample_id, (uint32_t)(sample_id >> 32), k0, k1, w);
    const int pair = (int)(e & 2);
    const float u1 = (float)((w[pair] >> 8) + 1u) * 0x1p-24f;   // (0, 1]: at most 2^24, exact
    const float u2 = (float)(w[pair + 1] >> 8) * 0x1p-24f;      // [0, 1)
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);                               // the angle 2 pi u2 with an exact argument
    return r * ((e & 1) ? s : c);
}

__global__ __launch_bounds__(256) void train_augment_kernel(const unsigned char *__restrict__ img, const AugTable t, int H, int W,
                                                            int pad, uint32_t k0, uint32_t k1, const AugNorm nm,
                                                            float *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t hw = (int64_t)H * W;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= hw) return;
    const int y = (int)(gid / W), x = (int)(gid % W);
    const int flip = t.p[b][0], top = t.p[b][1], left = t.p[b][2];
    const int e_top = t.p[b][3], e_left = t.p[b][4], e_h = t.p[b][5], e_w = t.p[b][6];
    float *o = out + (int64_t)b * 3 * hw + gid;
    if (e_h > 0 && y >= e_top && y < e_top + e_h && x >= e_left && x < e_left + e_w) {
        const uint64_t sid = (uint64_t)t.sample_id[b];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint64_t e = ((uint64_t)c * e_h + (uint64_t)(y - e_top)) * e_w + (uint64_t)(x - e_left);
            o[c * hw] = erase_noise(e, sid, k0, k1);
        }
        return;
    }
    const int sy = y + top - pad, sx = x + left - pad;
    unsigned char v[3] = {0, 0, 0};                              // Pad(pad, fill=0)
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
        const unsigned char *p = img + (((int64_t)b * H + sy) * W + (flip ? W - 1 - sx : sx)) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * hw] = IMAGE_U8_NORM(v[c], nm.mean[c], nm.std[c]);
}

// one row of the caller's table: 0, or MPREID_ERR_ARG with the image and the field named
int check_row(const int32_t *r, int b, int H, int W, int pad) {
#define AUG_FIELD(cond, name, idx, why)                                                                     \
    if (!(cond)) {                                                                                           \
        mpreid_set_error("bad argument: params[%d].%s = %d: %s (H %d, W %d, pad %d)", b, name, (int)r[idx], why, H, W, pad); \
        return MPREID_ERR_ARG;                                                                               \
    }
    AUG_FIELD(r[0] == 0 || r[0] == 1, "flip", 0, "must be 0 or 1");
    AUG_FIELD(r[1] >= 0 && r[1] <= 2 * pad, "crop_top", 1, "must lie in 0 .. 2 pad");
    AUG_FIELD(r[2] >= 0 && r[2] <= 2 * pad, "crop_left", 2, "must lie in 0 .. 2 pad");
    AUG_FIELD(r[5] >= 0 && r[5] < H, "erase_h", 5, "must lie in 0 .. H - 1");
    AUG_FIELD(r[6] >= 0 && r[6] < W, "erase_w", 6, "must lie in 0 .. W - 1");
    AUG_FIELD((r[5] == 0) == (r[6] == 0), "erase_w", 6, "erase_h and erase_w are both zero (no erasing) or both positive");
    AUG_FIELD(r[3] >= 0 && r[3] <= H - r[5], "erase_top", 3, "the erase box must lie inside the image");
    AUG_FIELD(r[4] >= 0 && r[4] <= W - r[6], "erase_left", 4, "the erase box must lie inside the image");
    AUG_FIELD(r[7] == 0, "reserved", 7, "the last field must be 0");
#undef AUG_FIELD
    return MPREID_OK;
}

} // namespace

extern "C" int mpreid_train_augment_f32(const uint8_t *img, int batch, int H, int W, int pad, const int32_t *params,
                                        const int64_t *sample_id, uint64_t seed, const float *mean, const float *std,
                                        float *out, mpreid_stream_t stream_) {
    ARG_CHECK(img && params && sample_id && mean && std && out);
    ARG_CHECK(batch > 0 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30));
    ARG_CHECK(pad >= 0 && pad <= (1 << 20));
    AugNorm nm;
    for (int c = 0; c < 3; ++c) {
        if (!(std[c] != 0.0f) || !(std[c] - std[c] == 0.0f) || !(mean[c] - mean[c] == 0.0f)) {
            mpreid_set_error("bad argument: mean[%d] = %g, std[%d] = %g: finite, std not 0", c, (double)mean[c], c, (double)std[c]);
            return MPREID_ERR_ARG;
        }
        nm.mean[c] = mean[c];
        nm.std[c] = std[c];
    }
    for (int b = 0; b < batch; ++b) {   // the whole table before the first launch
        const int rc = check_row(params + (size_t)b * 8, b, H, W, pad);
        if (rc != MPREID_OK) return rc;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t hw = (int64_t)H * W;
    const unsigned gx = (unsigned)((hw + 255) / 256);
    for (int b0 = 0; b0 < batch; b0 += AUG_MAX_B) {
        const int nb = batch - b0 < AUG_MAX_B ? batch - b0 : AUG_MAX_B;
        AugTable t = {};
        for (int i = 0; i < nb; ++i) {
            for (int j = 0; j < 8; ++j) t.p[i][j] = params[(size_t)(b0 + i) * 8 + j];
            t.sample_id[i] = sample_id[b0 + i];
        }
        hipLaunchKernelGGL(train_augment_kernel, dim3(gx, nb), dim3(256), 0, stream, img + (size_t)b0 * hw * 3, t, H, W, pad,
                           (uint32_t)seed, (uint32_t)(seed >> 32), nm, out + (size_t)b0 * hw * 3);
        LAUNCH_CHECK();
    }
    return 0;
}
