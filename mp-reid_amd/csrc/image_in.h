// image_in.h — the ONE pixel fetch of the encoders' first kernels (the ViT patch gathers of vit.hip, the RN50 stems of rn50.hip
// and rn50_f32.hip), on the image batch of include/mpreid.h as mpreid_check_image_in (common.h) returns it and as the kernels
// take it BY VALUE.  A rounding rule lives here and nowhere else.
//   fp32 input   [B][3][H][W], taken as it is
//   uint8 input  [B][H][W][3] (HWC, what PIL / cv2 hand over after Resize): ToTensor (x / 255) and Normalize ((x - mean) / std)
//                of the reference's val_transforms (datasets/make_dataloader.py:57-61), in fp32, two correctly rounded divisions
//   view         the test-time-augmentation views of processor/processor_uniprompt_stage2.py:605-633, on the normalised values
//                (the reference materialises each view as a new [B,3,H,W] tensor and runs the model on it):
//                0 original   1 torch.flip(img, [3]) (mirror in W)   2 pseudo-IR: img.mean(dim=1) in all 3 channels
//                3 pseudo-RGB: channel 0 in all 3 channels
#pragma once
#include "common.h"

// Which of the two inputs a kernel reads: known at compile time (the throughput kernels have an instance per type), or taken
// from the descriptor (the fp32-mode kernels).
enum ImageSrc { IMAGE_SRC_F32, IMAGE_SRC_U8, IMAGE_SRC_ANY };

// ToTensor (x / 255) then Normalize ((x - mean) / std) of one uint8 value: fp32, two correctly rounded divisions.  THE rounding
// rule of uint8 input, shared by the encoders' pixel fetch below and the training augmentation kernel (train_aug.hip).  A macro,
// not a function: the encoders' first kernels keep the device code they had when the expression stood in image_px_raw itself
// (tools/device_code_diff.py; an inline function moved the stems' instruction schedule).
#define IMAGE_U8_NORM(v, mean, std) __fdiv_rn(__fdiv_rn((float)(v), 255.0f) - (mean), (std))

// the pixel (b, c, y, x) of the batch, before any view
template <ImageSrc SRC = IMAGE_SRC_ANY>
__device__ __forceinline__ float image_px_raw(const mpreid_image_in &in, int b, int c, int y, int x, int H, int W) {
    if (SRC == IMAGE_SRC_U8 || (SRC == IMAGE_SRC_ANY && in.u8_hwc_dev))
        return IMAGE_U8_NORM(in.u8_hwc_dev[(((int64_t)b * H + y) * W + x) * 3 + c], in.mean[c], in.std[c]);
    return in.f32_dev[(((int64_t)b * 3 + c) * H + y) * W + x];
}

// the pixel (b, c, y, x) of view `view` of the batch (in.view itself is not read: the caller passes it, or a constant)
template <ImageSrc SRC = IMAGE_SRC_ANY>
__device__ __forceinline__ float image_px(const mpreid_image_in &in, int view, int b, int c, int y, int x, int H, int W) {
    if (view == 0) return image_px_raw<SRC>(in, b, c, y, x, H, W);
    const int xs = view == 1 ? W - 1 - x : x;
    if (view == 2)   // torch mean over the channel dim: ((c0 + c1) + c2) / 3
        return __fdiv_rn((image_px_raw<SRC>(in, b, 0, y, xs, H, W) + image_px_raw<SRC>(in, b, 1, y, xs, H, W)) +
                             image_px_raw<SRC>(in, b, 2, y, xs, H, W), 3.0f);
    return image_px_raw<SRC>(in, b, view == 3 ? 0 : c, y, xs, H, W);
}
// the same with the view as a template argument: the branches above fold away
template <int VIEW, ImageSrc SRC>
__device__ __forceinline__ float image_px_view(const mpreid_image_in &in, int b, int c, int y, int x, int H, int W) {
    static_assert(VIEW >= 0 && VIEW <= 3, "MPREID_VIEW_*");
    return image_px<SRC>(in, VIEW, b, c, y, x, H, W);
}
