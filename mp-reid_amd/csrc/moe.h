// moe.h — internal seams of csrc/moe.hip (mixture-of-experts MLP of the image tower), used by vit.hip's forward.
// The public entry points and the semantics are in include/mpreid.h ("MoE image encoder").
#pragma once
#include "common.h"

constexpr int MOE_BM = 128;   // row tile of the grouped GEMM: every expert's slot segment is padded to it

// Where the pieces of one routed-MLP workspace live (bytes from its 256-byte aligned base); a pure function of the sizes.
struct MoeLayout {
    int64_t rows;
    int W, E, K;
    int tiles_max, nblk;
    int64_t slots_max;
    size_t meta, tile_tab, blk_cnt, slot_row, tok_slot, tok_w, hidden, y, total;
};
MoeLayout moe_layout(int64_t rows, int W, int E, int K);

// MPREID_OK, or MPREID_ERR_UNSUPPORTED with the error text set (1 <= K <= min(E, 8), E <= 64, width % 128 == 0, width <= 1024,
// rows <= MPREID_MOE_MAX_ROWS = 2^20 whatever K is)
int moe_check_shape(int64_t rows, int W, int E, int K);
// MPREID_OK, or MPREID_ERR_ARG for a NULL or misaligned pointer of one MoE block (the gate is not looked at)
int moe_check_layer(const mpreid_moe_layer *ly);

// sel / w of every row from the fp32 residual stream (ln_g == ln_b == nullptr: x already holds h); no argument checks
int moe_route_launch(const float *x, int64_t rows, int W, const float *ln_g, const float *ln_b, const float *gate, int E, int K,
                     int32_t *sel, float *w, float *logits, hipStream_t stream);
// counts, scan, slot and tile tables in `ws` (laid out by moe_layout); once per forward
int moe_dispatch_launch(const int32_t *sel, const float *w, const MoeLayout &m, void *ws, hipStream_t stream);
// grouped FC1 (QuickGELU, fp16 pairs) -> grouped FC2 (fp32) -> combine into x, with the tables moe_dispatch_launch left in ws
int moe_mlp_launch(const _Float16 *a_pairs, const MoeLayout &m, const mpreid_moe_layer *ly, float *x, void *ws,
                   hipStream_t stream);
