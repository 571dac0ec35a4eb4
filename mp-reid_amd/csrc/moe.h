// moe.h — internal seams of csrc/moe.hip (mixture-of-experts MLP of the image tower), used by vit.hip's forward.
// The public entry points and the semantics are in include/mpreid.h ("MoE image encoder").
#pragma once
#include "common.h"

constexpr int MOE_BM = 128;   // row tile of the grouped GEMM: every expert's slot segment is padded to it
constexpr int MOE_META_COUNTS = 128;   // ints from MoeLayout::meta: [e] = rows whose sel holds expert e, left by the dispatch

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
// the two grouped GEMMs of moe_mlp_launch without the combine: hidden and y[slot] in ws.  u_out != nullptr: FC1 runs a second
// time through the fp32 epilogue and leaves the pre-activation u[slot][4W] there (the gradient's recompute)
int moe_experts_launch(const _Float16 *a_pairs, const MoeLayout &m, const mpreid_moe_layer *ly, void *ws, float *u_out,
                       hipStream_t stream);

// ---- csrc/moe_grad.hip: the gradient through one routed MLP and the router's gradient -------------------------------------
// The gradient workspace: the forward's layout first (tables, hidden, y), then u / du [slots][4W] fp32, the per-slot routing
// weight, and the router gradient's tables (per-1024-row expert counts, their sums, per-256-row pieces of sum_r p[r][e]).
struct MoeGradLayout {
    MoeLayout fwd;
    int npieces;
    size_t u, slot_w, cnt_blk, cnt, piece_p, total;
};
MoeGradLayout moe_grad_layout(int64_t rows, int W, int E, int K);
// bytes mpreid_moe_route_backward needs (its tables alone, laid out from the workspace's base)
size_t moe_route_grad_bytes(int64_t rows, int E);
// d_a[row] = sum over the row's experts, ascending e, of du_slot . Wfc_e (written), d_w[row][k] = <dy_row, y_slot> (written or
// added); either may be nullptr.  Needs the tables of moe_dispatch_launch in ws; runs moe_experts_launch itself.
int moe_mlp_backward_launch(const _Float16 *a_pairs, const int32_t *sel, const MoeGradLayout &m, const mpreid_moe_layer *ly,
                            const mpreid_moe_layer_t *lt, const float *dy, float *d_a, float *d_w, bool accumulate_d_w, void *ws,
                            hipStream_t stream);
// d_logits [rows][E] and l_aux [1] (either may be nullptr) from the routing and d_w (nullptr: zeros), with the tables laid out
// from `ws` (moe_route_grad_bytes of it, 256-byte aligned).  dispatch_cnt: the per-expert row counts moe_dispatch_launch left
// on the device (meta + MOE_META_COUNTS) for this sel; nullptr (a caller without a dispatch): counted from sel here
int moe_route_backward_ws(const float *logits, const int32_t *sel, const float *w, const float *d_w, int64_t rows, int E, int K,
                          float aux_coef, float *d_logits, float *l_aux, const int *dispatch_cnt, void *ws, hipStream_t stream);
// aux_coef is neither NaN nor infinite; lives in moe_grad.hip, which is compiled with strict IEEE semantics
bool moe_coef_is_finite(float aux_coef);
// t[row][:] += sum_e d_logits[row][e] * gate[e][:], e ascending in one fmaf chain per element
int moe_gate_dh_launch(const float *d_logits, const float *gate, int64_t rows, int W, int E, float *t, hipStream_t stream);
// moe_route_backward_ws with the three tables given one by one
int moe_route_backward_launch(const float *logits, const int32_t *sel, const float *w, const float *d_w, int64_t rows, int E, int K,
                              float aux_coef, float *d_logits, float *l_aux, const int *dispatch_cnt, int *cnt_blk, int *cnt,
                              float *piece_p, hipStream_t stream);
