// attention.h — the boundary of csrc/attention.hip: one dispatcher per attention form, and the work figure of their profile
// records.  qkv [B*L][3W] (q | k | v column blocks, head h = columns [64h, 64h + 64)); L up to MPREID_VIT_MAX_TOKENS
// (the causal form: MPREID_TEXT_MAX_TOKENS).  q_tiles: 0 = every query row, n > 0 = the first n 16-query tiles only.
#pragma once
#include "common.h"

// fp16 q | k | v -> fp16 out [B*L][W]
int attention_dispatch(const _Float16 *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles, hipStream_t stream);
// split precision: fp32 q | k | v -> fp16 pairs out [B*L][hi(W) | lo(W)]
int attention_split_dispatch(const float *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles, hipStream_t stream);
// the same with the causal mask of the text tower, every row
int attention_causal_dispatch(const float *qkv, int B, int L, int W, int heads, _Float16 *out, hipStream_t stream);
// all fp32: fp32 q | k | v -> fp32 out [B*L][W]
int attention_f32_dispatch(const float *qkv, int B, int L, int W, int heads, float *out, hipStream_t stream);

// the work figure of every attention profile record, algorithmic bytes: k, v of every token + q and the output of the query rows
double attention_bytes(int64_t M, int64_t qrows, int W, int pr);
