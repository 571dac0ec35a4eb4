// text.hip — the forward of CLIP's text tower for gfx950 (mpreid_text_forward; model/clip/model.py:609-619 after the embedding
// lookup, model/make_model_uniprompt.py:58-68): the residual blocks of the split mode (the block driver of vit.hip: tower_block,
// towers.h) with a CAUSAL attention (attention_causal_kernel, attention.hip), ln_final on the end-of-text row and
// text_projection (tower_head, vit.hip).  Split precision only: the text side is never the throughput path.
#include "towers.h"

int text_check_shape(int tokens, int width, int heads) {
    if (check_width_heads(width, heads) != SHAPE_OK) {
        mpreid_set_error("text tower: head dim must be 64 and the width a multiple of 128 up to 1024 (width %d, heads %d)", width, heads);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (tokens < 2 || tokens > MPREID_TEXT_MAX_TOKENS) {
        mpreid_set_error("text tower: %d tokens outside 2 .. %d (MPREID_TEXT_MAX_TOKENS: K / V of a head stay in LDS)", tokens,
                         MPREID_TEXT_MAX_TOKENS);
        return MPREID_ERR_UNSUPPORTED;
    }
    return MPREID_OK;
}

// x[m][:] = prompts[m][:] + pos[m % L][:]   (model/make_model_uniprompt.py:59)
__global__ __launch_bounds__(256) void text_add_pos_kernel(const float *__restrict__ prompts, const float *__restrict__ pos,
                                                           int64_t M, int L, int W, float *__restrict__ x) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one float4 each
    const int w4 = W / 4;
    if (gid >= M * w4) return;
    const int64_t m = gid / w4;
    const int k = (int)(gid - m * w4) * 4;
    const float4 a = *reinterpret_cast<const float4 *>(prompts + m * W + k);
    const float4 p = *reinterpret_cast<const float4 *>(pos + (int64_t)(m % L) * W + k);
    *reinterpret_cast<float4 *>(x + m * W + k) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

TextLayout text_layout(const mpreid_text_cfg *c, int B) {
    TextLayout v{};
    v.M = (int64_t)B * c->tokens;
    v.Mpad = (int64_t)align_up((size_t)v.M, 256);   // 256-row tiles of the big GEMM kernel
    WsCursor take;
    const size_t W = (size_t)c->width;
    v.x = take((size_t)v.Mpad * W * 4);          // residual stream, fp32
    v.a = take((size_t)v.Mpad * 2 * W * 2);      // LN output, then attention output: fp16 pairs
    v.qkv = take((size_t)v.Mpad * 3 * W * 4);    // q | k | v, fp32
    v.hbuf = take((size_t)v.Mpad * 8 * W * 2);   // MLP hidden, fp16 pairs
    v.y = take((size_t)B * W * 4);               // ln_final of the end-of-text rows
    v.total = take.off;
    return v;
}

int text_check_cfg(const mpreid_text_cfg *c) {
    ARG_CHECK(c != nullptr);
    ARG_CHECK(c->layers >= 0 && c->out_dim > 0);
    return text_check_shape(c->tokens, c->width, c->heads);
}

int text_embed(const float *prompts, const float *pos, int64_t M, int L, int W, float *x, hipStream_t stream) {
    const int64_t n4 = M * (W / 4);
    hipLaunchKernelGGL(text_add_pos_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, prompts, pos, M, L, W, x);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" size_t mpreid_text_workspace_bytes(const mpreid_text_cfg *cfg, int batch) {
    if (!cfg || batch <= 0 || cfg->tokens <= 0 || cfg->width <= 0) return 0;
    return text_layout(cfg, batch).total;
}

extern "C" int mpreid_text_forward(const mpreid_text_cfg *cfg, const mpreid_text_weights *w, const float *prompts,
                                   const int32_t *eot, int B, float *out, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    int rc = text_check_cfg(cfg);
    if (rc) return rc;
    ARG_CHECK(w && prompts && eot && out && B > 0);
    ARG_CHECK(w->pos_emb && w->ln_final_g && w->ln_final_b && w->proj && (w->layers || cfg->layers == 0));
    ARG_CHECK(((uintptr_t)prompts & 15) == 0 && ((uintptr_t)w->pos_emb & 15) == 0 && ((uintptr_t)eot & 3) == 0 &&
              ((uintptr_t)out & 3) == 0);
    ARG_CHECK((int64_t)B * cfg->tokens <= ((int64_t)1 << 31) - 256);   // GemmArgs::M is an int
    const TextLayout v = text_layout(cfg, B);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("text workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    hipStream_t stream = (hipStream_t)stream_;
    const int W = cfg->width, L = cfg->tokens;
    char *base = (char *)ws;
    float *x = (float *)(base + v.x);
    _Float16 *a = (_Float16 *)(base + v.a);
    float *qkv = (float *)(base + v.qkv);
    _Float16 *hbuf = (_Float16 *)(base + v.hbuf);
    float *y = (float *)(base + v.y);
    if ((rc = text_embed(prompts, w->pos_emb, v.M, L, W, x, stream))) return rc;
    const BlockShape shape{W, cfg->heads, B, L, true};
    for (int l = 0; l < cfg->layers; ++l)
        if ((rc = tower_block(shape, w->layers[l], x, a, qkv, hbuf, (int)v.Mpad, stream))) return rc;
    // ln_final on the end-of-text row alone (LayerNorm is per row: the same values as normalising every row first), @ proj
    return tower_head(x, (int64_t)L * W, eot, L, B, W, cfg->out_dim, w->ln_final_g, w->ln_final_b, w->proj, nullptr, nullptr,
                      nullptr, nullptr, y, out, cfg->out_dim, 0, false, stream);
}
