"""Inputs and float64 restatements of the image tower's gradient tests (test_gpu_vit_grad.py on the GPU, test_vit_grad_cpu.py on
the host).

Attention: text_cases.make_qkv's data (q, k ~ N(0, 2), v ~ N(0, 1)) at the image tower's token counts, unmasked.  At two tokens
the slab (image 0, head 0) is made SATURATED: q_i = k_i * 8 * SAT_SCORE / |k_i|^2 for both of its rows (the row's score of its
own key is SAT_SCORE, of the other key a small fraction of it), so that each row puts all but 1e-10 .. 1e-6 of its probability
on its own key -- beyond what fp32 holds of 1 - P, so the plain form of dS has no digits left there,
while float64 keeps nine.  The error figure is text_grad_cases.grad_figure (slab-relative per dq / dk / dv).

Tower: `tower` restates oracle.vit_features with torch operations on tensors that may require grad and returns the three
features of the training forward (f_last, f, f_proj)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import text_cases as tc
import text_grad_cases as tg
from mpreid import synth

BOUND = 2e-5                                   # the project's split-mode bar
ATT_SHAPES = [(128, 2), (768, 12)]             # (width, heads)
ATT_BATCH = 3
#: the minimum, both sides of the 64-row LDS block edges the two passes stream in (64, 128, 256), of the 8-row tile edge (129 =
#: 16 * 8 + 1, 257), the shipped geometries (129, 197, 257, 442)
ATT_TOKENS = [2, 3, 63, 64, 65, 128, 129, 130, 197, 256, 257, 258, 442]
ATT_MAX = (128, 2, 1025, 1)                    # (width, heads, tokens, batch): the limit
SAT_SCORE = 18.0
MASK_FLOOR = 0.1                               # a causally masked gradient is at least this far away in the figure


def make_qkv(width, heads, batch, tokens):
    qkv = tc.make_qkv(width, heads, batch, tokens)
    if tokens == 2:
        t = qkv.view(batch, tokens, 3, heads, 64)
        k = t[0, :, 1, 0]
        t[0, :, 0, 0] = k * (8.0 * SAT_SCORE / (k * k).sum(dim=1, keepdim=True))
    return qkv


def all_keys(L):
    return torch.ones(L, L, dtype=torch.bool)


def probabilities(qkv, batch, heads):
    """float64 softmax(q k^T / 8) -> [batch, heads, L, L]"""
    q, k, _ = tc.split_heads(qkv, batch, heads)
    return torch.softmax(q @ k.transpose(2, 3) / 8.0, -1)


@functools.lru_cache(maxsize=None)
def attention_grad_case(width, heads, tokens, batch=ATT_BATCH):
    """(qkv, d_o, float64 gradient of the unmasked attention) of one shape, computed once and shared"""
    qkv = make_qkv(width, heads, batch, tokens)
    d_o = tg.make_d_o(width, batch, tokens)
    return qkv, d_o, tg.attention_grad(qkv, d_o, batch, heads, all_keys(tokens))


#: saturated slabs of more than one block (text_grad_cases.saturate, unmasked): the minimum above two tokens, one key past the
#: first 64-key block, past the second, past the fourth, and the longest shipped geometry (a ragged tail of 58 keys)
SAT_TOKENS = [3, 65, 129, 257, 442]
TIED_TOKENS = 129


@functools.lru_cache(maxsize=None)
def saturated_case(width, heads, tokens, tied=False, batch=ATT_BATCH):
    """(qkv, d_o, float64 gradient) of an unmasked case whose slab (0, 0) is saturated with the strongest keys spread over every
    64-key block (and whose slab (1, 0) holds two exact copies of the strongest key in every fourth row)"""
    qkv = tg.saturate(tc.make_qkv(width, heads, batch, tokens), batch, heads, False, tied)
    d_o = tg.make_d_o(width, batch, tokens)
    return qkv, d_o, tg.attention_grad(qkv, d_o, batch, heads, all_keys(tokens))


# ----------------------------------------------------------------------------------------------
# the tower
# ----------------------------------------------------------------------------------------------
REDUCED = dict(patch=16, stride=16, width=128, layers=3, heads=2, out_dim=64)


def tower_cfg(img_hw, base=REDUCED, **over):
    cfg = dict(base, **over)
    cfg["h_res"] = (img_hw[0] - cfg["patch"]) // cfg["stride"] + 1
    cfg["w_res"] = (img_hw[1] - cfg["patch"]) // cfg["stride"] + 1
    return cfg


def weights(sd, dtype=torch.float64):
    return {k: tc._t64(v).to(dtype) for k, v in sd.items()}


def tower(cfg, g, imgs, cv_emb=None, taps=None):
    """oracle.vit_features on tensors as they are (g: `weights`, any of them may require grad; imgs [B, 3, H, W]) ->
    (f_last [B, W], f [B, W], f_proj [B, out_dim]): the CLS row of the last block's input (model/clip/model.py:458-468),
    ln_post of the CLS row, that @ proj"""
    w, heads, p, s = cfg["width"], cfg["heads"], cfg["patch"], cfg["stride"]
    B = imgs.shape[0]
    cols = F.unfold(imgs, kernel_size=p, stride=s)
    tok = cols.transpose(1, 2) @ g["conv1.weight"].reshape(w, -1).t()
    cls = g["class_embedding"].expand(B, 1, w)
    if cv_emb is not None:
        cls = cls + cv_emb[:, None, :]
    x = torch.cat([cls, tok], dim=1) + g["positional_embedding"]
    if taps is not None:
        if x.requires_grad:
            x.retain_grad()
        taps["tokens"] = x
    x = F.layer_norm(x, (w,), g["ln_pre.weight"], g["ln_pre.bias"], 1e-5)
    if taps is not None:   # what clip_like_cases' premises look at: ln_pre's output, every block's probabilities and FC1 pre-activations
        taps["ln_pre"], taps["probs"], taps["fc1_pre"] = x.detach(), [], []
    L = x.shape[1]
    f_last = x[:, 0]
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}"
        f_last = x[:, 0]
        h = F.layer_norm(x, (w,), g[b + ".ln_1.weight"], g[b + ".ln_1.bias"], 1e-5)
        qkv = h @ g[b + ".attn.in_proj_weight"].t() + g[b + ".attn.in_proj_bias"]
        q, k, v = (t.reshape(B, L, heads, 64).transpose(1, 2) for t in qkv.split(w, dim=2))
        pr = torch.softmax((q @ k.transpose(2, 3)) * 0.125, dim=-1)
        a = (pr @ v).transpose(1, 2).reshape(B, L, w)
        x = x + a @ g[b + ".attn.out_proj.weight"].t() + g[b + ".attn.out_proj.bias"]
        h = F.layer_norm(x, (w,), g[b + ".ln_2.weight"], g[b + ".ln_2.bias"], 1e-5)
        h = h @ g[b + ".mlp.c_fc.weight"].t() + g[b + ".mlp.c_fc.bias"]
        if taps is not None:
            taps["probs"].append(pr.detach())
            taps["fc1_pre"].append(h.detach())
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ g[b + ".mlp.c_proj.weight"].t() + g[b + ".mlp.c_proj.bias"]
    f = F.layer_norm(x[:, 0], (w,), g["ln_post.weight"], g["ln_post.bias"], 1e-5)
    return f_last, f, f @ g["proj"]


#: name -> (image size, cfg overrides, batch, seed): 129 tokens; overlapping patches (stride 12); one layer (f_last is ln_pre's
#: output); two layers; 257 tokens (the attention's streaming forward form); CLIP's width, heads and depth at 9 tokens
TOWER_CASES = {
    "t129": ((256, 128), {}, 3, 51),
    "stride12": ((64, 32), dict(stride=12), 3, 52),
    "one_layer": ((64, 32), dict(layers=1), 2, 53),
    "two_layers": ((48, 32), dict(layers=2), 2, 54),
    "t257": ((256, 256), {}, 2, 55),
    "full": ((64, 32), dict(width=768, heads=12, layers=12, out_dim=512), 3, 56),
    "e2e": ((64, 32), {}, 24, 57),
}


@functools.lru_cache(maxsize=None)
def tower_case(name):
    """(cfg, img_hw, state dict, images, cv_emb, float64 (f_last, f, f_proj)) of a case, computed once and shared"""
    img_hw, over, batch, seed = TOWER_CASES[name]
    cfg = tower_cfg(img_hw, **over)
    sd = synth.vit_state_dict(cfg, seed=seed, ln_jitter=0.1)
    imgs = synth.synthetic_images(batch, img_hw[0], img_hw[1], seed=seed + 100)
    rng = np.random.default_rng(seed + 200)
    cv = (rng.standard_normal((batch, cfg["width"])) * 0.05).astype(np.float32)
    with torch.no_grad():
        want = tower(cfg, weights(sd), tc._t64(imgs), tc._t64(cv))
    return cfg, img_hw, sd, imgs, cv, want


def make_seeds(name):
    """(d_f_last, d_f, d_f_proj) of a case, float32 numpy, all non-zero"""
    cfg, _, _, imgs, _, _ = tower_case(name)
    rng = np.random.default_rng(TOWER_CASES[name][3] + 300)
    B, w, od = imgs.shape[0], cfg["width"], cfg["out_dim"]
    return tuple((rng.standard_normal(shape) * 0.1).astype(np.float32) for shape in ((B, w), (B, w), (B, od)))


@functools.lru_cache(maxsize=None)
def tower_grads(name, use=(True, True, True), with_cv=True, dtype=torch.float64):
    """{reference key name | "cv_emb" | "tokens": gradient} of sum(f_last o d_f_last) + sum(f o d_f) + sum(f_proj o d_f_proj)
    under torch autograd in `dtype` (seeds with use[i] False are left out), computed once and shared"""
    return tower_grads_on(name, tower_case(name)[3], use, with_cv, dtype)


def tower_grads_on(name, imgs, use=(True, True, True), with_cv=True, dtype=torch.float64):
    """tower_grads of a case on other images of its size (a materialised view, host-normalised uint8 pixels); not cached"""
    cfg, _, sd, _, cv, _ = tower_case(name)
    g = {k: v.clone().requires_grad_(True) for k, v in weights(sd, dtype).items()}
    cv_t = tc._t64(cv).to(dtype).requires_grad_(True) if with_cv else None
    taps = {}
    feats = tower(cfg, g, tc._t64(imgs).to(dtype), cv_t, taps)
    loss = sum((f * tc._t64(d).to(dtype)).sum() for f, d, u in zip(feats, make_seeds(name), use) if u)
    loss.backward()
    out = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in g.items()}
    if with_cv:
        out["cv_emb"] = cv_t.grad.detach()
    out["tokens"] = taps["tokens"].grad.detach()
    return out


def rel_l2(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(want).detach().cpu().double().reshape(-1)
    return float((got - want).norm() / want.norm())


def k_slice_share(grad_in_proj_bias, width):
    """the norm of the K third of an in_proj_bias gradient (exactly 0 in exact arithmetic: softmax ignores a shift common to
    all keys) over the whole tensor's norm"""
    g = torch.as_tensor(grad_in_proj_bias).detach().cpu().double()
    return float(g[width:2 * width].norm() / g.norm())


# ----------------------------------------------------------------------------------------------
# sequential fp32 restatements of the transposing and the column-reduction kernels (include/mpreid.h)
# ----------------------------------------------------------------------------------------------
KERNEL_ROWS = [1, 7, 255, 256, 257, 1033]
KERNEL_COLS = [64, 128, 768, 3072]
CS_ROWS = 128


def kernel_inputs(rows, cols):
    rng = np.random.default_rng(rows * 10007 + cols)
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    x = (rng.standard_normal((rows, cols)) * 3.0 + 0.5).astype(np.float32)
    return dy, x


MASSIVE_ROWS = 1033
MASSIVE_COLS = [128, 768, 3072]


def massive_inputs(rows, cols):
    """(dy, x) with the residual stream's massive channels of a trained CLIP tower: x ~ N(0, 1) with channel 5 at +1900 and
    channel cols / 2 + 3 at -1900; in every third row only channel 5 is massive, at 2100"""
    rng = np.random.default_rng(rows * 10007 + cols + 1)
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    c0, c1 = 5, cols // 2 + 3
    x[:, c0] += np.float32(1900.0)
    x[:, c1] -= np.float32(1900.0)
    x[::3, c0] += np.float32(200.0)
    x[::3, c1] += np.float32(1900.0)
    return dy, x


def colsum_f64(dy, x):
    """(sum_m dy, sum_m dy * xhat) in float64, xhat of LayerNorm (biased variance, eps 1e-5)"""
    dy64, x64 = dy.astype(np.float64), x.astype(np.float64)
    xhat = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-5)
    return dy64.sum(0), (dy64 * xhat).sum(0)


def transpose_pad_ref(src, rows_pad):
    out = np.zeros((src.shape[1], rows_pad), np.float32)
    out[:, :src.shape[0]] = src.T
    return out


def _wave_sum(v):
    """per row of v [rows][cols] (cols a multiple of 64): lane l adds the elements l, l + 64, ... ascending, then the butterfly
    32 .. 1; every step one fp32 addition"""
    rows, cols = v.shape
    s = np.zeros((rows, 64), np.float32)
    for i in range(cols // 64):
        s = s + v[:, i * 64:(i + 1) * 64]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ off]
    return s[:, 0]


def _pieces_sum(v):
    """column sums of v in pieces of CS_ROWS rows, rows ascending, then the pieces ascending; fp32 additions"""
    rows, cols = v.shape
    total = None
    for r0 in range(0, rows, CS_ROWS):
        part = np.zeros(cols, np.float32)
        for r in range(r0, min(rows, r0 + CS_ROWS)):
            part = part + v[r]
        total = part if total is None else total + part
    return total


def colsum_ref(dy, x):
    """(sum_m dy, sum_m dy * xhat) in the kernels' order of single fp32 operations"""
    w = np.float32(x.shape[1])
    mean = _wave_sum(x) / w
    d = x - mean[:, None]
    rstd = np.float32(1.0) / np.sqrt(_wave_sum(d * d) / w + np.float32(1e-5))
    return _pieces_sum(dy), _pieces_sum(dy * (d * rstd[:, None]))


# ----------------------------------------------------------------------------------------------
# the golden pin: the reference's own VisionTransformer under float64 autograd (tests/golden/make_goldens_vit_grad.py)
# ----------------------------------------------------------------------------------------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_grad.npz")
GOLDEN_CASE = "two_layers"
GOLDEN_BOUND = 1e-12
SMALL = 4096          # tensors of at most this many elements are stored whole
GOLDEN_ROWS = 8       # of a larger matrix: this many fixed rows and the Frobenius norm


def golden_rows(key, n_rows):
    rng = np.random.default_rng(sum(key.encode()) + n_rows)
    return np.sort(rng.choice(n_rows, GOLDEN_ROWS, replace=False))


def golden_pack(key, g):
    g = np.asarray(g, np.float64)
    if g.size <= SMALL:
        return {"g_" + key: g}
    g2 = g.reshape(g.shape[0], -1)
    return {"rows_" + key: g2[golden_rows(key, g2.shape[0])], "norm_" + key: np.float64(np.linalg.norm(g2))}


def golden_deviation(key, mine, golden):
    """relative deviation of a gradient of the restatement from what the golden file holds of the reference's"""
    mine = np.asarray(mine, np.float64)
    if "g_" + key in golden:
        want = golden["g_" + key]
        return float(np.linalg.norm(mine - want) / np.linalg.norm(want))
    m2 = mine.reshape(mine.shape[0], -1)
    want = golden["rows_" + key]
    rows = float(np.linalg.norm(m2[golden_rows(key, m2.shape[0])] - want) / np.linalg.norm(want))
    return max(rows, abs(float(np.linalg.norm(m2)) / float(golden["norm_" + key]) - 1.0))
