"""Towers with the outlier structure of trained CLIP weights, and towers at the trainer's alignment, for the gradient and
training-forward tests of section 7 of test_gpu_vit_grad.py on the GPU; their premises: test_clip_like_premises_cpu.py on the host.

outlier_state_dict: massive residual channels, x30-100 LayerNorm gammas, FC1 units at +-60.  Its attention is uniform (the
massive channels take the row's variance and their ln_1 gamma is 0.02, so q k^T / 8 is about 0); clip_like_state_dict multiplies
the Q and K thirds of every in_proj_weight by a gain, which makes the attention peaked as in trained CLIP heads.

STRESS_CASES: two benign towers whose every weight-gradient GEMM has K % 16 == 0 (the trainer's 64 x 129 rows are such a
shape; no case of vit_grad_cases.TOWER_CASES is), and three clip-like towers.  Gradients come from vit_grad_cases.tower under
torch autograd in float64 and in float32.

formula_f32: the attention-gradient kernels' own expressions in fp32 on the host."""
import functools

import numpy as np
import torch

import text_cases as tc
import vit_grad_cases as vg
from mpreid import synth

EXPF_OVERFLOW = 52.13    # expf(1.702 |u|) overflows fp32 beyond this |u|
FULL9 = dict(width=768, heads=12, layers=12, out_dim=512)


def outlier_state_dict(cfg, seed=31):
    """seeded ViT weights with the outlier structure of trained CLIP towers (reference model/clip/model.py:150-161 LayerNorm,
    :260-281 block): ONE residual channel carried at about -2000 / +2000 through every block (a 'massive activation'
    channel: written by ln_pre with gamma 100 on a channel that dominates the embedding), LayerNorm gammas with a few
    channels x30-100, and FC1 units whose pre-activations sit at +-60."""
    sd = synth.vit_state_dict(cfg, seed=seed, std=0.02, ln_jitter=0.05)
    rng = np.random.default_rng(seed)
    w = cfg["width"]
    c0, c1 = 5, w // 2 + 3
    sd["positional_embedding"][:, c0] += 40.0          # dominates every token's embedding ...
    sd["positional_embedding"][:, c1] -= 40.0
    sd["ln_pre.weight"][c0] = 100.0                    # ... ln_pre turns it into ~ +-1900 in the residual stream
    sd["ln_pre.weight"][c1] = 100.0
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}"
        for ln in ("ln_1", "ln_2"):
            big = rng.choice(w, 4, replace=False)
            big = big[(big != c0) & (big != c1)]
            sd[f"{b}.{ln}.weight"][big] *= rng.uniform(30.0, 100.0, big.size).astype(np.float32)
            sd[f"{b}.{ln}.weight"][[c0, c1]] = 0.02     # trained towers damp the massive channels inside the blocks
        units = rng.choice(4 * w, 6, replace=False)
        sd[f"{b}.mlp.c_fc.bias"][units[:3]] = 60.0
        sd[f"{b}.mlp.c_fc.bias"][units[3:]] = -60.0
    return sd


def planted_units(sd, cfg, value=-60.0):
    """per layer, the FC1 units whose bias outlier_state_dict set to `value`"""
    return [np.nonzero(sd[f"transformer.resblocks.{i}.mlp.c_fc.bias"] == np.float32(value))[0] for i in range(cfg["layers"])]


def clip_like_state_dict(cfg, seed, qk_gain):
    """outlier_state_dict with rows [:2 * width] (the Q and K thirds) of every attn.in_proj_weight multiplied by qk_gain"""
    sd = outlier_state_dict(cfg, seed)
    for i in range(cfg["layers"]):
        sd[f"transformer.resblocks.{i}.attn.in_proj_weight"][:2 * cfg["width"]] *= np.float32(qk_gain)
    return sd


#: name -> (image size, cfg overrides, batch, seed, qk_gain or None for benign weights)
STRESS_CASES = {
    "aligned9": ((64, 32), {}, 16, 61, None),
    "aligned129": ((256, 128), dict(layers=2), 16, 62, None),
    "clip9": ((64, 32), {}, 16, 63, 300.0),
    "clip129": ((256, 128), dict(layers=2), 4, 64, 300.0),
    "clip_full9": ((64, 32), FULL9, 16, 65, 100.0),
}
ALIGNED = ["aligned9", "aligned129"]
CLIP_LIKE = ["clip9", "clip129", "clip_full9"]


def alignment(name):
    """(align4(B * L), align4(B), B * P) of a case: the K of the block matrices', of proj's and of conv1's weight-gradient GEMM"""
    cfg, _, _, imgs, _, _ = stress_case(name)
    B, P = imgs.shape[0], cfg["h_res"] * cfg["w_res"]
    a4 = lambda n: (n + 3) // 4 * 4
    return a4(B * (P + 1)), a4(B), B * P


@functools.lru_cache(maxsize=None)
def stress_case(name):
    """vit_grad_cases.tower_case for a stress case: (cfg, img_hw, state dict, images, cv_emb, float64 (f_last, f, f_proj))"""
    img_hw, over, batch, seed, gain = STRESS_CASES[name]
    cfg = vg.tower_cfg(img_hw, **over)
    if gain is None:
        sd = synth.vit_state_dict(cfg, seed=seed, ln_jitter=0.1)
    else:
        sd = clip_like_state_dict(cfg, seed, gain)
    imgs = synth.synthetic_images(batch, img_hw[0], img_hw[1], seed=seed + 100)
    rng = np.random.default_rng(seed + 200)
    cv = (rng.standard_normal((batch, cfg["width"])) * 0.05).astype(np.float32)
    with torch.no_grad():
        want = vg.tower(cfg, vg.weights(sd), tc._t64(imgs), tc._t64(cv))
    return cfg, img_hw, sd, imgs, cv, want


def make_seeds(name):
    """(d_f_last, d_f, d_f_proj) of a case, float32 numpy, all non-zero (as vit_grad_cases.make_seeds)"""
    cfg, _, _, imgs, _, _ = stress_case(name)
    rng = np.random.default_rng(STRESS_CASES[name][3] + 300)
    B, w, od = imgs.shape[0], cfg["width"], cfg["out_dim"]
    return tuple((rng.standard_normal(shape) * 0.1).astype(np.float32) for shape in ((B, w), (B, w), (B, od)))


def _run(name, dtype, grad=True):
    cfg, _, sd, imgs, cv, _ = stress_case(name)
    g = {k: v.clone().requires_grad_(grad) for k, v in vg.weights(sd, dtype).items()}
    cv_t = tc._t64(cv).to(dtype).requires_grad_(grad)
    taps = {}
    feats = vg.tower(cfg, g, tc._t64(imgs).to(dtype), cv_t, taps)
    return g, cv_t, taps, feats


@functools.lru_cache(maxsize=None)
def stress_grads(name, dtype=torch.float64):
    """{reference key name | "cv_emb" | "tokens": gradient} of sum(f_last o d_f_last) + sum(f o d_f) + sum(f_proj o d_f_proj)
    under torch autograd in `dtype`, computed once and shared"""
    g, cv_t, taps, feats = _run(name, dtype)
    loss = sum((f * tc._t64(d).to(dtype)).sum() for f, d in zip(feats, make_seeds(name)))
    loss.backward()
    out = {k: v.grad.detach() for k, v in g.items()}
    out["cv_emb"] = cv_t.grad.detach()
    out["tokens"] = taps["tokens"].grad.detach()
    return out


@functools.lru_cache(maxsize=None)
def stress_features(name, dtype=torch.float32):
    """(f_last, f, f_proj) of the restatement in `dtype` with cv_emb"""
    with torch.no_grad():
        return tuple(f.detach() for f in _run(name, dtype, grad=False)[3])


@functools.lru_cache(maxsize=None)
def stress_taps(name):
    """float64: dict(ln_pre = ln_pre's output, probs = per block [B, heads, L, L], fc1_pre = per block [B, L, 4 width])"""
    with torch.no_grad():
        return _run(name, torch.float64, grad=False)[2]


def host_figures(name):
    """{tensor: relative L2 of fp32 autograd against float64 autograd}"""
    want, f32 = stress_grads(name), stress_grads(name, torch.float32)
    return {k: vg.rel_l2(f32[k], want[k]) for k in want}


def formula_f32(qkv, d_o, batch, heads, mask):
    """The attention-gradient kernels' own expressions in fp32 with torch on the host: the row's maximum m, the FIRST key j* that
    holds it, sum = sum_j exp(s_j - m), P = exp(s - m) / sum, r = dP[j*], dot = sum_j P_j (dP_j - r), dS = P ((dP - r) - dot);
    dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO.  mask: bool [L, L], True where key j is visible to query i.
    -> d_qkv [batch * L, 3 * width] fp32"""
    t = qkv.detach().cpu().float().view(batch, -1, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    L = q.shape[2]
    g = d_o.detach().cpu().float().view(batch, L, heads, 64).permute(0, 2, 1, 3)
    s = ((q @ k.transpose(2, 3)) * 0.125).masked_fill(~mask, -float("inf"))
    m = s.amax(dim=-1, keepdim=True)
    idx = torch.arange(L).expand_as(s)
    jstar = torch.where(s == m, idx, torch.full_like(idx, L)).amin(dim=-1, keepdim=True)
    e = torch.exp(s - m)
    p = e / e.sum(dim=-1, keepdim=True)
    dp = g @ v.transpose(2, 3)
    c = dp - dp.gather(-1, jstar)
    ds = p * (c - (p * c).sum(dim=-1, keepdim=True))
    dq, dk, dv = (ds @ k) * 0.125, (ds.transpose(2, 3) @ q) * 0.125, p.transpose(2, 3) @ g
    out = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4)   # [batch, L, 3, heads, 64]
    return out.reshape(batch * L, 3 * heads * 64).contiguous()
