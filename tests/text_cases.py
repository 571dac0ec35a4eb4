"""Inputs and float64 references of the text-tower tests (test_gpu_text.py on the GPU, test_text_cpu.py on the host).

Attention: q | k | v as fp32 [B * L][3 * width], head h in columns h * 64 .. h * 64 + 63 of each third (the layout
mpreid_text_attention reads); q, k ~ N(0, 2) so that the scaled scores q . k / 8 have a standard deviation of about 2, v ~ N(0, 1)
(tests/attention_direct_cases.py, kind "plain").  The reference is softmax(q k^T / 8 + mask) v in float64 with key j visible to
query i iff j <= i.  The error figure of a call is the largest, over its (prompt, head) slabs, of max |got - want| / max |v of the
slab|: every output row is a convex combination of the slab's v rows.

Tower: a float64 restatement of model/make_model_uniprompt.py:58-68 on a CLIP-style state dict, and the prompt assembly of
PromptLearner.forward (:334-377) in plain torch."""
import functools
import math
import os

import numpy as np
import torch

from mpreid import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text.npz")

ATT_SHAPES = [(128, 2), (512, 8)]                     # (width, heads)
ATT_BATCH = 3
#: both sides of every 16-key tile edge, CLIP's length, and the limit
ATT_TOKENS = [2, 3, 16, 17, 32, 33, 48, 49, 64, 65, 77, 80, 127, 128]
BOUND_SPLIT = 2e-5                                    # the project's split-mode bar (test_gpu_attention_forms.py: BOUND["split"])
MUTANT_FLOOR = 5e-2

#: the configurations of tests/golden/text.npz (weights: synth.text_state_dict(cfg, seed); prompts, eot rows and outputs stored)
REDUCED = dict(tokens=21, width=128, layers=2, heads=2, out_dim=64)
FULL = dict(synth.CLIP_TEXT)
GOLDEN_CASES = {"reduced": (REDUCED, 31, (1, 5, 19, 20, 20)), "full": (FULL, 32, (1, 19, 40, 76))}


@functools.lru_cache(maxsize=4)
def _plain(width, heads, batch, tokens):
    rng = np.random.default_rng(100000 * tokens + 100 * width + batch)
    qkv = rng.standard_normal((batch, tokens, 3, heads, 64), dtype=np.float32)
    qkv[:, :, :2] *= np.float32(math.sqrt(2.0))
    return torch.from_numpy(qkv)


def make_qkv(width, heads, batch, tokens):
    """fp32 [batch * tokens, 3 * width] on the host"""
    assert width == 64 * heads
    return _plain(width, heads, batch, tokens).clone().reshape(batch * tokens, 3 * width).contiguous()


def split_heads(qkv, batch, heads):
    """[batch * L, 3 * width] -> q, k, v as float64 [batch, heads, L, 64]"""
    t = qkv.double().view(batch, -1, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def causal_mask(L):
    """bool [L, L]: True where key j is visible to query i (j <= i)"""
    i = torch.arange(L)
    return i[None, :] <= i[:, None]


#: wrong masks a kernel could implement instead; each as a function L -> bool [L, L] (True = visible)
def _wrong_masks():
    def idx(L):
        i = torch.arange(L)
        return i[:, None], i[None, :]
    return {
        "no_mask": lambda L: torch.ones(L, L, dtype=torch.bool),
        "one_ahead": lambda L: (lambda i, j: j <= i + 1)(*idx(L)),
        "strict": lambda L: (lambda i, j: (j < i) | ((i == 0) & (j == 0)))(*idx(L)),   # j < i; row 0 keeps key 0 (no empty row)
        "tile_granular": lambda L: (lambda i, j: (j // 16) <= (i // 16))(*idx(L)),
        "transposed": lambda L: (lambda i, j: j >= i)(*idx(L)),
    }


WRONG_MASKS = _wrong_masks()


def attention_f64(qkv, batch, heads, mask=None):
    """float64 softmax(q k^T / 8 + mask) v of the fp32 inputs -> [batch, L, heads, 64]; mask: bool [L, L], default causal"""
    q, k, v = split_heads(qkv, batch, heads)
    L = q.shape[2]
    vis = causal_mask(L) if mask is None else mask
    sc = (q @ k.transpose(2, 3) / 8.0).masked_fill(~vis, -float("inf"))
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).contiguous()


def slab_scale(qkv, batch, heads):
    """max |v| of every (prompt, head) slab -> float64 [batch, 1, heads, 1]"""
    _, _, v = split_heads(qkv, batch, heads)
    return v.abs().amax(dim=(2, 3)).view(batch, 1, heads, 1)


def error_figure(got, want, scale):
    """got, want [batch, L, heads, 64] float64 -> the largest slab-relative error"""
    return float(((got - want).abs() / scale).max())


def pairs_to_f64(out, batch, tokens, heads):
    """the kernel's fp16 pair rows [batch * tokens, 2 * width] = [hi | lo] -> float64 [batch, tokens, heads, 64]"""
    w = 64 * heads
    o = out.detach().cpu().double()
    return (o[:, :w] + o[:, w:]).view(batch, tokens, heads, 64)


@functools.lru_cache(maxsize=None)
def attention_case(width, heads, tokens, batch=ATT_BATCH):
    """(qkv, float64 reference, slab scales) of one shape, computed once and shared"""
    qkv = make_qkv(width, heads, batch, tokens)
    return qkv, attention_f64(qkv, batch, heads), slab_scale(qkv, batch, heads)


# ----------------------------------------------------------------------------------------------
# the tower in float64
# ----------------------------------------------------------------------------------------------
def _t64(v):
    return (torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.detach().cpu()).double()


def _ln64(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def tower_f64(cfg, sd, prompts, eot):
    """float64 restatement of the text encoder: prompts [B, L, W] (positional embedding not added), eot [B] -> [B, out_dim]"""
    g = {k: _t64(v) for k, v in sd.items() if k != "token_embedding.weight"}
    x = _t64(prompts) + g["positional_embedding"]
    B, L, W = x.shape
    H = cfg["heads"]
    vis = causal_mask(L)
    for l in range(cfg["layers"]):
        p = f"transformer.resblocks.{l}."
        y = _ln64(x, g[p + "ln_1.weight"], g[p + "ln_1.bias"])
        qkv = y @ g[p + "attn.in_proj_weight"].T + g[p + "attn.in_proj_bias"]
        q, k, v = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t in qkv.split(W, dim=-1))
        sc = (q @ k.transpose(2, 3) / 8.0).masked_fill(~vis, -float("inf"))
        o = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, L, W)
        x = x + o @ g[p + "attn.out_proj.weight"].T + g[p + "attn.out_proj.bias"]
        y = _ln64(x, g[p + "ln_2.weight"], g[p + "ln_2.bias"])
        h = y @ g[p + "mlp.c_fc.weight"].T + g[p + "mlp.c_fc.bias"]
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ g[p + "mlp.c_proj.weight"].T + g[p + "mlp.c_proj.bias"]
    x = _ln64(x, g["ln_final.weight"], g["ln_final.bias"])
    e = torch.as_tensor(np.asarray(eot)).long()
    return x[torch.arange(B), e] @ g["text_projection"]


def rel_l2(got, want):
    got, want = _t64(got), _t64(want)
    return float((got - want).norm() / want.norm())


def make_prompts(cfg, batch, seed):
    """embedded prompts ~ N(0, 0.02) (the scale of CLIP's token embedding), fp32 [batch, tokens, width]"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((batch, cfg["tokens"], cfg["width"])) * 0.02).astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(cfg, state dict, prompts, eot, the reference's output, the float64 restatement's output) of a stored configuration"""
    cfg, seed, _ = GOLDEN_CASES[name]
    z = np.load(GOLDEN)
    sd = synth.text_state_dict(cfg, seed=seed)
    prompts, eot, ref = z[name + "_prompts"], z[name + "_eot"], z[name + "_out"]
    return cfg, sd, prompts, eot, ref, tower_f64(cfg, sd, prompts, eot)


# ----------------------------------------------------------------------------------------------
# the prompt assembly of PromptLearner.forward in plain torch
# ----------------------------------------------------------------------------------------------
N_GENERIC, N_MODAL, N_PLAT, CTX_DIM = 8, 4, 4, 512


def prompt_learner_tensors(num_class, seed, tokens=77, dim=CTX_DIM):
    """seeded stand-ins for the prompt learner's tensors: ctx_* ~ N(0, 0.02), prefix [1, 1, dim], suffix [1, tokens - 17, dim]"""
    rng = np.random.default_rng(seed)

    def nrm(*shape):
        return torch.from_numpy((rng.standard_normal(shape) * 0.02).astype(np.float32))
    return {"ctx_generic": nrm(num_class, N_GENERIC, dim), "ctx_modality": nrm(2, N_MODAL, dim), "ctx_platform": nrm(2, N_PLAT, dim),
            "token_prefix": nrm(1, 1, dim), "token_suffix": nrm(1, tokens - 1 - N_GENERIC - N_MODAL - N_PLAT, dim)}


def assemble_prompts(t, label, stage, view=None):
    """prefix | ctx_generic[label] | modality ctx | platform ctx | suffix -> [b, tokens, dim]"""
    label = torch.as_tensor(label).long()
    b = label.shape[0]
    generic = t["ctx_generic"][label]
    if stage == "1a":
        modal = torch.zeros(b, *t["ctx_modality"].shape[1:], dtype=generic.dtype)
        plat = torch.zeros(b, *t["ctx_platform"].shape[1:], dtype=generic.dtype)
    elif view is not None:
        view = torch.as_tensor(view).long()
        plat = t["ctx_platform"][(view >= 12).long()]
        modal = t["ctx_modality"][(((view >= 6) & (view < 12)) | (view == 13)).long()]
    else:
        modal = t["ctx_modality"].mean(dim=0, keepdim=True).expand(b, -1, -1)
        plat = t["ctx_platform"].mean(dim=0, keepdim=True).expand(b, -1, -1)
    return torch.cat([t["token_prefix"].expand(b, -1, -1), generic, modal, plat, t["token_suffix"].expand(b, -1, -1)], dim=1)
