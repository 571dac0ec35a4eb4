"""Float64 oracles of the text tower's prompt gradient (test_gpu_text_grad.py on the GPU, test_text_grad_cpu.py on the host).

text_cases.tower_f64 / attention_f64 detach their inputs, so they cannot carry a gradient; `tower` and `attention` below restate
them with the same torch operations in the same order on tensors that may require grad (test_text_grad_cpu.py: their forward
values equal the originals exactly), and the gradients come from torch.autograd.grad.  There is no reference golden: the
reference's text tower is the same graph, already pinned by tests/golden/text.npz.

The error figure of an attention gradient: d_qkv = dq | dk | dv, each part viewed as [batch, L, heads, 64]; for each part
text_cases.error_figure with the part's own slab scale (max |want| over every (prompt, head) slab); the figure of a call is the
largest of the three."""
import functools

import numpy as np
import torch

import text_cases as tc

#: the minimum, both sides of every tile edge of the forward kernel's neighbourhood, CLIP's own count, and the limit
GRAD_TOKENS = [2, 3, 16, 17, 64, 65, 77, 127, 128]


def _ln(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def weights(sd, dtype=torch.float64):
    return {k: tc._t64(v).to(dtype) for k, v in sd.items() if k != "token_embedding.weight"}


def tower(cfg, g, prompts, eot):
    """text_cases.tower_f64 on tensors as they are (g: `weights`; prompts [B, L, W] may require grad) -> [B, out_dim]"""
    x = prompts + g["positional_embedding"]
    B, L, W = x.shape
    H = cfg["heads"]
    vis = tc.causal_mask(L)
    for l in range(cfg["layers"]):
        p = f"transformer.resblocks.{l}."
        y = _ln(x, g[p + "ln_1.weight"], g[p + "ln_1.bias"])
        qkv = y @ g[p + "attn.in_proj_weight"].T + g[p + "attn.in_proj_bias"]
        q, k, v = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t in qkv.split(W, dim=-1))
        sc = (q @ k.transpose(2, 3) / 8.0).masked_fill(~vis, -float("inf"))
        o = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, L, W)
        x = x + o @ g[p + "attn.out_proj.weight"].T + g[p + "attn.out_proj.bias"]
        y = _ln(x, g[p + "ln_2.weight"], g[p + "ln_2.bias"])
        h = y @ g[p + "mlp.c_fc.weight"].T + g[p + "mlp.c_fc.bias"]
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ g[p + "mlp.c_proj.weight"].T + g[p + "mlp.c_proj.bias"]
    x = _ln(x, g["ln_final.weight"], g["ln_final.bias"])
    e = torch.as_tensor(np.asarray(eot)).long()
    return x[torch.arange(B), e] @ g["text_projection"]


def attention(qkv, batch, heads, mask=None):
    """text_cases.attention_f64 on a [batch * L, 3 * width] tensor as it is (any float dtype) -> [batch, L, heads, 64]"""
    t = qkv.view(batch, -1, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    L = q.shape[2]
    vis = tc.causal_mask(L) if mask is None else mask
    sc = (q @ k.transpose(2, 3) / 8.0).masked_fill(~vis, -float("inf"))
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).contiguous()


def tower_grad(cfg, sd, prompts, eot, grad_out):
    """float64 d <grad_out, tower(prompts)> / d prompts -> [B, L, W]"""
    p = tc._t64(prompts).requires_grad_(True)
    out = tower(cfg, weights(sd), p, eot)
    return torch.autograd.grad(out, p, grad_outputs=tc._t64(grad_out))[0]


def attention_grad(qkv, d_o, batch, heads, mask=None, dtype=torch.float64):
    """d <d_o, attention(qkv)> / d qkv in `dtype` on the host -> [batch * L, 3 * width]"""
    x = qkv.detach().cpu().to(dtype).requires_grad_(True)
    out = attention(x, batch, heads, mask)
    return torch.autograd.grad(out, x, grad_outputs=d_o.detach().cpu().to(dtype).view(out.shape))[0]


def grad_figure(got, want, batch, heads):
    """the error figure of an attention gradient (module docstring); got, want [batch * L, 3 * width]"""
    g = got.detach().cpu().double().view(batch, -1, 3, heads, 64)
    w = want.detach().cpu().double().view(batch, -1, 3, heads, 64)
    figs = []
    for part in range(3):
        scale = w[:, :, part].abs().amax(dim=(1, 3)).view(batch, 1, heads, 1)
        figs.append(tc.error_figure(g[:, :, part], w[:, :, part], scale))
    return max(figs)


def make_d_o(width, batch, tokens):
    """the incoming gradient of an attention case: N(0, 1), fp32 [batch * tokens, width]"""
    rng = np.random.default_rng(7000000 + 1000 * tokens + width + batch)
    return torch.from_numpy(rng.standard_normal((batch * tokens, width), dtype=np.float32))


@functools.lru_cache(maxsize=None)
def attention_grad_case(width, heads, tokens, batch=tc.ATT_BATCH):
    """(qkv, d_o, float64 gradient) of one shape, computed once and shared; qkv is text_cases' input of the shape"""
    qkv = tc.make_qkv(width, heads, batch, tokens)
    d_o = make_d_o(width, batch, tokens)
    return qkv, d_o, attention_grad(qkv, d_o, batch, heads)


# ----------------------------------------------------------------------------------------------
# saturated slabs of more than one 64-key block (both attention-gradient kernels; vit_grad_cases uses the same construction)
# ----------------------------------------------------------------------------------------------
SAT_SCORE = 18.0
#: the minimum above two tokens, both sides of the 16-key tile and of the second lane half (keys 64 ..), CLIP's count, the limit
SAT_TOKENS = [3, 17, 65, 77, 128]
TIED_TOKENS = 128


def strongest_keys(L, causal):
    """the key row i of the saturated slab is pointed at: (37 i + 5) mod L unmasked, mod (i + 1) under the causal mask"""
    i = torch.arange(L)
    return (37 * i + 5) % ((i + 1) if causal else torch.full_like(i, L))


def tied_targets(L, causal):
    """{query row: key} of the tied slab: every fourth row is pointed at key 63 (whose copy is key 64) or at key 0 (whose copy
    is key L - 1), in turn.  Under the causal mask a row sees both copies of key 63 from row 64 on, so earlier rows take key 0;
    the last row is the only one that sees key L - 1, so it is pointed at key 0 too."""
    out = {}
    for n, i in enumerate(range(0, L, 4)):
        want63 = L >= 65 and n % 2 == 0 and (not causal or i >= 64)
        out[i] = 63 if want63 else 0
    if causal:
        out[L - 1] = 0
    return out


def saturate(qkv, batch, heads, causal, tied=False):
    """In place on make_qkv's tensor.  Slab (image 0, head 0): q_i = k_j * 8 * SAT_SCORE / |k_j|^2 with j = strongest_keys: every
    row's score of that key is SAT_SCORE, of any other a few units, so the row puts all but ~1e-6 of its probability on it, and
    the strongest keys visit every 64-key block and the ragged tail.  tied: in slab (1, 0) key rows 63 and 64, and key rows 0 and
    L - 1, are exact copies of each other and the rows of tied_targets are pointed at one of them: two keys hold the row's
    maximum to the bit.  The other slabs stay ordinary."""
    t = qkv.view(batch, -1, 3, heads, 64)
    L = t.shape[1]
    k = t[0, :, 1, 0][strongest_keys(L, causal)]
    t[0, :, 0, 0] = k * (8.0 * SAT_SCORE / (k * k).sum(dim=1, keepdim=True))
    if tied:
        if L >= 65:
            t[1, 64, 1, 0] = t[1, 63, 1, 0]
        t[1, L - 1, 1, 0] = t[1, 0, 1, 0]
        for i, j in tied_targets(L, causal).items():
            kj = t[1, j, 1, 0]
            t[1, i, 0, 0] = kj * (8.0 * SAT_SCORE / (kj * kj).sum())
    return qkv


def slab(x, batch, heads, b, h):
    """the (image b, head h) slab of a [batch * L, 3 * width] gradient as a [L, 3 * 64] tensor (grad_figure(.., 1, 1) judges it)"""
    return x.detach().cpu().view(batch, -1, 3, heads, 64)[b, :, :, h].reshape(-1, 3 * 64)


@functools.lru_cache(maxsize=None)
def saturated_case(width, heads, tokens, tied=False, batch=tc.ATT_BATCH):
    """(qkv, d_o, float64 gradient) of a causal case whose slab (0, 0) is saturated (and whose slab (1, 0) is tied)"""
    qkv = saturate(tc.make_qkv(width, heads, batch, tokens), batch, heads, True, tied)
    d_o = make_d_o(width, batch, tokens)
    return qkv, d_o, attention_grad(qkv, d_o, batch, heads)


def make_grad_out(batch, out_dim, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((batch, out_dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tower_grad_case(name):
    """(cfg, sd, prompts, eot, grad_out, float64 prompt gradient) of a golden configuration with the eot rows of GOLDEN_CASES"""
    cfg, sd, prompts, _, _, _ = tc.golden_case(name)
    eot = list(tc.GOLDEN_CASES[name][2])
    assert len(eot) == prompts.shape[0]
    g = make_grad_out(len(eot), cfg["out_dim"], seed=900 + len(name))
    return cfg, sd, prompts, eot, g, tower_grad(cfg, sd, prompts, eot, g)


def contrastive(a, b, la, lb):
    """the supervised contrastive loss of the reference's prompt learning (loss/supcontrast.py, temperature 1): the mean over
    the rows of a of minus the mean log-softmax probability of the columns of b that carry the row's label"""
    logp = torch.log_softmax(a @ b.T, dim=1)
    pos = (la[:, None] == lb[None, :]).to(logp.dtype)
    return -((pos * logp).sum(1) / pos.sum(1)).mean()


def symmetric_loss(image_features, text_features, target):
    """processor/processor_uniprompt_stage1.py:90-93: image -> text plus text -> image"""
    return contrastive(image_features, text_features, target, target) + contrastive(text_features, image_features, target, target)
