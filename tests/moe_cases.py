"""Cases and float64 references of the MoE image-encoder tests (test_gpu_moe.py on the GPU, test_moe_cpu.py on the host).

The tower: a float64 restatement of model/clip/model.py:163-258, 283-330, 415-479 in eval mode on a CLIP-style state dict
with MoE blocks first (mpreid.synth.vit_moe_state_dict).  Rows are b * L + l everywhere in this project; the reference's
flat token order is l * B + b (LND), which matters only for its router logits (golden_case converts them).

Deliberately wrong variants of the restatement (WRONG_VARIANTS) are what a kernel could implement instead; the GPU test
checks that the device output is farther than MUTANT_FLOOR from each of them on at least one case.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from mpreid import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moe.npz")
BOUND_SPLIT = 2e-5      # the project's split-mode bar (tests/text_cases.py: BOUND_SPLIT)
MARGIN_RATIO = 1000.0   # K-th / (K+1)-th logit gap >= MARGIN_RATIO * max |logits fp32 - logits float64|, on every token
#: relative L2 every wrong variant must exceed on at least one case.  Measured on the CPU (float64 variants against the
#: goldens, tests/test_moe_cpu.py prints them), each variant's largest figure over the reduced cases: re-gating 2.9e-1 on
#: `reduced` (7.0e-1 on `reduced_all`), LND / NLD mix-up 6.5e-1, no renormalisation 1.7e-2, bias outside the weight 9.6e-3.
#: The floor sits 100 x above the parity bound and 4.8 x below the smallest of them.
MUTANT_FLOOR = 2e-3

_RED = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=3, heads=2, out_dim=64)
_WIDE = dict(h_res=8, w_res=4, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
#: name -> (tower cfg incl. num_experts / top_k / moe_layers, image (h, w), images, base seed, weight std)
CASES = {
    "reduced": (dict(_RED, num_experts=4, top_k=2, moe_layers=2), (64, 32), 3, 4100, 0.05),
    "reduced_all": (dict(_RED, num_experts=3, top_k=1, moe_layers=-1), (64, 32), 3, 4200, 0.05),
    "reduced_wide": (dict(_WIDE, num_experts=8, top_k=2, moe_layers=1), (128, 64), 3, 4300, 0.05),
    "full": (dict(synth.VIT_B16, num_experts=4, top_k=2, moe_layers=2), (256, 128), 2, 4400, 0.02),
}
GATE_STD = 0.3


def resolved_moe_layers(cfg):
    return cfg["layers"] if cfg["moe_layers"] == -1 else min(cfg["moe_layers"], cfg["layers"])


def state_dict(name, seed):
    cfg, _, _, _, std = CASES[name]
    return synth.vit_moe_state_dict(cfg, seed=seed, std=std, ln_jitter=0.1, gate_std=GATE_STD)


def make_images(name, seed):
    _, (h, w), n, _, _ = CASES[name]
    return synth.synthetic_images(n, h, w, seed=seed + 500)


def _t64(v):
    return (torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.detach().cpu()).double()


def _ln64(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def rel_l2(got, want):
    got, want = _t64(got), _t64(want)
    return float((got - want).norm() / want.norm())


def topk_lower_first(p, k):
    """top-k of every row in descending value, equal values: the lower index first (a stable descending sort)"""
    order = torch.sort(p, dim=-1, descending=True, stable=True).indices
    return order[..., :k]


def route_f64(h, gate, k, renorm=True):
    """h [rows, W], gate [E, W] float64 -> (logits, sel [rows, k], w [rows, k])"""
    logits = h @ gate.T
    p = torch.softmax(logits, dim=-1)
    sel = topk_lower_first(p, k)
    ps = torch.gather(p, -1, sel)
    return logits, sel, (ps / ps.sum(-1, keepdim=True) if renorm else ps)


def experts_f64(h, sel, w, fc_w, fc_b, proj_w, proj_b, bias_outside=False):
    """sum over the selected experts, ascending e, of w * (c_proj(QuickGELU(c_fc(h))) + b_proj); h [rows, W]; weights stacked
    over experts"""
    out = torch.zeros_like(h)
    for e in range(fc_w.shape[0]):
        hit = sel == e
        rows = hit.any(-1)
        if not bool(rows.any()):
            continue   # an expert nobody chose is skipped: its weights may be anything
        we = (w * hit).sum(-1)[rows]
        t = h[rows] @ fc_w[e].T + fc_b[e]
        t = t * torch.sigmoid(1.702 * t)
        y = t @ proj_w[e].T
        out[rows] += (we[:, None] * y + proj_b[e]) if bias_outside else we[:, None] * (y + proj_b[e])
    return out


#: what a wrong implementation could do instead
WRONG_VARIANTS = ("regate", "bias_outside", "no_renorm", "lnd_mixup")


def tower_f64(cfg, sd, imgs, variant=None, cv_emb=None):
    """float64 restatement of the MoE image tower.  imgs [B, 3, H, W] -> dict(feat [B, W + out_dim] = ln_post(x)[:, 0] |
    that @ proj, logits [B * L, E] (rows b * L + l; None for a dense tower), x1 = block 0's residual stream in front of ln_2
    [B * L, W], sel / w of the routing)."""
    assert variant is None or variant in WRONG_VARIANTS
    g = {k: _t64(v) for k, v in sd.items()}
    x = F.conv2d(_t64(imgs), g["conv1.weight"], stride=cfg["stride"])
    B, W = x.shape[0], x.shape[1]
    x = x.reshape(B, W, -1).permute(0, 2, 1)
    cls = g["class_embedding"].expand(B, 1, W).clone()
    if cv_emb is not None:
        cls[:, 0] += _t64(cv_emb)
    x = _ln64(torch.cat([cls, x], 1) + g["positional_embedding"], g["ln_pre.weight"], g["ln_pre.bias"])
    L, H = x.shape[1], cfg["heads"]
    E, K = cfg.get("num_experts", 0), cfg.get("top_k", 0)
    n_moe = resolved_moe_layers(cfg) if E > 0 and K > 0 else 0
    out = dict(logits=None, x1=None, sel=None, w=None)
    sel = w = None
    for l in range(cfg["layers"]):
        p = f"transformer.resblocks.{l}."
        y = _ln64(x, g[p + "ln_1.weight"], g[p + "ln_1.bias"])
        qkv = y @ g[p + "attn.in_proj_weight"].T + g[p + "attn.in_proj_bias"]
        q, k, v = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t in qkv.split(W, dim=-1))
        o = (torch.softmax(q @ k.transpose(2, 3) / 8.0, -1) @ v).permute(0, 2, 1, 3).reshape(B, L, W)
        x = x + o @ g[p + "attn.out_proj.weight"].T + g[p + "attn.out_proj.bias"]
        h = _ln64(x, g[p + "ln_2.weight"], g[p + "ln_2.bias"])
        if l < n_moe:
            hf = h.reshape(B * L, W)
            if l == 0 or variant == "regate":
                logits, sel, w = route_f64(hf, g[p + "gate.weight"], K, renorm=variant != "no_renorm")
                if variant == "lnd_mixup":   # the routing table indexed l * B + b where the rows are b * L + l
                    sel = sel.view(B, L, K).permute(1, 0, 2).reshape(B * L, K)
                    w = w.view(B, L, K).permute(1, 0, 2).reshape(B * L, K)
                if l == 0:
                    out.update(logits=logits, x1=x.reshape(B * L, W).clone(), sel=sel, w=w)
            st = [torch.stack([g[f"{p}experts.{e}.{nm}"] for e in range(E)])
                  for nm in ("c_fc.weight", "c_fc.bias", "c_proj.weight", "c_proj.bias")]
            x = x + experts_f64(hf, sel, w, *st, bias_outside=variant == "bias_outside").view(B, L, W)
        else:
            t = h @ g[p + "mlp.c_fc.weight"].T + g[p + "mlp.c_fc.bias"]
            t = t * torch.sigmoid(1.702 * t)
            x = x + t @ g[p + "mlp.c_proj.weight"].T + g[p + "mlp.c_proj.bias"]
    c = _ln64(x[:, 0], g["ln_post.weight"], g["ln_post.bias"])
    out["feat"] = torch.cat([c, c @ g["proj"]], dim=1)
    return out


def lnd_to_rows(logits_lnd, B, L):
    """the reference's router logits [L * B, E] (flat index l * B + b) -> rows b * L + l"""
    a = np.asarray(logits_lnd)
    return np.ascontiguousarray(a.reshape(L, B, -1).transpose(1, 0, 2).reshape(B * L, -1))


def margin_figures(logits64, logits_ref32, K):
    """(smallest gap between the K-th and (K+1)-th largest float64 logit over the tokens, max |logits fp32 - float64|)"""
    l64 = _t64(logits64)
    err = float((l64 - _t64(logits_ref32)).abs().max())
    if K >= l64.shape[1]:
        return float("inf"), err
    s = torch.sort(l64, dim=-1, descending=True).values
    return float((s[:, K - 1] - s[:, K]).min()), err


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """dict(cfg, hw, seed, sd, imgs, ref = the reference's x12[:, 0] | xproj[:, 0], ref_logits (rows b * L + l), f64 = tower_f64's
    result) of a stored case, computed once and shared"""
    cfg, hw, n, _, _ = CASES[name]
    z = np.load(GOLDEN)
    seed = int(z[name + "_seed"])
    sd = state_dict(name, seed)
    imgs = z[name + "_imgs"]
    L = cfg["h_res"] * cfg["w_res"] + 1
    return dict(cfg=cfg, hw=hw, seed=seed, sd=sd, imgs=imgs, ref=z[name + "_feat"],
                ref_logits=lnd_to_rows(z[name + "_logits"], imgs.shape[0], L), f64=tower_f64(cfg, sd, imgs))


def dense_as_single_expert(sd, layers):
    """a dense state dict -> the MoE state dict (num_experts 1, every block) whose single expert holds the dense MLP"""
    out = {}
    for k, v in sd.items():
        out[k.replace(".mlp.", ".experts.0.")] = v
    w = sd["ln_pre.weight"].shape[0]
    for i in range(layers):
        out[f"transformer.resblocks.{i}.gate.weight"] = np.zeros((1, w), np.float32)
    return out
