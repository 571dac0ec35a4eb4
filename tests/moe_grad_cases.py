"""Cases and float64 references of the MoE tower's backward (test_gpu_moe_grad.py on the GPU, test_moe_grad_cpu.py on the host).
Built on moe_cases (the forward's float64 restatement) and vit_grad_cases (the gradient bar, the golden packing).  Three parts:

  seams   the gradient through one routed MLP (mpreid_moe_mlp_backward) and the router's gradient with the load-balancing
          loss (mpreid_moe_route_backward): autograd and closed forms, routings, wrong variants of the router gradient
  tower   a differentiable float64 restatement of the MoE tower (tower / tower_case / tower_grads), pinned to the REFERENCE's
          own VisionTransformer by tests/golden/moe_grad.npz (golden_deviations); cases, wrong variants of the sweep
  e2e     the fused stage-2 step on a small MoE tower against the same loop in float64

Seams: two statements of each gradient: autograd through the float64 forward, and the closed forms the kernels implement
(include/mpreid.h).  test_moe_grad_cpu.py checks the one against the other; the GPU tests compare the device with autograd.

Deliberately wrong variants of the router gradient (ROUTE_WRONG_VARIANTS) are what a kernel could compute instead.  Their
relative L2 from the right d_logits, float64 on the CPU over ROUTE_EK at 300 rows (tests/test_moe_grad_cpu.py prints them),
smallest figure of each variant over the cases that can tell it apart (variant_applies):
    no_grad_through_w (routing term dropped)                                              1.0
    aux_dropped (judged alone, d_w = 0: beside a unit seed the term is ~1e-6 of the total)  1.0
    softmax_correction (top-k of the softmax without the renormalisation)                 2.45e-1 (E 3, K 2)
The floor sits 100 x above the parity bound and 120 x below the smallest of them.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import moe_cases as mc
import vit_grad_cases as vg
from mpreid import synth

BOUND = vg.BOUND            # 2e-5: relative L2 per tensor
MUTANT_FLOOR = 2e-3         # 100 x BOUND
AUX_COEF = 0.01             # processor_uniprompt_stage2.py:76

#: (E, K) of the router gradient cases
ROUTE_EK = [(E, K) for E in (1, 3, 8, 64) for K in sorted({1, 2, E}) if K <= min(E, 8)]
ROUTE_ROWS = 1300           # more than one 1024-row count workgroup, several 256-row pieces, a ragged last piece


def quickgelu(t):
    return t * torch.sigmoid(1.702 * t)


def quickgelu_slope(t):
    s = torch.sigmoid(1.702 * t)
    return s + 1.702 * t * s * (1 - s)


def mlp_backward_autograd(h, sel, w, fc_w, fc_b, proj_w, proj_b, dy):
    """float64 autograd through moe_cases.experts_f64: gradients of sum(out * dy) with respect to h and w"""
    h = mc._t64(h).clone().requires_grad_(True)
    w = mc._t64(w).clone().requires_grad_(True)
    out = mc.experts_f64(h, torch.as_tensor(sel).long(), w, *(mc._t64(a) for a in (fc_w, fc_b, proj_w, proj_b)))
    (out * mc._t64(dy)).sum().backward()
    return h.grad, w.grad


def mlp_backward_closed(h, sel, w, fc_w, fc_b, proj_w, proj_b, dy):
    """the closed forms of include/mpreid.h, slot by slot, float64"""
    h, w, dy = mc._t64(h), mc._t64(w), mc._t64(dy)
    fc_w, fc_b, proj_w, proj_b = (mc._t64(a) for a in (fc_w, fc_b, proj_w, proj_b))
    sel = torch.as_tensor(sel).long()
    d_a, d_w = torch.zeros_like(h), torch.zeros_like(w)
    for e in range(fc_w.shape[0]):            # ascending e
        for k in range(sel.shape[1]):
            rows = (sel[:, k] == e).nonzero().flatten()
            if rows.numel() == 0:
                continue
            u = h[rows] @ fc_w[e].T + fc_b[e]
            y = quickgelu(u) @ proj_w[e].T + proj_b[e]
            d_w[rows, k] = (dy[rows] * y).sum(-1)
            dt = (w[rows, k, None] * dy[rows]) @ proj_w[e]
            d_a[rows] += (dt * quickgelu_slope(u)) @ fc_w[e]
    return d_a, d_w


def load_balancing_loss(logits, sel):
    """model/clip/model.py:342-377 restated on tensors that may require grad: E * sum_e f_e P_e, f not differentiated"""
    E = logits.shape[-1]
    p = torch.softmax(logits, dim=-1)
    f = torch.nn.functional.one_hot(sel, E).to(logits.dtype).mean(0)       # [K, E]
    return (f * p.mean(0)).sum() * E


def route_backward_autograd(logits, K, d_w, coef, variant=None):
    """float64 autograd: d/dlogits of sum(w * d_w) + coef * l_aux, w = renormalised top-k of softmax(logits).  Returns
    (d_logits, l_aux, sel, w)."""
    lg = mc._t64(logits).clone().requires_grad_(True)
    p = torch.softmax(lg, dim=-1)
    sel = mc.topk_lower_first(p.detach(), K)
    ps = torch.gather(p, -1, sel)
    w = ps if variant == "softmax_correction" else ps / ps.sum(-1, keepdim=True)
    l_aux = load_balancing_loss(lg, sel)
    loss = lg.sum() * 0.0
    if variant != "no_grad_through_w":
        loss = loss + (w * mc._t64(d_w)).sum()
    if variant != "aux_dropped":
        loss = loss + coef * l_aux
    loss.backward()
    wn = (ps / ps.sum(-1, keepdim=True)).detach()
    return lg.grad, l_aux.detach(), sel, wn


ROUTE_WRONG_VARIANTS = ("no_grad_through_w", "aux_dropped", "softmax_correction")


def variant_applies(variant, E, K):
    """False where the variant computes the right thing: the routing term is zero for K == 1, the renormalisation is the identity
    for K == E, and the load-balancing gradient vanishes for K == E (f_e = 1 for every e makes g uniform)"""
    return {"no_grad_through_w": K >= 2, "aux_dropped": K < E, "softmax_correction": 2 <= K < E}[variant]


def variant_seed(variant, d_w):
    """the d_w a variant is judged on.  The load-balancing term is ~coef * E / rows of the routing term under a seed of unit
    size, far below any bound, so it is judged alone (d_w = 0), which is also how the device test isolates it."""
    return np.zeros_like(d_w) if variant == "aux_dropped" else d_w


def route_backward_closed(logits, sel, w, d_w, coef):
    """the closed forms of include/mpreid.h, float64"""
    lg, w, d_w = mc._t64(logits), mc._t64(w), mc._t64(d_w)
    rows, E = lg.shape
    p = torch.softmax(lg, dim=-1)
    c = (w * d_w).sum(-1, keepdim=True)
    d = torch.zeros_like(lg)
    d.scatter_(1, sel, w * (d_w - c))
    f = torch.zeros(E, dtype=torch.float64)
    f.scatter_add_(0, sel.flatten(), torch.ones(sel.numel(), dtype=torch.float64))
    f = f / rows
    g = coef * E * f / rows
    d = d + p * (g - (p * g).sum(-1, keepdim=True))
    return d, E * (f * p.mean(0)).sum()


def route_case(E, K, rows=ROUTE_ROWS, seed=0):
    """logits with a clear top-k margin (no float32 / float64 disagreement about the selection) and a seed for d_w"""
    rng = np.random.default_rng(1000 * E + 10 * K + seed)
    logits = rng.standard_normal((rows, E)).astype(np.float32) * 1.5
    # keep the K-th / (K+1)-th gap away from rounding: redraw rows whose gap is below 1e-3
    if K < E:
        for _ in range(50):
            s = np.sort(logits, -1)[:, ::-1]
            bad = (s[:, K - 1] - s[:, K]) < 1e-3
            if not bad.any():
                break
            logits[bad] = rng.standard_normal((int(bad.sum()), E)).astype(np.float32) * 1.5
    d_w = rng.standard_normal((rows, K)).astype(np.float32)
    return logits, d_w


def mlp_weights(E, width, rng, nan_unused=None):
    fc_w = (rng.standard_normal((E, 4 * width, width)) * width ** -0.5).astype(np.float32)
    fc_b = (rng.standard_normal((E, 4 * width)) * 0.1).astype(np.float32)
    proj_w = (rng.standard_normal((E, width, 4 * width)) * (4 * width) ** -0.5).astype(np.float32)
    proj_b = (rng.standard_normal((E, width)) * 0.1).astype(np.float32)
    if nan_unused is not None:
        for e in nan_unused:
            fc_w[e] = fc_b[e] = proj_w[e] = proj_b[e] = np.nan
    return fc_w, fc_b, proj_w, proj_b


#: routings of the routed-MLP seam at E = 4 (those of test_gpu_moe.py::test_routed_mlp_against_float64, and one of more than
#: 1024 rows): segment sizes on both sides of the 128-row tile, an empty expert between used ones, K = 1, 2 and E
MLP_KINDS = ["counts_0_1_127_128", "counts_129_0_0_255", "counts_one_expert_three_tiles", "k2_hole", "k_all", "k2_1300_rows"]
MLP_E = 4


def mlp_routing(kind):
    """(sel int32 [rows, K], w fp32 [rows, K] summing to one per row)"""
    rng = np.random.default_rng(7)
    E = MLP_E
    if kind.startswith("counts"):
        counts = {"counts_0_1_127_128": (0, 1, 127, 128), "counts_129_0_0_255": (129, 0, 0, 255),
                  "counts_one_expert_three_tiles": (0, 0, 300, 0)}[kind]
        sel = rng.permutation(np.concatenate([np.full(c, e, np.int32) for e, c in enumerate(counts)]))[:, None]
    elif kind == "k2_hole":         # two experts per row out of {0, 2, 3}: expert 1 stays empty between used ones
        sel = np.stack([rng.permutation(np.array([0, 2, 3], np.int32))[:2] for _ in range(193)])
    elif kind == "k2_1300_rows":    # two dispatch workgroups, several tiles per expert
        sel = np.stack([rng.permutation(E).astype(np.int32)[:2] for _ in range(1300)])
    else:                           # k == E: every row on every expert, in a shuffled order
        sel = np.stack([rng.permutation(E).astype(np.int32) for _ in range(130)])
    w = rng.uniform(0.1, 1.0, size=sel.shape).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    return np.ascontiguousarray(sel), np.ascontiguousarray(w.astype(np.float32))


# ----------------------------------------------------------------------------------------------
# the tower
# ----------------------------------------------------------------------------------------------
_WIDE = dict(h_res=8, w_res=4, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
#: name -> (tower cfg, image (h, w), images, base seed, weight std).  The first three are moe_cases' shapes (2 of 3 blocks MoE;
#: every block MoE with K = 1, where the routing gradient is exactly zero; 33 tokens and 8 experts); `full`: CLIP's width, heads
#: and depth at 9 tokens, 27 rows; `rows1320`: 40 images of 33 tokens, more than one 1024-row dispatch workgroup and several
#: 128-row tiles per expert; `aligned`: `reduced` with 16 images, 144 token rows: align4(M) = 144, align4(B) = 16 and B P = 128 are
#: multiples of 16, the fast staging of every weight-gradient GEMM (28 / 100 / 260 rows in the other cases: none is).
TOWER_CASES = {
    "reduced": mc.CASES["reduced"],
    "reduced_all": mc.CASES["reduced_all"],
    "reduced_wide": mc.CASES["reduced_wide"],
    "full": (dict(synth.VIT_B16, h_res=4, w_res=2, num_experts=4, top_k=2, moe_layers=2), (64, 32), 3, 5400, 0.02),
    "rows1320": (dict(_WIDE, num_experts=4, top_k=2, moe_layers=1), (128, 64), 40, 5500, 0.05),
    "aligned": (dict(mc._RED, num_experts=4, top_k=2, moe_layers=2), (64, 32), 16, 5600, 0.05),
}
#: what a wrong sweep could compute instead.  Relative L2 from the right gradient on (gate.weight, tokens), float64 on the CPU
#: (tests/test_moe_grad_cpu.py prints them); the case on which each variant is judged is the one where it is farthest:
#:   no_grad_through_w   `reduced`  1.0, 5.0e-1      regate             `reduced`  4.1e-1, 3.9e-1
#:   f_last_at_input     `reduced`  4.0e-1, 2.4e-1   d_w_one_block      `reduced`  7.4e-1, 2.5e-1
#:   aux_dropped         judged with the three seeds off (beside them the term is ~1e-6 of the gradient): 1.0, 1.0 on `reduced`
#: (`reduced_wide` and `rows1320` have ONE MoE block: re-gating and d_w_one_block compute the right thing there; `reduced_all`
#: has K = 1, where no routing gradient exists.)  MUTANT_FLOOR = 2e-3 is 100 x the parity bound and 120 x below the smallest (2.4e-1).
TOWER_WRONG_VARIANTS = ("no_grad_through_w", "regate", "aux_dropped", "f_last_at_input", "d_w_one_block")
TOWER_VARIANT_CASE = "reduced"


def tower_variant_use(variant):
    """which seeds a variant is judged under"""
    return (False, False, False) if variant == "aux_dropped" else (True, True, True)


def tower(cfg, g, imgs, cv_emb=None, taps=None, variant=None):
    """The MoE tower on tensors as they are (g: weights, any may require grad) -> (f_last, f, f_proj, logits [B * L, E] in rows
    b * L + l, l_aux).  f_last is the CLS row of the LAST block's OUTPUT (model/clip/model.py:448-454); the routing of block 0
    serves every MoE block (:310-322)."""
    w, heads, p, s = cfg["width"], cfg["heads"], cfg["patch"], cfg["stride"]
    E, K, n_moe = cfg["num_experts"], cfg["top_k"], mc.resolved_moe_layers(cfg)
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
    L = x.shape[1]
    logits = sel = wr = None
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}"
        x_in = x
        h = F.layer_norm(x, (w,), g[b + ".ln_1.weight"], g[b + ".ln_1.bias"], 1e-5)
        qkv = h @ g[b + ".attn.in_proj_weight"].t() + g[b + ".attn.in_proj_bias"]
        q, k, v = (t.reshape(B, L, heads, 64).transpose(1, 2) for t in qkv.split(w, dim=2))
        a = (torch.softmax((q @ k.transpose(2, 3)) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(B, L, w)
        x = x + a @ g[b + ".attn.out_proj.weight"].t() + g[b + ".attn.out_proj.bias"]
        h = F.layer_norm(x, (w,), g[b + ".ln_2.weight"], g[b + ".ln_2.bias"], 1e-5)
        if i < n_moe:
            hf = h.reshape(B * L, w)
            if i == 0 or variant == "regate":
                lg = hf @ g[b + ".gate.weight"].t()
                pr = torch.softmax(lg, dim=-1)
                sel_i = mc.topk_lower_first(pr.detach(), K)
                ps = torch.gather(pr, -1, sel_i)
                wr_i = ps / ps.sum(-1, keepdim=True)
                if variant == "no_grad_through_w":
                    wr_i = wr_i.detach()
                if i == 0:
                    logits, sel, wr = lg, sel_i, wr_i
            use_sel, use_w = (sel_i, wr_i) if variant == "regate" else (sel, wr)
            if variant == "d_w_one_block" and i != n_moe - 1:
                use_w = use_w.detach()   # only the last MoE block's d_w reaches the gate
            out = torch.zeros_like(hf)
            for e in range(E):
                hit = use_sel == e
                rows = hit.any(-1)
                if not bool(rows.any()):
                    continue
                we = (use_w * hit).sum(-1)[rows]
                t = quickgelu(hf[rows] @ g[f"{b}.experts.{e}.c_fc.weight"].t() + g[f"{b}.experts.{e}.c_fc.bias"])
                y = t @ g[f"{b}.experts.{e}.c_proj.weight"].t() + g[f"{b}.experts.{e}.c_proj.bias"]
                out = out.index_add(0, rows.nonzero().flatten(), we[:, None] * y)
            x = x + out.view(B, L, w)
        else:
            t = quickgelu(h @ g[b + ".mlp.c_fc.weight"].t() + g[b + ".mlp.c_fc.bias"])
            x = x + t @ g[b + ".mlp.c_proj.weight"].t() + g[b + ".mlp.c_proj.bias"]
    f_last = x_in[:, 0] if variant == "f_last_at_input" else x[:, 0]
    f = F.layer_norm(x[:, 0], (w,), g["ln_post.weight"], g["ln_post.bias"], 1e-5)
    return f_last, f, f @ g["proj"], logits, load_balancing_loss(logits, sel)


def _weights(sd, dtype):
    return {k: mc._t64(v).to(dtype) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def tower_case(name):
    """dict(cfg, hw, seed, sd, imgs, cv, seeds (d_f_last, d_f, d_f_proj), f64 = the float64 tower's outputs, margin, err).
    cv_emb moves the logits, so the case walks its seed until moe_cases.MARGIN_RATIO holds for ITS inputs: the gap between the
    K-th and (K+1)-th logit of every token is at least MARGIN_RATIO times the float32 restatement's distance from float64."""
    cfg, hw, n, base, std = TOWER_CASES[name]
    for seed in range(base, base + 64):
        sd = synth.vit_moe_state_dict(cfg, seed=seed, std=std, ln_jitter=0.1, gate_std=mc.GATE_STD)
        imgs = synth.synthetic_images(n, hw[0], hw[1], seed=seed + 500)
        rng = np.random.default_rng(seed + 700)
        cv = (rng.standard_normal((n, cfg["width"])) * 0.05).astype(np.float32)
        with torch.no_grad():
            f64 = tower(cfg, _weights(sd, torch.float64), mc._t64(imgs), mc._t64(cv))
            l32 = tower(cfg, _weights(sd, torch.float32), mc._t64(imgs).float(), mc._t64(cv).float())[3]
        margin, err = mc.margin_figures(f64[3], l32, cfg["top_k"])
        if margin >= mc.MARGIN_RATIO * err:
            break
    else:
        raise AssertionError("no seed with a routing margin for " + name)
    od = cfg["out_dim"]
    seeds = tuple((rng.standard_normal(shape) * 0.1).astype(np.float32) for shape in ((n, cfg["width"]), (n, cfg["width"]), (n, od)))
    return dict(cfg=cfg, hw=hw, seed=seed, sd=sd, imgs=imgs, cv=cv, seeds=seeds, f64=f64, margin=margin, err=err)


@functools.lru_cache(maxsize=None)
def tower_grads(name, use=(True, True, True), coef=AUX_COEF, variant=None, dtype=torch.float64):
    """{reference key name | "cv_emb" | "tokens": gradient} of sum(f_last o d1) + sum(f o d2) + sum(f_proj o d3) + coef * l_aux
    under autograd in `dtype` (seeds with use[i] False are left out); a parameter the function does not reach gets None"""
    c = tower_case(name)
    g = {k: v.clone().requires_grad_(True) for k, v in _weights(c["sd"], dtype).items()}
    cv_t = mc._t64(c["cv"]).to(dtype).requires_grad_(True)
    taps = {}
    out = tower(c["cfg"], g, mc._t64(c["imgs"]).to(dtype), cv_t, taps, variant=variant)
    loss = out[4] * (0.0 if variant == "aux_dropped" else coef)
    for f, d, u in zip(out[:3], c["seeds"], use):
        if u:
            loss = loss + (f * mc._t64(d).to(dtype)).sum()
    loss.backward()
    res = {k: (None if v.grad is None else v.grad.detach()) for k, v in g.items()}
    res["cv_emb"] = cv_t.grad.detach()
    res["tokens"] = taps["tokens"].grad.detach()
    return res


# ----------------------------------------------------------------------------------------------
# the golden: the reference's own MoE VisionTransformer under float64 autograd (tests/golden/make_goldens_moe_grad.py)
# ----------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moe_grad.npz")
GOLDEN_CASES = ("reduced", "reduced_all")
GATE_KEY = "transformer.resblocks.0.gate.weight"
GOLDEN_BOUND = 1e-12   # float64 against float64: vit_grad_cases.GOLDEN_BOUND


def golden_deviations(name, golden=None):
    """{what: relative deviation of this module's restatement from the reference's recorded run} for a golden case: the three
    features, the logits (the reference's flat order l * B + b -> rows), l_aux, every gradient the file holds; a parameter the
    reference's autograd left without .grad must be one that tower_grads leaves at None, and the other way round"""
    z = dict(np.load(GOLDEN)) if golden is None else golden
    c = tower_case(name)
    p = name + "_"
    assert int(z[p + "seed"]) == c["seed"], (name, int(z[p + "seed"]), c["seed"])
    mine, grads = c["f64"], tower_grads(name, coef=0.0)
    aux = tower_grads(name, use=(False, False, False), coef=1.0)
    B = c["imgs"].shape[0]
    L = c["cfg"]["h_res"] * c["cfg"]["w_res"] + 1
    dev = {k: mc.rel_l2(m, z[p + k]) for k, m in zip(("f_last", "f", "f_proj"), mine[:3])}
    dev["logits"] = mc.rel_l2(mine[3], mc.lnd_to_rows(z[p + "logits"], B, L))
    dev["l_aux"] = abs(float(mine[4]) - float(z[p + "l_aux_f64"])) / float(z[p + "l_aux_f64"])
    nograd = set(str(k) for k in z[p + "nograd"])
    assert nograd == {k for k, g in grads.items() if g is None}, (name, sorted(nograd))
    sub = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    for k, g in grads.items():
        if g is None or k == "tokens" or not any(t + k in sub for t in ("g_", "rows_")):   # (the experts' matrices are not stored)
            continue
        if k == GATE_KEY and c["cfg"]["top_k"] == 1:
            # K == 1: w = p / p, the routing gradient is zero in exact arithmetic and both sides hold rounding residue of their
            # own; each is judged against a gradient of the place's scale, that of block 0's ln_2.weight
            scale = np.linalg.norm(sub["g_transformer.resblocks.0.ln_2.weight"])
            dev["d " + k] = max(float(np.linalg.norm(g.numpy())), float(np.linalg.norm(sub["g_" + k]))) / float(scale)
        elif ("norm_" + k in sub and float(sub["norm_" + k]) == 0.0) or ("g_" + k in sub and not sub["g_" + k].any()):
            # an expert no token chose: exactly zero on both sides
            dev["d " + k] = 0.0 if not g.numpy().any() else float("inf")
        else:
            dev["d " + k] = vg.golden_deviation(k, g.numpy(), sub)
    # the load-balancing loss's own gradients: the same parameters reached (nothing behind block 0's ln_2), the same values
    sub = {k[len(p) + 4:]: v for k, v in z.items() if k.startswith(p + "aux_")}
    reached = {k for k, g in aux.items() if g is not None and g.numpy().any() and k != "tokens" and ".experts." not in k}
    assert reached == set(str(k) for k in z[p + "aux_keys"]), (name, sorted(reached))
    for k in reached:
        dev["d_aux " + k] = vg.golden_deviation(k, aux[k].numpy(), sub)
    return dev


# ----------------------------------------------------------------------------------------------
# end to end: the fused stage-2 step on a small MoE tower (the shapes of stage2_train_cases.TRAIN)
# ----------------------------------------------------------------------------------------------
E2E_STEPS = 20
E2E_EK = [(2, 1), (4, 2)]


@functools.lru_cache(maxsize=None)
def e2e_setup(E, K):
    """stage2_train_cases.train_setup with an MoE tower (2 of 3 blocks MoE), its seed walked until the routing margin holds for
    the initial parameters"""
    import stage2_head_cases as hc
    import stage2_train_cases as s2
    c = s2.TRAIN
    cfg = dict(vg.tower_cfg(c["img_hw"]), num_experts=E, top_k=K, moe_layers=2)
    imgs = synth.synthetic_images(c["batch"], c["img_hw"][0], c["img_hw"][1], seed=171)
    for seed in range(7100 + 10 * E, 7100 + 10 * E + 64):
        sd = synth.vit_moe_state_dict(cfg, seed=seed, std=0.05, ln_jitter=0.1, gate_std=mc.GATE_STD)
        with torch.no_grad():
            l64 = tower(cfg, _weights(sd, torch.float64), mc._t64(imgs))[3]
            l32 = tower(cfg, _weights(sd, torch.float32), mc._t64(imgs).float())[3]
        margin, err = mc.margin_figures(l64, l32, K)
        if margin >= mc.MARGIN_RATIO * err:
            break
    head = hc.head_setup(cfg["width"], cfg["out_dim"], batch=c["batch"], per_id=c["per_id"], classes=c["classes"], seed=3)
    return dict(cfg=cfg, sd=sd, imgs=imgs, head=head)


def e2e_trained_names(s):
    """the masters of the MoE tower (no expert, no later gate) and the head's bound three"""
    import stage2_train_cases as s2
    return sorted(k for k in s["sd"] if ".experts." not in k and not (".gate." in k and ".resblocks.0." not in k)) + list(s2.HEAD_BOUND)


@functools.lru_cache(maxsize=None)
def e2e_f64(E, K, steps=E2E_STEPS):
    """stage2_train_cases.train_f64 (SGD) for the MoE tower, the loss = the head's + AUX_COEF * l_aux -> losses [steps],
    aux [steps]"""
    import stage1_cases as sc
    import stage2_head_cases as hc
    import stage2_train_cases as s2
    s, c = e2e_setup(E, K), s2.TRAIN
    cfg, head = s["cfg"], s["head"]
    P = {k: v.clone() for k, v in _weights(s["sd"], torch.float64).items()}
    for k in hc.PARAMS:
        P[k] = mc._t64(head[k]).clone()
    stats = {k + n: mc._t64(head[k + n]).clone() for k in ("bottleneck", "bottleneck_proj") for n in (".running_mean", ".running_var")}
    names = e2e_trained_names(s)
    bufs = {k: np.zeros(tuple(P[k].shape)) for k in names}
    imgs, y, text = mc._t64(s["imgs"]), torch.from_numpy(head["target"]), mc._t64(head["text"])
    losses, auxes = [], []
    for step in range(1, steps + 1):
        g = {k: v.clone().requires_grad_(k in names) for k, v in P.items()}
        f_last, f, f_proj, _, l_aux = tower(cfg, g, imgs)
        t = dict(g, f_last=f_last, f=f, f_proj=f_proj, target=y, text=text, **stats)
        new_stats = {}
        loss = hc.head_loss_torch(t, "uniprompt", 0.1, hc.MARGIN, 1.0, 1.0, 1.0, True, new_stats)[0] + AUX_COEF * l_aux
        grads = torch.autograd.grad(loss, [g[k] for k in names])
        losses.append(float(loss.detach()))
        auxes.append(float(l_aux.detach()))
        for k, gr in zip(names, grads):
            fac, wd = s2.group_of(k)
            p, bufs[k] = s2.sgd_f64(P[k].numpy(), gr.numpy(), bufs[k], step, sc.f32(sc.f32(c["sgd_lr"]) * fac), sc.f32(c["sgd_mu"]),
                                    sc.f32(wd))
            P[k] = torch.from_numpy(np.ascontiguousarray(p))
        stats.update({k: v.detach() for k, v in new_stats.items() if k in stats})
    return dict(losses=np.asarray(losses), aux=np.asarray(auxes))
