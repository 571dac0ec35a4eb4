"""Seeded inputs and float64 restatements of the stage-2 head tests (test_gpu_stage2_head.py on the GPU, test_stage2_head_cpu.py
on the host): row cross-entropy with label smoothing, the batch-hard triplet loss, BatchNorm1d in training mode, the linear
products and the whole head under torch autograd.  tests/golden/stage2_head.npz holds what the reference's own
CrossEntropyLabelSmooth and TripletLoss (float64, autograd) give for the GOLDEN_* cases below
(tests/golden/make_goldens_stage2_head.py); test_stage2_head_cpu.py holds the restatements to them."""
import functools
import os

import numpy as np

import stage1_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage2_head.npz")
BOUND = sc.BOUND                          # 2e-5: relative error of a loss, relative L2 of a gradient
rel_l2 = sc.rel_l2
MARGIN = 0.3                              # SOLVER.MARGIN
EPSILONS = (0.0, 0.1)

# ----------------------------------------------------------------------------------------------
# row cross-entropy
# ----------------------------------------------------------------------------------------------
XENT_ROWS = (1, 2, 63, 64, 65, 257)
XENT_CLASSES = (1, 2, 63, 64, 65, 255, 256, 257, 751, 1025)   # around the wave, the workgroup and its second round; the data set
XENT_SCALE, XENT_SCALE_HOT = 3.0, 40.0    # the hot scale at 64 classes only: a logit above OVERFLOW_LOGIT
OVERFLOW_LOGIT = sc.OVERFLOW_LOGIT


def xent_cases():
    """(rows, classes, epsilon, logit scale) of every cross-entropy case"""
    out = [(r, c, e, XENT_SCALE) for r in XENT_ROWS for c in XENT_CLASSES for e in EPSILONS]
    return out + [(r, 64, e, XENT_SCALE_HOT) for r in XENT_ROWS for e in EPSILONS]


GOLDEN_XENT = [(r, c, e, XENT_SCALE) for r in (2, 65) for c in (1, 2, 65, 257) for e in EPSILONS] + [(64, 751, 0.1, XENT_SCALE)]


def xent_key(case):
    return "r%d_c%d_e%s_s%g" % (case[0], case[1], ("%g" % case[2]).replace(".", "p"), case[3])


@functools.lru_cache(maxsize=None)
def xent_case(rows, classes, epsilon, scale):
    """(logits fp32 [rows, classes] ~ N(0, scale^2), labels int64 [rows]); epsilon is not part of the seed.  At the hot scale the
    seed advances until the largest logit exceeds OVERFLOW_LOGIT: found within a few draws, asserted."""
    base = 2000003 * rows + 1013 * classes + int(scale)
    for attempt in range(256):
        rng = np.random.default_rng(base + 7919 * attempt)
        logits = (rng.standard_normal((rows, classes)) * scale).astype(np.float32)
        labels = rng.integers(0, classes, rows).astype(np.int64)
        if scale != XENT_SCALE_HOT or float(logits.max()) > OVERFLOW_LOGIT:
            return logits, labels
    raise AssertionError("no draw with a logit above %g" % OVERFLOW_LOGIT)


def xent_f64(logits, labels, epsilon, scale=1.0):
    """float64: (loss, d_logits) of loss = -(scale / rows) sum_a sum_c t_ac logp_ac, t_ac = (1 - epsilon) [c == y_a] + epsilon / K"""
    s = np.asarray(logits, np.float64)
    rows, K = s.shape
    m = s.max(1, keepdims=True)
    lp = s - m - np.log(np.exp(s - m).sum(1, keepdims=True))
    t = np.full((rows, K), epsilon / K)
    t[np.arange(rows), np.asarray(labels)] += 1 - epsilon
    return -scale * (t * lp).sum() / rows, scale * (np.exp(lp) - t) / rows


@functools.lru_cache(maxsize=None)
def xent_want(rows, classes, epsilon, scale, loss_scale):
    logits, labels = xent_case(rows, classes, epsilon, scale)
    return xent_f64(logits, labels, epsilon, loss_scale)


def xent_torch(logits, labels, epsilon, scale, dtype):
    """the same loss through torch autograd on the host in `dtype` -> (loss, d_logits) as float64 numpy"""
    import torch
    x = torch.from_numpy(np.asarray(logits)).to(dtype).requires_grad_(True)
    lp = torch.log_softmax(x, 1)
    t = torch.zeros_like(lp).scatter_(1, torch.from_numpy(np.asarray(labels)).unsqueeze(1), 1) * (1 - epsilon) + epsilon / x.shape[1]
    loss = scale * (-t * lp).sum(1).mean()
    (g,) = torch.autograd.grad(loss, [x])
    return float(loss.detach()), g.double().numpy()


# ----------------------------------------------------------------------------------------------
# batch-hard triplet loss
# ----------------------------------------------------------------------------------------------
TRIPLET_GROUPS = ("2x1", "2x2", "16x4", "13x5", "4x16", "ragged63", "ragged65", "ragged257", "equal5")
TRIPLET_DIMS = (4, 5, 64, 512, 768)
TRIPLET_FORMS = (MARGIN, None)            # the margin form and the soft-margin form
FEAT_SCALE = 0.6


def triplet_cases():
    return [(g, d, m) for g in TRIPLET_GROUPS for d in TRIPLET_DIMS for m in TRIPLET_FORMS]


#: the reference answers equal group sizes only
GOLDEN_TRIPLET = [(g, d, m) for g in ("2x1", "2x2", "16x4", "13x5", "4x16") for d in (4, 5, 64) for m in TRIPLET_FORMS] + \
                 [("16x4", 768, MARGIN), ("16x4", 768, None)]


def triplet_key(case):
    return "%s_d%d_%s" % (case[0], case[1], "soft" if case[2] is None else "m%g" % case[2])


def group_labels(groups, rng):
    """int64 labels of a group pattern, shuffled: 'PxK' = P identities of K rows, 'raggedB' = groups of sizes 1, 2, 3, ... cut at
    B rows, 'equalB' = B rows of one identity (no negatives at all)"""
    if groups.startswith("ragged"):
        batch = int(groups[6:])
        lab = np.concatenate([np.full(k + 1, 3 * k - 4, dtype=np.int64) for k in range(batch)])[:batch]
    elif groups.startswith("equal"):
        lab = np.full(int(groups[5:]), 5, dtype=np.int64)
    else:
        p, k = (int(v) for v in groups.split("x"))
        lab = np.repeat(np.arange(p, dtype=np.int64) * 7 - 3, k)
    return rng.permutation(lab)


def pair_d2(x):
    """float64 [B, B] squared distances as sums of squared differences, row by row (no [B, B, D] array)"""
    x = np.asarray(x, np.float64)
    return np.stack([((x[a] - x) ** 2).sum(-1) for a in range(len(x))])


def triplet_f64(x, y, margin, p=None, n=None):
    """x [B, D], y int labels [B]; margin None = the soft-margin form.  p / n: mined indices to use instead of float64's own.
    -> (loss, d_x, dist_ap, dist_an, p, n, d [B, B]); an anchor without negatives has n = -1, dist_an = inf and no term"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y)
    B = len(y)
    d2 = pair_d2(x)
    d = np.sqrt(np.maximum(d2, 1e-12))
    pos = y[:, None] == y[None, :]
    has_n = (~pos).any(1)
    if p is None:
        p = np.where(pos, d, -np.inf).argmax(1)          # hardest positive / negative, lowest index on ties
        n = np.where(~pos, d, np.inf).argmin(1)
        n = np.where(has_n, n, -1)
    p, n = np.asarray(p, np.int64), np.asarray(n, np.int64)
    ar = np.arange(B)
    dap = d[ar, p]
    dan = np.where(has_n, d[ar, np.maximum(n, 0)], np.inf)
    with np.errstate(over="ignore"):
        if margin is None:
            z = dap - dan
            per, w = np.logaddexp(0, z), 1 / (1 + np.exp(-z))
        else:
            z = dap - dan + margin
            per, w = np.maximum(z, 0), (z > 0).astype(np.float64)
    per, w = np.where(has_n, per, 0.0), np.where(has_n, w, 0.0)
    g = np.zeros_like(x)
    for a in range(B):
        if not has_n[a]:
            continue
        if d2[a, p[a]] >= 1e-12:                          # a pair below the clamp gives no gradient
            u = (x[a] - x[p[a]]) / dap[a] * w[a] / B
            g[a] += u
            g[p[a]] -= u
        if d2[a, n[a]] >= 1e-12:
            u = (x[a] - x[n[a]]) / dan[a] * w[a] / B
            g[a] -= u
            g[n[a]] += u
    return per.mean(), g, dap, dan, p, n, d


def margin_premise(x, y, margin):
    """the smallest of |ap - an + margin| / (4 (ap + an) D 2^-23) over the anchors that have a negative (inf when none has): at
    1 or above, fp32 distances with the chain's worst-case error leave every hinge on its side"""
    _, _, dap, dan, _, n, _ = triplet_f64(x, y, margin)
    k = n >= 0
    if not k.any():
        return float("inf")
    D = np.asarray(x).shape[1]
    return float(np.min(np.abs(dap[k] - dan[k] + margin) / (4 * (dap[k] + dan[k]) * D * 2.0 ** -23)))


@functools.lru_cache(maxsize=None)
def triplet_case(groups, dim, margin):
    """(features fp32 [B, dim] ~ N(0, 0.6^2), labels int64 [B]).  In the margin form the seed advances until margin_premise >= 1
    (asserted to happen within 256 draws); no case is dropped."""
    base = 3000017 * TRIPLET_GROUPS.index(groups) + 1019 * dim
    for attempt in range(256):
        rng = np.random.default_rng(base + 7919 * attempt)
        y = group_labels(groups, rng)
        x = (rng.standard_normal((len(y), dim)) * FEAT_SCALE).astype(np.float32)
        if margin is None or margin_premise(x, y, margin) >= 1.0:
            return x, y
    raise AssertionError("no draw that keeps every hinge away from its corner")


@functools.lru_cache(maxsize=None)
def triplet_want(groups, dim, margin):
    return triplet_f64(*triplet_case(groups, dim, margin), margin)


def triplet_tie_case(groups):
    """small-integer features at D = 4: every squared distance is an exact small integer in fp32 as in float64, with many ties"""
    rng = np.random.default_rng(41 + TRIPLET_GROUPS.index(groups))
    y = group_labels(groups, rng)
    return rng.integers(-2, 3, (len(y), 4)).astype(np.float32), y


def triplet_torch(x, y, margin, dtype):
    """the loss through torch autograd on the host in `dtype`, distances as sums of squared differences -> (loss, d_x) float64"""
    import torch
    X = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    loss = triplet_loss_torch(X, torch.from_numpy(np.asarray(y)), margin)
    if not loss.requires_grad:
        return float(loss), np.zeros(X.shape)
    (g,) = torch.autograd.grad(loss, [X])
    return float(loss.detach()), g.double().numpy()


def triplet_loss_torch(X, y, margin):
    import torch
    d = torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").clamp(min=1e-6)   # (no [B, B, D] tensor)
    pos = y[:, None] == y[None, :]
    inf = torch.full_like(d, float("inf"))
    ap, an = torch.where(pos, d, -inf).max(1)[0], torch.where(pos, inf, d).min(1)[0]
    z = ap - an
    return torch.relu(z + margin).mean() if margin is not None else torch.nn.functional.softplus(z).mean()


# ----------------------------------------------------------------------------------------------
# BatchNorm1d in training mode
# ----------------------------------------------------------------------------------------------
BN_BATCHES = (2, 3, 64, 65)
BN_DIMS = (1, 5, 512, 768)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def bn_case(batch, dim):
    """(x, dy fp32 [batch, dim], gamma, beta, running_mean, running_var fp32 [dim]); the last column of x holds one value, 1.5"""
    rng = np.random.default_rng(4000037 * batch + dim)
    x = (rng.standard_normal((batch, dim)) * 0.8 + 0.3).astype(np.float32)
    x[:, -1] = 1.5
    dy = rng.standard_normal((batch, dim)).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(dim)).astype(np.float32)
    rm = (0.5 * rng.standard_normal(dim)).astype(np.float32)
    rv = (0.5 + rng.random(dim)).astype(np.float32)
    return x, dy, gamma, beta, rm, rv


def bn_f64(x, dy, gamma, beta, rm, rv, eps=BN_EPS, momentum=BN_MOMENTUM):
    """float64 -> dict(y, mean, invstd, running_mean, running_var, dx, dgamma, dbeta)"""
    x, dy, gamma, beta, rm, rv = (np.asarray(t, np.float64) for t in (x, dy, gamma, beta, rm, rv))
    B = x.shape[0]
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    inv = 1 / np.sqrt(var + eps)
    xh = (x - mu) * inv
    return dict(y=xh * gamma + beta, mean=mu, invstd=inv, running_mean=(1 - momentum) * rm + momentum * mu,
                running_var=(1 - momentum) * rv + momentum * var * B / (B - 1),
                dx=(gamma * inv / B) * (B * dy - dy.sum(0) - xh * (dy * xh).sum(0)), dgamma=(dy * xh).sum(0), dbeta=dy.sum(0))


# ----------------------------------------------------------------------------------------------
# the linear products
# ----------------------------------------------------------------------------------------------
LINEAR_SIZES = ((64, 768, 751), (3, 5, 2))      # (batch, width, classes)


@functools.lru_cache(maxsize=None)
def linear_case(batch, width, classes):
    rng = np.random.default_rng(5000011 * batch + 31 * width + classes)
    return (rng.standard_normal((batch, width)).astype(np.float32), (rng.standard_normal((classes, width)) * 0.05).astype(np.float32),
            (rng.standard_normal((batch, classes)) * 0.01).astype(np.float32))


# ----------------------------------------------------------------------------------------------
# the restatement of the appendix: identity loss behind a training-mode BNNeck and a bias-free classifier
# ----------------------------------------------------------------------------------------------
def head_f64(f, gamma, beta, W, y, eps_ls, eps_bn=BN_EPS):
    """f [B, D], gamma / beta [D], W [C, D], y int labels [B] -> (loss, dW, dgamma, df, batch mean, biased variance)"""
    f, gamma, beta, W = (np.asarray(t, np.float64) for t in (f, gamma, beta, W))
    B, C = f.shape[0], W.shape[0]
    mu = f.mean(0)
    var = ((f - mu) ** 2).mean(0)
    inv = 1 / np.sqrt(var + eps_bn)
    xh = (f - mu) * inv
    yb = xh * gamma + beta
    loss, dS = xent_f64(yb @ W.T, y, eps_ls)
    dW, dy = dS.T @ yb, dS @ W
    dgamma = (dy * xh).sum(0)
    df = (gamma * inv / B) * (B * dy - dy.sum(0) - xh * (dy * xh).sum(0))
    return loss, dW, dgamma, df, mu, var


# ----------------------------------------------------------------------------------------------
# the whole head
# ----------------------------------------------------------------------------------------------
HEAD_WIDTHS = ((768, 512), (128, 64))
HEAD_B, HEAD_P, HEAD_K, HEAD_C = 64, 16, 4, 751
HEAD_WEIGHTS = dict(id_weight=0.25, triplet_weight=1.0, i2t_weight=0.5)
PARAMS = ("classifier.weight", "classifier_proj.weight", "bottleneck.weight", "bottleneck.bias", "bottleneck_proj.weight",
          "bottleneck_proj.bias")


@functools.lru_cache(maxsize=None)
def head_setup(width, width_proj, batch=HEAD_B, per_id=HEAD_K, classes=HEAD_C, seed=0, cluster=0.0):
    """dict of fp32 numpy arrays: f_last, f, f_proj, target, text, the six parameters and the four running statistics.
    cluster > 0: the features of an identity are its centre plus N(0, cluster^2) noise (the run that learns)"""
    rng = np.random.default_rng(6000001 + 13 * width + width_proj + 101 * seed)
    ids = batch // per_id
    target = rng.permutation(np.repeat(rng.choice(classes, ids, replace=False).astype(np.int64), per_id))
    out = {"target": target}
    for name, n in (("f_last", width), ("f", width), ("f_proj", width_proj)):
        if cluster:
            centres = rng.standard_normal((classes, n))
            out[name] = (centres[target] + cluster * rng.standard_normal((batch, n))).astype(np.float32)
        else:
            out[name] = (rng.standard_normal((batch, n)) * FEAT_SCALE).astype(np.float32)
    out["text"] = (rng.standard_normal((classes, width_proj)) * 0.3).astype(np.float32)
    out["classifier.weight"] = (rng.standard_normal((classes, width)) * 0.05).astype(np.float32)
    out["classifier_proj.weight"] = (rng.standard_normal((classes, width_proj)) * 0.05).astype(np.float32)
    for name, n in (("bottleneck", width), ("bottleneck_proj", width_proj)):
        out[name + ".weight"] = (1 + 0.2 * rng.standard_normal(n)).astype(np.float32)
        out[name + ".bias"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        out[name + ".running_mean"] = (0.5 * rng.standard_normal(n)).astype(np.float32)
        out[name + ".running_var"] = (0.5 + rng.random(n)).astype(np.float32)
    return out


def head_loss_torch(t, form, epsilon, margin, id_weight, triplet_weight, i2t_weight, with_text=True, stats=None):
    """the head's loss in torch from a dict of tensors (features, parameters, text, target) of one dtype: BatchNorm in training
    mode (running statistics, when `stats` is a dict, are updated into it), the classifiers, the smoothed cross-entropy written
    out, triplet_loss_torch -> (total, identity part, triplet part, image-to-text part), the parts with their weights"""
    import torch
    y = t["target"]

    def xent(s):
        lp = torch.log_softmax(s, 1)
        tt = torch.zeros_like(lp).scatter_(1, y.unsqueeze(1), 1) * (1 - epsilon) + epsilon / s.shape[1]
        return (-tt * lp).sum(1).mean()

    def branch(f, name, cls):
        rm = rv = None
        if stats is not None:
            rm, rv = t[name + ".running_mean"].clone(), t[name + ".running_var"].clone()
            stats[name + ".running_mean"], stats[name + ".running_var"] = rm, rv
        yb = torch.nn.functional.batch_norm(f, rm, rv, t[name + ".weight"], t[name + ".bias"], True, BN_MOMENTUM, BN_EPS)
        return yb @ t[cls + ".weight"].T
    zero = torch.zeros((), dtype=t["f"].dtype)
    if form == "uniprompt":
        idl = xent(branch(t["f"], "bottleneck", "classifier"))
        tri = triplet_loss_torch(t["f"], y, margin)
    else:
        idl = xent(branch(t["f"], "bottleneck", "classifier")) + xent(branch(t["f_proj"], "bottleneck_proj", "classifier_proj"))
        tri = sum(triplet_loss_torch(t[k], y, margin) for k in ("f_last", "f", "f_proj"))
    i2t = xent(t["f_proj"] @ t["text"].T) if with_text else zero
    idl, tri, i2t = id_weight * idl, triplet_weight * tri, i2t_weight * i2t
    return i2t + (idl + tri), idl, tri, i2t


GRAD_KEYS = ("f_last", "f", "f_proj") + PARAMS


def head_host(setup, form, dtype, epsilon=0.1, margin=MARGIN, with_text=True, **weights):
    """the head under torch autograd on the host in `dtype` -> (losses float64 [4], dict of gradients (exact zeros where the form
    does not use a tensor) and updated running statistics, float64 numpy)"""
    import torch
    w = dict(HEAD_WEIGHTS, **weights)
    t = {k: torch.from_numpy(v) if v.dtype == np.int64 else torch.from_numpy(v).to(dtype) for k, v in setup.items()}
    for k in GRAD_KEYS:
        t[k].requires_grad_(True)
    stats = {}
    losses = head_loss_torch(t, form, epsilon, margin, w["id_weight"], w["triplet_weight"], w["i2t_weight"], with_text, stats)
    grads = torch.autograd.grad(losses[0], [t[k] for k in GRAD_KEYS], allow_unused=True)
    out = {k: (np.zeros(tuple(t[k].shape)) if g is None else g.double().numpy()) for k, g in zip(GRAD_KEYS, grads)}
    for k in ("bottleneck", "bottleneck_proj"):
        for s in (".running_mean", ".running_var"):
            out[k + s] = (stats[k + s] if k + s in stats else t[k + s]).double().numpy()
    return np.array([float(v.detach()) for v in losses]), out


# ----------------------------------------------------------------------------------------------
# "it learns": 40 steps on fixed features, the head's own parameters updated with Adam
# ----------------------------------------------------------------------------------------------
LEARN = dict(identities=6, per_id=8, steps=40, lr=5e-3, width=128, width_proj=64, cluster=0.1)


@functools.lru_cache(maxsize=None)
def learn_setup():
    c = LEARN
    return head_setup(c["width"], c["width_proj"], batch=c["identities"] * c["per_id"], per_id=c["per_id"], classes=c["identities"],
                      seed=9, cluster=c["cluster"])


def learn_curve_host(dtype):
    """the loss before each of the 40 steps in `dtype` on the host: the list form without text features under autograd,
    torch.optim.Adam (foreach=False, no weight decay) on the six head parameters -> float64 [steps]"""
    import torch
    s = learn_setup()
    t = {k: torch.from_numpy(v) if v.dtype == np.int64 else torch.from_numpy(v).to(dtype) for k, v in s.items()}
    for k in PARAMS:
        t[k].requires_grad_(True)
    opt = torch.optim.Adam([t[k] for k in PARAMS], lr=sc.f32(LEARN["lr"]), betas=(sc.f32(sc.BETA1), sc.f32(sc.BETA2)), eps=sc.f32(sc.EPS),
                           foreach=False)
    curve = []
    for _ in range(LEARN["steps"]):
        opt.zero_grad()
        stats = {}
        loss = head_loss_torch(t, "list", 0.1, MARGIN, 1.0, 1.0, 1.0, False, stats)[0]
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k, v in stats.items():
                t[k] = v
        curve.append(float(loss.detach()))
    return np.asarray(curve, np.float64)
