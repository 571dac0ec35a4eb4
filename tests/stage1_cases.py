"""Seeded inputs and float64 restatements of the stage-1 prompt-learning tests (test_gpu_stage1.py on the GPU,
test_stage1_cpu.py on the host): the symmetric supervised contrastive loss with its gradients, the context gradient as a
segment sum, both forms of the Adam step and the one-cycle cosine schedule.  tests/golden/stage1.npz holds what the
reference's own SupConLoss (float64, autograd) and scheduler give for GOLDEN_SUPCON and the schedules below
(tests/golden/make_goldens_stage1.py); test_stage1_cpu.py holds the restatements to them."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage1.npz")

BATCHES = (1, 2, 3, 63, 64, 65, 257)     # one, the smallest, odd, both sides of the wave and of the 16-row tile, five waves
DIMS = (4, 64, 512)
PATTERNS = ("distinct", "equal", "groups")
SCALE, SCALE_HOT = 0.6, 3.0              # the hot scale at dim 64 only: logits beyond +-100
OVERFLOW_LOGIT = 89.0                    # exp(x) overflows fp32 above 88.73
BOUND = 2e-5                             # relative L2 of a gradient, relative error of a loss: the project's split-mode bar


def supcon_cases():
    """(batch, dim, label pattern, feature scale) of every loss case"""
    out = [(b, d, p, SCALE) for b in BATCHES for d in DIMS for p in PATTERNS]
    return out + [(b, 64, p, SCALE_HOT) for b in BATCHES for p in PATTERNS]


#: the cases whose float64 reference results are stored (a committed file stays far below 1 MiB): every case at dim 4, and the
#: unequal groups at dim 64 (both scales) and 512 around the tile edge
GOLDEN_SUPCON = ([c for c in supcon_cases() if c[1] == 4] +
                 [(b, 64, "groups", s) for b in (2, 5, 64, 65) for s in (SCALE, SCALE_HOT)] + [(3, 512, "groups", SCALE)])


def case_key(case):
    return "b%d_d%d_%s_s%s" % (case[0], case[1], case[2], ("%g" % case[3]).replace(".", "p"))


def make_labels(pattern, batch, rng):
    """int64 [batch]: all distinct (arbitrary values, a negative one among them), all equal, or groups of sizes 1, 2, 3, ...
    (the last one cut) in a shuffled order"""
    if pattern == "distinct":
        return (rng.permutation(batch).astype(np.int64) * 7 - 3)
    if pattern == "equal":
        return np.full(batch, 5, dtype=np.int64)
    lab = np.concatenate([np.full(k + 1, k, dtype=np.int64) for k in range(batch)])[:batch]
    return rng.permutation(lab)


@functools.lru_cache(maxsize=None)
def supcon_case(batch, dim, pattern, scale):
    """(img, txt fp32 [batch, dim] ~ N(0, scale^2), labels int64 [batch]).  At the hot scale the seed advances until the largest
    logit exceeds OVERFLOW_LOGIT (an unstabilised fp32 exp would overflow): found within a few draws, asserted."""
    base = 1000003 * batch + 1009 * dim + 17 * PATTERNS.index(pattern) + int(scale * 10)
    for attempt in range(256):
        rng = np.random.default_rng(base + 7919 * attempt)
        img = (rng.standard_normal((batch, dim)) * scale).astype(np.float32)
        txt = (rng.standard_normal((batch, dim)) * scale).astype(np.float32)
        labels = make_labels(pattern, batch, rng)
        if scale != SCALE_HOT or float((img.astype(np.float64) @ txt.astype(np.float64).T).max()) > OVERFLOW_LOGIT:
            return img, txt, labels
    raise AssertionError("no draw with a logit above %g" % OVERFLOW_LOGIT)


def _lse(s, axis):
    m = s.max(axis=axis, keepdims=True)
    return m + np.log(np.exp(s - m).sum(axis=axis, keepdims=True))


def supcon_f64(img, txt, labels):
    """float64: (loss [2] = loss_i2t, loss_t2i; d_txt, d_img [batch, dim]: the gradients of loss_i2t + loss_t2i)
    S = img txt^T, M_ab = (y_a == y_b), n_a = sum_b M_ab, P = softmax over rows, Q = softmax over columns,
    loss = -(1/B) sum_a (1/n_a) sum_b M_ab (log P_ab + log Q_ba),  dL/dS_ab = -(1/B) ((M_ab/n_a - P_ab) + (M_ab/n_b - Q_ab))"""
    I, T = np.asarray(img, np.float64), np.asarray(txt, np.float64)
    y = np.asarray(labels)
    B = I.shape[0]
    S = I @ T.T
    M = (y[:, None] == y[None, :]).astype(np.float64)
    n = M.sum(1)
    logp, logq = S - _lse(S, 1), S - _lse(S, 0)
    loss = np.array([-((M * logp).sum(1) / n).mean(), -((M * logq).sum(0) / n).mean()])
    G = -((M / n[:, None] - np.exp(logp)) + (M / n[None, :] - np.exp(logq))) / B
    return loss, G.T @ I, G @ T


@functools.lru_cache(maxsize=None)
def supcon_want(batch, dim, pattern, scale):
    """the float64 results of a case, computed once and shared"""
    return supcon_f64(*supcon_case(batch, dim, pattern, scale))


def supcon_torch(img, txt, labels, dtype):
    """the same loss through torch autograd on the host in `dtype` (log_softmax): (loss [2], d_txt, d_img) as float64 numpy"""
    import torch
    I = torch.from_numpy(np.asarray(img)).to(dtype).requires_grad_(True)
    T = torch.from_numpy(np.asarray(txt)).to(dtype).requires_grad_(True)
    y = torch.from_numpy(np.asarray(labels))
    M = (y[:, None] == y[None, :]).to(dtype)
    S = I @ T.T
    l1 = -((M * torch.log_softmax(S, 1)).sum(1) / M.sum(1)).mean()
    l2 = -((M * torch.log_softmax(S, 0)).sum(0) / M.sum(0)).mean()
    dT, dI = torch.autograd.grad(l1 + l2, [T, I])
    return (np.array([float(l1.detach()), float(l2.detach())]), dT.double().numpy(), dI.double().numpy())


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = float(np.linalg.norm(want))
    return float(np.linalg.norm(got - want)) / d if d else float(np.linalg.norm(got - want))


# ----------------------------------------------------------------------------------------------
# the segment sum
# ----------------------------------------------------------------------------------------------
def segment_sum_f32(src, idx, tok0, n_tok, n_seg):
    """out[s][t][e] = sum over b ascending with idx[b] == s of src[b][tok0 + t][e]: sequential fp32 additions from 0.0"""
    src = np.asarray(src, np.float32)
    out = np.zeros((n_seg, n_tok, src.shape[2]), np.float32)
    for b, s in enumerate(np.asarray(idx).tolist()):
        if 0 <= s < n_seg:
            out[s] = out[s] + src[b, tok0:tok0 + n_tok]
    return out


#: (name, batch, tokens, width, tok0, n_tok, n_seg, idx): one and seven prompts, a full batch, eight equal indices in a row, an
#: empty segment, the two-segment form of the modality / platform contexts, both widths, a window at either end of the prompt
def segment_cases():
    rng = np.random.default_rng(77)
    c = [("one", 1, 21, 128, 1, 8, 3, [1]),
         ("seven", 7, 21, 128, 1, 8, 6, [5, 0, 3, 3, 0, 5, 3]),                        # segments 1, 2 and 4 stay empty
         ("run_of_eight", 12, 21, 128, 9, 4, 4, [2, 1, 1, 1, 1, 1, 1, 1, 1, 0, 3, 2]),
         ("batch64", 64, 21, 128, 1, 8, 40, rng.integers(0, 40, 64).tolist()),
         ("two_segments", 64, 21, 128, 13, 4, 2, rng.integers(0, 2, 64).tolist()),
         ("all_in_one_of_two", 7, 21, 128, 9, 4, 2, [1] * 7),                          # segment 0 empty
         ("clip_generic", 64, 77, 512, 1, 8, 50, rng.integers(0, 50, 64).tolist()),
         ("clip_platform", 7, 77, 512, 13, 4, 2, [0, 1, 1, 0, 1, 1, 1]),
         ("front_window", 7, 21, 128, 0, 3, 3, [0, 1, 2, 0, 1, 2, 0]),
         ("back_window", 7, 21, 128, 18, 3, 3, [2, 2, 1, 1, 0, 0, 2]),
         ("whole_prompt", 3, 5, 128, 0, 5, 2, [1, 0, 1]),
         ("odd_width", 7, 6, 5, 1, 3, 3, [0, 2, 2, 0, 1, 2, 0])]                       # the one-element-per-thread path
    return c


def segment_src(batch, tokens, width, seed=0):
    rng = np.random.default_rng(5000 + 100 * batch + tokens + width + seed)
    return rng.standard_normal((batch, tokens, width)).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# Adam / AdamW
# ----------------------------------------------------------------------------------------------
ADAM_N = (1, 3, 255, 257, 8 * 512 * 6)
ADAM_STEPS = (1, 2, 1000)
ADAM_WD = (0.0, 5e-4)
LR, BETA1, BETA2, EPS = 3e-4, 0.9, 0.999, 1e-8


def f32(x):
    """a hyperparameter as the C ABI receives it: rounded to fp32, as a Python float"""
    return float(np.float32(x))


def adam_f64(p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled):
    """one step of torch.optim.Adam (decoupled False) / AdamW (True) in float64 -> (p, m, v); the hyperparameters as given"""
    p, g, m, v = (np.asarray(t, np.float64) for t in (p, g, m, v))
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - lr / (1.0 - beta1 ** step) * (m / (np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps))
    return p, m, v


def adam_state(n, seed, same_sign):
    """fp32 (p ~ N(0, 0.02), grad ~ N(0, 1e-3), exp_avg, exp_avg_sq > 0) of n elements.  same_sign: exp_avg carries the sign of
    the gradient, so that no term of the first-moment update cancels and a count of roundings bounds the error of the result"""
    rng = np.random.default_rng(31000 + n + seed)
    p = (rng.standard_normal(n) * 0.02).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    m = (rng.standard_normal(n) * 5e-4).astype(np.float32)
    if same_sign:
        m = (np.abs(m) * np.where(g < 0, -1.0, 1.0)).astype(np.float32)
    v = ((rng.standard_normal(n) * 1e-3) ** 2 + 1e-9).astype(np.float32)
    return p, g, m, v


def ulp32(x):
    """the spacing of fp32 at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------
# the schedule
# ----------------------------------------------------------------------------------------------
SCHEDULE = dict(base_lr=3e-4, num_epochs=100, lr_min=0.000016, warmup_lr_init=0.01, warmup_t=5)   # SOLVER.STAGE1A defaults


def schedule_f64(epoch, base_lr, num_epochs, lr_min, warmup_lr_init, warmup_t):
    """the learning rate the reference's scheduler sets at scheduler.step(epoch): linear from warmup_lr_init towards base_lr over
    warmup_t epochs, then one cosine cycle from base_lr to lr_min over num_epochs (counted from epoch 0), lr_min from then on"""
    if epoch < warmup_t:
        return warmup_lr_init + epoch * ((base_lr - warmup_lr_init) / warmup_t)
    if epoch >= num_epochs:
        return lr_min
    return lr_min + 0.5 * (base_lr - lr_min) * (1 + math.cos(math.pi * epoch / num_epochs))


# ----------------------------------------------------------------------------------------------
# "it learns": 40 steps of stage 1a on a reduced tower towards a hidden teacher
# ----------------------------------------------------------------------------------------------
LEARN = dict(identities=6, per_id=8, steps=40, lr=2e-3, weight_decay=5e-4, noise=0.05, eot=19)


@functools.lru_cache(maxsize=None)
def learn_setup():
    """(cfg, tower state dict, the student's prompt tensors, image features fp32 [48, out_dim], labels int64 [48]): each image
    feature is the float64 text feature of its identity under a hidden teacher ctx_generic plus N(0, (noise * feature std)^2)"""
    import text_cases as tc
    from mpreid import synth
    cfg = tc.REDUCED
    sd = synth.text_state_dict(cfg, seed=51)
    student = tc.prompt_learner_tensors(LEARN["identities"], seed=52, tokens=cfg["tokens"], dim=cfg["width"])
    teacher = dict(student, ctx_generic=tc.prompt_learner_tensors(LEARN["identities"], seed=53, tokens=cfg["tokens"],
                                                                    dim=cfg["width"])["ctx_generic"])
    rng = np.random.default_rng(54)
    labels = rng.permutation(np.repeat(np.arange(LEARN["identities"], dtype=np.int64), LEARN["per_id"]))
    feats = tc.tower_f64(cfg, sd, tc.assemble_prompts(teacher, labels, "1a"), [LEARN["eot"]] * len(labels)).numpy()
    img = feats + LEARN["noise"] * feats.std() * rng.standard_normal(feats.shape)
    return cfg, sd, student, img.astype(np.float32), labels


def learn_curve_host(dtype):
    """the loss before each of the 40 steps of the loop on the host in `dtype`: text_grad_cases.tower and the symmetric loss
    under autograd, torch.optim.Adam (foreach=False) with the hyperparameters as the C ABI receives them -> float64 [steps]"""
    import torch
    import text_cases as tc
    import text_grad_cases as tg
    cfg, sd, student, img, labels = learn_setup()
    w = tg.weights(sd, dtype)
    t = {k: v.to(dtype) for k, v in student.items()}
    t["ctx_generic"].requires_grad_(True)
    opt = torch.optim.Adam([t["ctx_generic"]], lr=f32(LEARN["lr"]), betas=(f32(BETA1), f32(BETA2)), eps=f32(EPS),
                           weight_decay=f32(LEARN["weight_decay"]), foreach=False)
    I, y = torch.from_numpy(img).to(dtype), torch.from_numpy(labels)
    curve = []
    for _ in range(LEARN["steps"]):
        opt.zero_grad()
        feats = tg.tower(cfg, w, tc.assemble_prompts(t, y, "1a"), [LEARN["eot"]] * len(labels))
        loss = tg.symmetric_loss(I, feats, y)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return np.asarray(curve, np.float64)


def curve_deviation(curve, want):
    """the largest relative deviation of a loss curve from the float64 curve"""
    return float(np.max(np.abs(np.asarray(curve, np.float64) - want) / np.abs(want)))
