"""Seeded inputs and float64 restatements of the stage-2 training tests (test_gpu_stage2_train.py on the GPU,
test_stage2_train_cpu.py on the host): the multi-tensor optimizer step, the per-tensor largest finite entry, the batched re-pack
and the fused training step on the reduced tower.  tests/golden/stage2_train.npz holds what the reference's own WarmupMultiStepLR
and make_optimizer_2astage / make_optimizer_2bstage give (tests/golden/make_goldens_stage2_train.py)."""
import functools
import os

import numpy as np
import torch

import stage1_cases as sc
import stage2_head_cases as hc
import text_cases as tc
import vit_grad_cases as vg
from mpreid import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage2_train.npz")
BOUND = vg.BOUND                          # 2e-5: the project's split-mode bar

# ----------------------------------------------------------------------------------------------
# the optimizer table
# ----------------------------------------------------------------------------------------------
CHUNK = 4096                              # MPREID_OPTIM_CHUNK
#: one element, around the 16-byte group, below the workgroup, above 1024, exactly one work chunk, one chunk + 1, three chunks + 7
OPT_SIZES = (1, 3, 4, 5, 255, 1025, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
OPT_MISALIGNED_SIZES = (5, 1025, CHUNK + 1)
OPT_STEPS = (1, 2, 1000)
SGD_WD = (0.0, 5e-4)
SGD_LR, SGD_MU = 0.01, 0.9
#: eight (lr, weight_decay) classes: the reference's three (weights, biases, large-FC) and five more to fill the table
CLASSES8 = [(3e-4, 5e-4), (6e-4, 0.0), (6e-4, 5e-4), (1e-3, 1e-2), (0.0, 5e-4), (3e-5, 0.0), (1e-2, 1e-4), (7e-4, 3e-3)]


def opt_state(n, seed):
    """fp32 (p, grad, exp_avg | momentum buffer, exp_avg_sq) of n elements"""
    return sc.adam_state(n, seed, False)


def sgd_f64(p, g, buf, step, lr, mu, wd):
    """one step of torch.optim.SGD(momentum=mu, dampening=0, nesterov=False) in float64 -> (p, buf)"""
    p, g, buf = (np.asarray(t, np.float64) for t in (p, g, buf))
    g = g + wd * p
    buf = g if step == 1 else mu * buf + g
    return p - lr * buf, buf


def sgd_lines(p, g, buf, step, lr, mu, wd):
    """the three lines of the kernel, each computed in float64 from fp32 operands and rounded ONCE MORE to fp32 (not always what
    fmaf gives: the double result is itself rounded) -> float64 arrays of fp32 values (p, buf)"""
    r = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
    p, g, buf = r(p), r(g), r(buf)
    lr, mu, wd = (float(np.float32(x)) for x in (lr, mu, wd))
    g = r(wd * p + g)
    buf = g if step == 1 else r(mu * buf + g)
    return r(p - lr * buf), buf


# ----------------------------------------------------------------------------------------------
# the largest finite entry
# ----------------------------------------------------------------------------------------------
ABSMAX_SHAPES = ((1,), (63,), (64,), (65,), (4097,), (768, 3072))


def absmax_input(shape, seed=0):
    rng = np.random.default_rng(8100 + int(np.prod(shape)) + seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)


def absmax_torch(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs().max()


# ----------------------------------------------------------------------------------------------
# the fused training step on the reduced tower
# ----------------------------------------------------------------------------------------------
TRAIN = dict(img_hw=(64, 32), batch=8, per_id=2, classes=7, cv_rows=5, sie_coe=3.0, steps=10, wd=5e-4, bias_lr_factor=2.0,
             adam_lr=3e-4, sgd_lr=0.002, sgd_mu=0.9)
HEAD_BOUND = ("classifier.weight", "bottleneck.weight", "bottleneck.bias")
NEVER_BOUND = ("classifier_proj.weight", "bottleneck_proj.weight", "bottleneck_proj.bias")


@functools.lru_cache(maxsize=None)
def train_setup():
    """dict: cfg, tower state dict, images fp32 [8, 3, 64, 32], the head's setup (stage2_head_cases.head_setup at the tower's
    widths: target = 4 identities of 2 among 7 classes, text, parameters, running statistics), cv_table fp32 [5, 128], cv_index"""
    c = TRAIN
    cfg = vg.tower_cfg(c["img_hw"])
    sd = synth.vit_state_dict(cfg, seed=71, ln_jitter=0.1)
    imgs = synth.synthetic_images(c["batch"], c["img_hw"][0], c["img_hw"][1], seed=171)
    head = hc.head_setup(cfg["width"], cfg["out_dim"], batch=c["batch"], per_id=c["per_id"], classes=c["classes"], seed=3)
    rng = np.random.default_rng(271)
    cv_table = (rng.standard_normal((c["cv_rows"], cfg["width"])) * 0.02).astype(np.float32)
    cv_index = np.array([0, 3, 3, 1, 4, 0, 3, 1], dtype=np.int64)     # row 2 is never used: its gradient is exactly 0
    return dict(cfg=cfg, sd=sd, imgs=imgs, head=head, cv_table=cv_table, cv_index=cv_index)


def group_of(name):
    """(lr factor, weight decay) of a trained tensor by the reference's rule: "bias" in its name"""
    return (TRAIN["bias_lr_factor"], 0.0) if "bias" in name else (1.0, TRAIN["wd"])


def trained_names(sie):
    s = train_setup()
    return sorted(s["sd"]) + list(HEAD_BOUND) + (["cv_embed"] if sie else [])


@functools.lru_cache(maxsize=None)
def train_f64(sie, algo, steps):
    """the loop in float64 under torch autograd: vit_grad_cases.tower, stage2_head_cases.head_loss_torch in the Uni-Prompt form,
    bottleneck_proj in training mode beside it, then stage1_cases.adam_f64 / sgd_f64 per trained tensor with the
    hyper-parameters as the C ABI receives them -> dict(losses [steps] (total, before each update), grads: name -> the
    gradient of step 1, params: name -> value after the last step, stats: the running statistics after the last step)"""
    s, c = train_setup(), TRAIN
    cfg, head = s["cfg"], s["head"]
    P = {k: v.clone() for k, v in vg.weights(s["sd"]).items()}
    for k in hc.PARAMS:
        P[k] = tc._t64(head[k]).clone()
    if sie:
        P["cv_embed"] = tc._t64(s["cv_table"]).clone()
    stats = {k + n: tc._t64(head[k + n]).clone() for k in ("bottleneck", "bottleneck_proj") for n in (".running_mean", ".running_var")}
    names = trained_names(sie)
    state = {k: (np.zeros(tuple(P[k].shape)), np.zeros(tuple(P[k].shape))) for k in names}
    imgs, y, text = tc._t64(s["imgs"]), torch.from_numpy(head["target"]), tc._t64(head["text"])
    idx = torch.from_numpy(s["cv_index"])
    base_lr = sc.f32(c["adam_lr"] if algo != "SGD" else c["sgd_lr"])
    losses, first = [], None
    for step in range(1, steps + 1):
        g = {k: v.clone().requires_grad_(k in names) for k, v in P.items()}
        cv = c["sie_coe"] * g["cv_embed"][idx] if sie else None
        f_last, f, f_proj = vg.tower(cfg, g, imgs, cv)
        t = dict(g, f_last=f_last, f=f, f_proj=f_proj, target=y, text=text, **stats)
        new_stats = {}
        loss = hc.head_loss_torch(t, "uniprompt", 0.1, hc.MARGIN, 1.0, 1.0, 1.0, True, new_stats)[0]
        rm, rv = stats["bottleneck_proj.running_mean"].clone(), stats["bottleneck_proj.running_var"].clone()
        torch.nn.functional.batch_norm(f_proj.detach(), rm, rv, P["bottleneck_proj.weight"], P["bottleneck_proj.bias"], True,
                                       hc.BN_MOMENTUM, hc.BN_EPS)
        new_stats.update({"bottleneck_proj.running_mean": rm, "bottleneck_proj.running_var": rv})
        grads = torch.autograd.grad(loss, [g[k] for k in names])
        losses.append(float(loss.detach()))
        if first is None:
            first = {k: gr.detach().numpy().copy() for k, gr in zip(names, grads)}
        for k, gr in zip(names, grads):
            fac, wd = group_of(k)
            lr, wd = sc.f32(base_lr * fac), sc.f32(wd)
            if algo == "SGD":
                p, buf = sgd_f64(P[k].numpy(), gr.numpy(), state[k][0], step, lr, sc.f32(c["sgd_mu"]), wd)
                state[k] = (buf, None)
            else:
                p, m, v = sc.adam_f64(P[k].numpy(), gr.numpy(), state[k][0], state[k][1], step, lr, sc.f32(sc.BETA1), sc.f32(sc.BETA2),
                                      sc.f32(sc.EPS), wd, algo == "AdamW")
                state[k] = (m, v)
            P[k] = torch.from_numpy(np.ascontiguousarray(p))
        stats.update({k: v.detach() for k, v in new_stats.items()})
    return dict(losses=np.asarray(losses), grads=first, params={k: P[k].numpy() for k in P}, stats={k: v.numpy() for k, v in stats.items()})


# ----------------------------------------------------------------------------------------------
# the schedule and the parameter selection (golden: the reference's own classes)
# ----------------------------------------------------------------------------------------------
#: name -> (milestones, gamma, warmup_factor, warmup_iters, warmup_method); base lr 3e-4; epochs 1 .. 100 via scheduler.step(epoch)
SCHEDULES = {"default": ((40, 70), 0.1, 0.01, 500, "linear"), "constant": ((40, 70), 0.1, 0.01, 500, "constant"),
             "warmup0": ((40, 70), 0.1, 0.01, 0, "linear"), "warmup10": ((40, 70), 0.1, 0.01, 10, "linear")}
SCHEDULE_BASE_LR = 3e-4
SCHEDULE_EPOCHS = 100
#: name -> (stage function, BIAS_LR_FACTOR, LARGE_FC_LR)
SELECTIONS = {"2a": ("2a", 2, False), "2a_large_fc": ("2a", 2, True), "2b": ("2b", 2, False), "2b_large_fc": ("2b", 2, True)}


def schedule_f64(epoch, base_lr, milestones, gamma, warmup_factor, warmup_iters, warmup_method):
    """the reference's WarmupMultiStepLR.get_lr at last_epoch = epoch, in its order of operations"""
    from bisect import bisect_right
    f = 1
    if epoch < warmup_iters:
        if warmup_method == "constant":
            f = warmup_factor
        else:
            alpha = epoch / warmup_iters
            f = warmup_factor * (1 - alpha) + alpha
    return base_lr * f * gamma ** bisect_right(list(milestones), epoch)


def standin_names(layers=2, experts=2):
    """this project's parameter names (a dense ViT model of `layers` blocks with the SIE table and the Uni-Prompt extras, plus
    the MoE and text names the filters look for), in named_parameters order of the stand-in module"""
    names = []
    for top in ("class_embedding", "positional_embedding", "proj", "conv1.weight", "ln_pre.weight", "ln_pre.bias"):
        names.append("image_encoder." + top)
    for i in range(layers):
        b = f"image_encoder.transformer.resblocks.{i}."
        names += [b + k for k in ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                                  "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                                  "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")]
        names += [b + f"experts.{e}.{k}" for e in range(experts) for k in ("c_fc.weight", "c_fc.bias", "c_proj.weight", "c_proj.bias")]
        names.append(b + "gate.weight")
    names += ["image_encoder.ln_post.weight", "image_encoder.ln_post.bias"]
    names += ["classifier.weight", "classifier_proj.weight", "bottleneck.weight", "bottleneck.bias", "bottleneck_proj.weight",
              "bottleneck_proj.bias", "cv_embed", "visual_prompt", "text_encoder.ln_final.weight", "text_encoder.ln_final.bias",
              "prompt_learner.ctx_generic"]
    return names


def standin_module(names=None):
    """an nn.Module whose named_parameters() yields `names` in order with 1-element tensors, all requiring grad"""
    import torch.nn as nn
    root = nn.Module()
    for dotted in names or standin_names():
        parts, mod = dotted.split("."), root
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        mod.register_parameter(parts[-1], nn.Parameter(torch.zeros(1)))
    return root


def stage2a_requires_grad(model):
    """what the reference's train_uniprompt.py:137-154 does before make_optimizer_2astage"""
    for name, p in model.named_parameters():
        p.requires_grad = not ("text_encoder" in name or "expert" in name or "prompt_learner" in name)


SELECTION_WD_BIAS = 1e-4            # unlike WEIGHT_DECAY, so that the rule shows
SELECTION_SOLVER_BASE_LR = 1e-3     # the key LARGE_FC_LR reads (absent from the defaults)


def selection_cfg(bias_lr_factor, large_fc):
    """the project's default config with the selection's settings (attribute access is all the reference's functions need)"""
    from config import cfg_base
    c = cfg_base.clone()
    c.defrost()
    c.SOLVER.STAGE2.update(BIAS_LR_FACTOR=bias_lr_factor, WEIGHT_DECAY_BIAS=SELECTION_WD_BIAS, LARGE_FC_LR=large_fc)
    if large_fc:
        c.SOLVER.BASE_LR = SELECTION_SOLVER_BASE_LR
    return c


def run_selection(fn_2a, fn_2b, name):
    """(names, lrs, weight decays) of the optimizer's groups, and the names left requiring grad, for one of SELECTIONS"""
    import torch.nn as nn
    stage, factor, large_fc = SELECTIONS[name]
    model = standin_module()
    if stage == "2a":
        stage2a_requires_grad(model)
    center = nn.Module()
    center.register_parameter("centers", nn.Parameter(torch.zeros(1)))
    opt, opt_center = (fn_2a if stage == "2a" else fn_2b)(selection_cfg(factor, large_fc), model, center)
    by_id = {id(p): n for n, p in model.named_parameters()}
    groups = [(by_id[id(g["params"][0])], float(g["lr"]), float(g["weight_decay"])) for g in opt.param_groups]
    assert len(opt_center.param_groups) == 1 and opt_center.param_groups[0]["params"][0] is center.centers
    return ([g[0] for g in groups], np.array([g[1] for g in groups]), np.array([g[2] for g in groups]),
            [n for n, p in model.named_parameters() if p.requires_grad], float(opt_center.param_groups[0]["lr"]))
