"""Drop-in for the stage-1 part of the reference's ``solver/make_optimizer_prompt.py``:
``make_optimizer_1stage(cfg, model, stage_name)`` with stage_name 'STAGE1A' / 'STAGE1B' (a section of ``cfg.SOLVER``).

One parameter group per trainable tensor with the section's BASE_LR and WEIGHT_DECAY, as in the reference.  The trainable
tensors are the context tensors of ``model.prompt_learner`` that require grad (``enable_stage1a_training()`` /
``enable_stage1b_training()`` mark them; they are not registered parameters of the model here), else the model's own parameters
that require grad.  OPTIMIZER_NAME 'Adam' (L2 weight decay added to the gradient, betas 0.9 / 0.999, eps 1e-8: torch's
defaults) and 'AdamW' give ``mpreid.ops.PromptAdam``, whose step is the library's Adam kernel and which
``processor_uniprompt_stage1.do_train_stage1`` drives through the fused ``PromptTrainer``.  'SGD', any other name and AdamW with
``AMSGRAD`` fall through to ``torch.optim`` (the autograd path of the loop).

Stage 2: ``make_optimizer_2astage(cfg, model, center_criterion)`` and ``make_optimizer_2bstage(...)`` -> ``(optimizer,
optimizer_center)``, selected by the reference's rules.  2a takes every parameter that requires grad (``train_uniprompt.py``
has set that: everything but ``text_encoder``, ``expert`` and ``prompt_learner`` names; here
``model.enable_stage2_training()``), dropping ``text_encoder`` and ``expert`` names again; 2b sets ``requires_grad`` itself: the
``gate`` names and the ``image_encoder`` names without ``experts``, nothing else.  One group per tensor with
SOLVER.STAGE2.BASE_LR / WEIGHT_DECAY; a name containing ``bias`` gets BASE_LR * BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS; in 2a
with LARGE_FC_LR a name containing ``classifier`` or ``arcface`` gets ``cfg.SOLVER.BASE_LR * 2`` -- the reference reads
SOLVER.BASE_LR there, not SOLVER.STAGE2.BASE_LR, a key its defaults do not have: the quirk is kept, and without the key the
call raises as the reference's does.  OPTIMIZER_NAME 'Adam', 'AdamW' and 'SGD' (with MOMENTUM) over fp32 device tensors give
``mpreid.ops.TensorOptimizer``, whose step is one multi-tensor kernel call and which ``do_train_stage2`` drives through the fused
``Stage2Trainer``; anything else (another name, parameters still on the host) gives ``torch.optim`` and the autograd path.
``optimizer_center`` is ``torch.optim.SGD`` over the centers with CENTER_LR: built and passed along, never stepped (the
reference's loss_func never calls center_criterion).  The LoRA optimizer of the reference belongs to a stage this build does not
have.
"""
import logging

import torch

from mpreid import ops as _ops


def make_optimizer_1stage(cfg, model, stage_name):
    stage_cfg = getattr(cfg.SOLVER, stage_name)
    learner = getattr(model, "prompt_learner", None)
    if learner is not None and hasattr(learner, "parameters"):
        tensors = [p for p in learner.parameters() if p is not None and p.requires_grad]
    else:
        tensors = [p for _, p in model.named_parameters() if p.requires_grad]
    if not tensors:
        raise ValueError("make_optimizer_1stage: no trainable tensor; call model.enable_stage1a_training() or "
                         "enable_stage1b_training() first")
    params = [{"params": [p], "lr": stage_cfg.BASE_LR, "weight_decay": stage_cfg.WEIGHT_DECAY} for p in tensors]
    name = stage_cfg.OPTIMIZER_NAME
    amsgrad = bool(stage_cfg.get("AMSGRAD", False))
    ours = all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in tensors)
    if name == 'SGD':
        return torch.optim.SGD(params, momentum=stage_cfg.MOMENTUM)
    if name == 'AdamW' and ours and not amsgrad:
        return _ops.PromptAdam(params, decoupled=True)     # (every group carries its own lr and weight_decay)
    if name == 'AdamW':
        return torch.optim.AdamW(params, amsgrad=amsgrad)
    if name == 'Adam' and ours:
        return _ops.PromptAdam(params)
    return getattr(torch.optim, name)(params)


def _stage2_optimizer(cfg, params, stage):
    logger = logging.getLogger("transreid.train")
    s2 = cfg.SOLVER.STAGE2
    if not params:
        logger.warning("no trainable parameter found for the stage %s optimizer", stage)
    name = s2.OPTIMIZER_NAME
    tensors = [g["params"][0] for g in params]
    ours = bool(tensors) and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in tensors)
    if name in ("SGD", "Adam", "AdamW") and ours:
        return _ops.TensorOptimizer(params, name, lr=s2.BASE_LR, weight_decay=s2.WEIGHT_DECAY, momentum=s2.MOMENTUM)
    if name == 'SGD':
        return torch.optim.SGD(params, momentum=s2.MOMENTUM)
    if name == 'AdamW':
        return torch.optim.AdamW(params, lr=s2.BASE_LR, weight_decay=s2.WEIGHT_DECAY)
    return getattr(torch.optim, name)(params)


def _stage2_group(cfg, key, value, large_fc):
    s2 = cfg.SOLVER.STAGE2
    lr, weight_decay = s2.BASE_LR, s2.WEIGHT_DECAY
    if "bias" in key:
        lr, weight_decay = s2.BASE_LR * s2.BIAS_LR_FACTOR, s2.WEIGHT_DECAY_BIAS
    if large_fc and ("classifier" in key or "arcface" in key):
        lr = cfg.SOLVER.BASE_LR * 2          # (SOLVER.BASE_LR, as the reference reads it; absent from its defaults)
    logging.getLogger("transreid.train").info(f"  [Trainable] {key} (Size: {tuple(value.shape)}, LR: {lr:.2e}, WD: {weight_decay:.2e})")
    return {"params": [value], "lr": lr, "weight_decay": weight_decay}


def _stage2_summary(stage, params, total):
    n = sum(g["params"][0].numel() for g in params)
    logging.getLogger("transreid.train").info(
        f"stage {stage} optimizer: {len(params)} parameter groups, {n} / {total} parameters trained ({n / max(total, 1):.2%})")


def make_optimizer_2astage(cfg, model, center_criterion):
    params, total = [], 0
    for key, value in model.named_parameters():
        total += value.numel()
        if not value.requires_grad:
            continue
        if "text_encoder" in key or "expert" in key:
            value.requires_grad_(False)
            continue
        params.append(_stage2_group(cfg, key, value, cfg.SOLVER.STAGE2.LARGE_FC_LR))
    _stage2_summary("2a", params, total)
    optimizer = _stage2_optimizer(cfg, params, "2a")
    return optimizer, torch.optim.SGD(center_criterion.parameters(), lr=cfg.SOLVER.STAGE2.CENTER_LR)


def make_optimizer_2bstage(cfg, model, center_criterion):
    params, total = [], 0
    for key, value in model.named_parameters():
        total += value.numel()
        if "gate" in key or ("image_encoder" in key and "experts" not in key):
            value.requires_grad_(True)
        else:
            value.requires_grad_(False)
            continue
        params.append(_stage2_group(cfg, key, value, False))
    _stage2_summary("2b", params, total)
    optimizer = _stage2_optimizer(cfg, params, "2b")
    return optimizer, torch.optim.SGD(center_criterion.parameters(), lr=cfg.SOLVER.STAGE2.CENTER_LR)
