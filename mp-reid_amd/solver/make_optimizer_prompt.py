"""Drop-in for the stage-1 part of the reference's ``solver/make_optimizer_prompt.py``:
``make_optimizer_1stage(cfg, model, stage_name)`` with stage_name 'STAGE1A' / 'STAGE1B' (a section of ``cfg.SOLVER``).

One parameter group per trainable tensor with the section's BASE_LR and WEIGHT_DECAY, as in the reference.  The trainable
tensors are the context tensors of ``model.prompt_learner`` that require grad (``enable_stage1a_training()`` /
``enable_stage1b_training()`` mark them; they are not registered parameters of the model here), else the model's own parameters
that require grad.  OPTIMIZER_NAME 'Adam' (L2 weight decay added to the gradient, betas 0.9 / 0.999, eps 1e-8: torch's
defaults) and 'AdamW' give ``mpreid.ops.PromptAdam``, whose step is the library's Adam kernel and which
``processor_uniprompt_stage1.do_train_stage1`` drives through the fused ``PromptTrainer``.  'SGD', any other name and AdamW with
``AMSGRAD`` fall through to ``torch.optim`` (the autograd path of the loop).  The stage-2 and LoRA optimizers of the reference
belong to training stages this build does not have.
"""
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
