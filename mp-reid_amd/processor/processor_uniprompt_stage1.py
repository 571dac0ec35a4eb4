"""Drop-in for the reference's ``processor/processor_uniprompt_stage1.py``: ``do_train_stage1(cfg, model,
train_loader_stage1, optimizer, scheduler, local_rank, is_stage1b=False)`` -- stage 1a (the generic context vectors) and
stage 1b (the modality and platform context vectors) of Uni-Prompt's prompt learning, every tower weight frozen.

The loop is the reference's (:11-120).  Every training image is encoded once with ``model(x=img, get_image=True)`` under
``no_grad``; features, labels and views stay on the device.  Each epoch calls ``scheduler.step(epoch)`` and draws
``torch.randperm(num_image)``; each batch of ``SOLVER.STAGE1.IMS_PER_BATCH`` takes one step on
``loss_i2t + loss_t2i`` (loss/supcontrast.py, both directions) of the batch's text features -- the identity prompts of its
labels, with ``view=None`` in stage 1a and the batch's views in stage 1b -- against its fixed image features.  Every
``CHECKPOINT_PERIOD`` epochs ``MODEL.NAME + '_stage1a_{epoch}.pth'`` (``1b``) is written to ``OUTPUT_DIR``: it holds
``model.text_state_dict()``, the text tower and the prompt tensors under the reference's key names, which ``load_param`` reads
back (the image tower is frozen in this stage: its checkpoint is the one the model was loaded from).

With the optimizer of ``solver/make_optimizer_prompt.py`` (``mpreid.ops.PromptAdam``) a step is ``mpreid.ops.PromptTrainer.step``:
prompt assembly, text forward, the loss pair with its gradient, text backward, the context gradients and the Adam update, all
enqueued without waiting for the device; the loss values are read back at the log lines and at the end of an epoch only.  With
any other optimizer (``torch.optim``) a step is the autograd path: ``get_text`` under autograd, ``SupConLoss`` twice,
``backward()``, ``optimizer.step()``.  The model stays in ``.eval()`` (neither branch has a mode-dependent layer).

Two behaviours of the reference are not reproduced:
  * autocast and ``GradScaler``: the text features and their gradient are fp32-grade here and the backward never passes through
    fp16, so there is nothing to scale;
  * the empty last batch: the reference runs ``num_image // batch + 1`` batches, the last of which is empty when the batch size
    divides the number of images, and its loss is NaN.  An empty batch is skipped here (``stage1_batches``); the log line's batch
    count is the number of batches that run.
"""
import logging
import os
import time
from datetime import timedelta

import torch

from loss.supcontrast import SupConLoss
from mpreid import ops as _ops
from utils.meter import AverageMeter


def stage1_batches(num_image, batch):
    """the (start, stop) slices of a permutation of num_image indices, `batch` at a time; the last one may be short, none is empty"""
    if batch <= 0:
        raise ValueError("SOLVER.STAGE1.IMS_PER_BATCH must be positive")
    return [(s, min(s + batch, num_image)) for s in range(0, num_image, batch)]


def _encode_images(model, loader, device):
    feats, labels, views = [], [], []
    with torch.no_grad():
        for img, vid, _target_cam, target_view in loader:
            feats.append(model(x=img.to(device), get_image=True).float())
            labels.append(torch.as_tensor(vid).to(device).long())
            views.append(torch.as_tensor(target_view).to(device).long())
    return torch.cat(feats).contiguous(), torch.cat(labels), torch.cat(views)


def _fused_trainer(model, optimizer, stage):
    """the PromptTrainer of this model and optimizer, or None when the step has to go through autograd"""
    if not isinstance(optimizer, _ops.PromptAdam) or not hasattr(model, "text_tower") or not hasattr(model, "prompt_learner"):
        return None
    enc = model.text_tower()
    return _ops.PromptTrainer(enc, model.prompt_learner, stage, optimizer=optimizer, eot=model._eot_rows)


def do_train_stage1(cfg, model, train_loader_stage1, optimizer, scheduler, local_rank, is_stage1b=False):
    checkpoint_period = cfg.SOLVER.STAGE1.CHECKPOINT_PERIOD
    device = "cuda"
    epochs = cfg.SOLVER.STAGE1.MAX_EPOCHS
    log_period = cfg.SOLVER.STAGE1.LOG_PERIOD
    stage = '1b' if is_stage1b else '1a'

    logger = logging.getLogger("transreid.train")
    logger.info(f"Start training stage {stage}")
    model.to(device)
    model.eval()
    loss_meter = AverageMeter()
    xent = SupConLoss(device)
    all_start_time = time.monotonic()

    image_features_list, labels_list, views_list = _encode_images(model, train_loader_stage1, device)
    batch = cfg.SOLVER.STAGE1.IMS_PER_BATCH
    num_image = labels_list.shape[0]
    num_class = getattr(model, "num_classes", None)
    if num_image and num_class is not None and (int(labels_list.min()) < 0 or int(labels_list.max()) >= num_class):
        raise ValueError(f"stage 1: labels outside 0 .. {num_class - 1}")      # checked once: the steps do not look again
    slices = stage1_batches(num_image, batch)
    trainer = _fused_trainer(model, optimizer, stage)
    logger.info("stage {}: {} images, {} batches per epoch, {} step".format(
        stage, num_image, len(slices), "fused (mpreid.ops.PromptTrainer)" if trainer is not None else "autograd"))

    for epoch in range(1, epochs + 1):
        loss_meter.reset()
        pending = []     # (device scalar, batch size) of the steps whose loss has not been read back yet
        if scheduler is not None:
            scheduler.step(epoch)
        iter_list = torch.randperm(num_image).to(device)
        for i, (lo, hi) in enumerate(slices):
            b_list = iter_list[lo:hi]
            target = labels_list[b_list]
            target_view_batch = views_list[b_list]
            image_features = image_features_list[b_list]
            if trainer is not None:
                loss = trainer.step(image_features, target, views=target_view_batch if is_stage1b else None).sum()
            else:
                optimizer.zero_grad()
                text_features = model(label=target, get_text=True, view=target_view_batch if is_stage1b else None)
                loss = xent(image_features, text_features, target, target) + xent(text_features, image_features, target, target)
                loss.backward()
                optimizer.step()
                loss = loss.detach()
            pending.append((loss, hi - lo))
            if (i + 1) % log_period == 0 or i + 1 == len(slices):
                for value, n in pending:
                    loss_meter.update(float(value), n)
                pending = []
            if (i + 1) % log_period == 0:
                lr = scheduler._get_lr(epoch)[0] if scheduler is not None else optimizer.param_groups[0]['lr']
                logger.info("Epoch[{}] Iteration[{}/{}] Loss: {:.3f}, Base Lr: {:.2e}"
                            .format(epoch, (i + 1), len(slices), loss_meter.avg, lr))

        if epoch % checkpoint_period == 0:
            rank0 = not (cfg.MODEL.DIST_TRAIN and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0
            if rank0:
                state = model.text_state_dict() if hasattr(model, "text_state_dict") else model.state_dict()
                torch.save(state, os.path.join(cfg.OUTPUT_DIR, cfg.MODEL.NAME + f'_stage{stage}_{epoch}.pth'))

    total_time = timedelta(seconds=time.monotonic() - all_start_time)
    logger.info(f"Stage {stage} running time: {total_time}")
