"""Drop-in for the reference's ``processor/processor_uniprompt_stage2.py``:

  do_train_stage2(cfg, model, center_criterion, train_loader_stage2, val_loader, optimizer, optimizer_center, scheduler,
                  loss_fn, num_query, local_rank, max_epochs, log_period, checkpoint_period, eval_period)   reference :14-223
  do_inference(cfg, model, val_loader, num_query)                 reference :225-266
  do_inference_ttpt_option_a(cfg, model, val_loader, num_query)   reference :530-693  (TTA "option A")

Same loops, log lines and return values.  In option A every QUERY batch is encoded four times (original, W-flip,
pseudo-IR = channel mean, pseudo-RGB = channel 0 replicated), the four features are averaged and L2-normalised
(:598-640); gallery batches are encoded once and normalised (:649-654).  Here the views are produced inside the
patch-gather kernel (no transformed image tensors) and the average + normalise is one kernel
(mpreid_tta_mean_f32).  Quirks kept: whether a batch is "query" is decided by the number of samples processed
BEFORE it (:594), so a batch straddling num_query is augmented as a whole; TEST.FEAT_NORM is a truthy string.

``do_inference_ttpt_clipstyle`` (option B) matches images against text features of the prompt learner and
optimises prompts at test time.  The text tower and its prompt gradient exist (model(label=..., get_text=True) after
model.enable_stage1a_training()), but the reference's branch reads prompt_learner.cls_ctx and num_class, which its own
PromptLearner does not have: there is no reference behaviour to reproduce -> NotImplementedError.

``do_train_stage2`` is the reference's loop: the text features of all identities once (``get_text`` in batches of
SOLVER.STAGE2.IMS_PER_BATCH labels, no grad), then per epoch ``scheduler.step(epoch)``, ``model.train()`` and one step per batch
on ``loss_fn(score, feat, target, target_cam, image_features_proj @ text_features.t())``; the reference's log lines; every
``checkpoint_period`` epochs ``OUTPUT_DIR/EXP_SETTING/NAME_{epoch}.pth`` (the module's ``state_dict()`` plus
``text_state_dict()``, which ``load_param`` reads back); every ``eval_period`` epochs the validation with the evaluator.  The model
must have had ``enable_stage2_training()`` (the optimizers of solver/make_optimizer_prompt.py are built over its device
parameters); a model that has not is enabled here, its ``requires_grad`` flags kept.  With a ``mpreid.ops.TensorOptimizer`` a
batch is ONE ``mpreid.ops.Stage2Trainer.step`` -- forward, head, backward, the multi-tensor optimizer step and the re-pack, no
autograd graph -- and the loss and accuracy are read back only at the log lines and at the epoch's end.  With any other
optimizer a batch takes the autograd path through the training-mode forward and ``loss_fn``.  Not reproduced:
  * autocast and ``GradScaler``: features, loss and gradients are fp32-grade throughout, there is nothing to scale;
  * ``nn.DataParallel`` over several GPUs: one device;
  * the center-loss branch: the reference's ``loss_func`` never calls ``center_criterion``, its loop touches the centers only
    when ``'center' in MODEL.METRIC_LOSS_TYPE``, a configuration ``make_loss`` cannot answer -- ``optimizer_center`` is built,
    passed along, zeroed and never stepped.  The same holds here;
  * the reference's loop over the rows of the tower's fourth output: its own MoE stage 2 cannot run (its model wrapper unpacks
    three values from a four-value tower).  Here the load-balancing term is the documented contract of
    ``load_balancing_loss_func``: ONE layer of logits [L * B, E], coefficient 0.01.
The labels and the SIE rows address tables on the device: each batch's are range-checked on the host before they are copied
(no wait for the device).
"""
import logging
import os
import time

import torch

from mpreid import ops as _ops
from processor.processor import (ENCODE_GROUP, SAME_CAM_NOTE, configure_extra_metrics, configure_query_expansion,
                                 grouped_batches, merge_batches, report_extra_metrics)
from utils.metrics import R1_mAP_eval


def do_inference(cfg, model, val_loader, num_query):
    device = "cuda"
    logger = logging.getLogger("transreid.test")
    logger.info("Enter inferencing")

    evaluator = R1_mAP_eval(num_query, max_rank=50, feat_norm=cfg.TEST.FEAT_NORM)
    evaluator.remove_same_cam = bool(getattr(cfg.TEST, "REMOVE_SAME_CAM", False))   # not a reference key (config/node.py)
    if evaluator.remove_same_cam:
        logger.info(SAME_CAM_NOTE)
    evaluator.rank_list_k = int(getattr(cfg.TEST, "RANK_LIST_K", 0) or 0)   # not a reference key: evaluator.last_rank_lists
    configure_query_expansion(cfg, evaluator)   # TEST.QE_K / QE_ALPHA / QE_TIMES, not reference keys
    configure_extra_metrics(cfg, evaluator)     # TEST.EXTRA_METRICS / ROC_FPRS / PAIR_HIST_BINS / PAIR_HIST_RANGE, likewise
    evaluator.reset()

    model.to(device)
    model.eval()
    img_path_list = []
    for group in grouped_batches(val_loader, ENCODE_GROUP):   # see processor/processor.py: same features, fuller GPU
        with torch.no_grad():
            img, camids, target_view = merge_batches(group, device)
            camids = camids if cfg.MODEL.SIE_CAMERA else None
            target_view = target_view if cfg.MODEL.SIE_VIEW else None
            feat = model(x=img, cam_label=camids, view_label=target_view)
            lo = 0
            for (_, pid, camid, _, _, imgpath) in group:
                evaluator.update((feat[lo:lo + len(pid)], pid, camid))
                img_path_list.extend(imgpath)
                lo += len(pid)

    cmc, mAP, distmat, pids, camids, qf, gf = evaluator.compute()
    logger.info("Validation Results ")
    logger.info("mAP: {:.1%}".format(mAP))
    report_extra_metrics(cfg, logger, evaluator)
    for r in [1, 5, 10]:
        logger.info("CMC curve, Rank-{:<3}:{:.1%}".format(r, cmc[r - 1]))
    return cmc[0], cmc[4]


def do_inference_ttpt_clipstyle(cfg, model, val_loader, num_query):
    raise NotImplementedError("TTA + TTPT with CLIP-style image-text matching (option B) tunes prompt_learner.cls_ctx over num_class "
                              "prompts, which the reference's own PromptLearner does not have: there is no reference behaviour to "
                              "reproduce.  The pieces exist (model(label=..., get_text=True) is differentiable with respect to the "
                              "context vectors after model.enable_stage1a_training()); only option A (image features) is on the "
                              "accelerated path")


def do_inference_ttpt_option_a(cfg, model, val_loader, num_query):
    device = "cuda"
    logger = logging.getLogger("transreid.test_ttpt_option_a")
    logger.info("Enter inferencing with TTA only (Option A - Image Feature Evaluation)")

    tta_enabled = cfg.TEST.get('TTA_ENABLED', True)
    feat_norm = cfg.TEST.FEAT_NORM
    if tta_enabled:
        logger.info("Test Time Augmentation (TTA) enabled.")
    logger.info("TTPT optimization part is disabled for this run.")

    model.to(device)
    evaluator = R1_mAP_eval(num_query, max_rank=50, feat_norm=cfg.TEST.FEAT_NORM)
    evaluator.remove_same_cam = bool(getattr(cfg.TEST, "REMOVE_SAME_CAM", False))   # not a reference key (config/node.py)
    if evaluator.remove_same_cam:
        logger.info(SAME_CAM_NOTE)
    evaluator.rank_list_k = int(getattr(cfg.TEST, "RANK_LIST_K", 0) or 0)   # not a reference key: evaluator.last_rank_lists
    configure_query_expansion(cfg, evaluator)   # TEST.QE_K / QE_ALPHA / QE_TIMES, not reference keys
    configure_extra_metrics(cfg, evaluator)     # TEST.EXTRA_METRICS / ROC_FPRS / PAIR_HIST_BINS / PAIR_HIST_RANGE, likewise
    evaluator.reset()
    model.eval()

    logger.info("Starting feature extraction...")
    start_time = time.time()
    processed_samples = 0
    views = (_ops.VIEW_ORIGINAL, _ops.VIEW_FLIP, _ops.VIEW_PSEUDO_IR, _ops.VIEW_PSEUDO_RGB) if tta_enabled else \
        (_ops.VIEW_ORIGINAL,)

    def tagged():
        """loader batches tagged query / gallery by the reference's rule (:594: decided by the number of samples
        processed BEFORE the batch), consecutive batches of one kind grouped up to ENCODE_GROUP images"""
        seen, kind, group, n = 0, None, [], 0
        for batch in val_loader:
            k = seen < num_query
            if group and (k != kind or n >= ENCODE_GROUP):
                yield kind, group
                group, n = [], 0
            kind = k
            group.append(batch)
            n += len(batch[1])
            seen += len(batch[1])
        if group:
            yield kind, group

    for is_query, group in tagged():
        img, cam, vw = merge_batches(group, device)
        cam = cam if cfg.MODEL.SIE_CAMERA else None
        vw = vw if cfg.MODEL.SIE_VIEW else None
        with torch.no_grad():
            if is_query:
                if isinstance(img, (list, tuple)):      # decoded images: resize once, then the views
                    img = _ops.resize_bilinear_u8(img, model.img_hw)
                feats = torch.stack([model(x=img, cam_label=cam, view_label=vw, tta_view=v) for v in views], dim=0)
                feat = _ops.tta_mean(feats, normalize=bool(feat_norm))
            else:
                feat = model(x=img, cam_label=cam, view_label=vw)
                if feat_norm:
                    feat = _ops.l2_normalize(feat)
            lo = 0
            for (_, pid, camid, _, _, _) in group:
                evaluator.update((feat[lo:lo + len(pid)], pid, camid))
                lo += len(pid)
                processed_samples += len(pid)
                if processed_samples % 1000 == 0:
                    logger.info(f"Processed {processed_samples}/{getattr(val_loader, 'n', '?')} samples...")

    logger.info("Feature extraction finished in %.2f seconds." % (time.time() - start_time))

    cmc, mAP = evaluator.compute()[:2]
    return _report_option_a(logger, cmc, mAP, limit=getattr(evaluator, "max_rank", 50),
                            extra=lambda: report_extra_metrics(cfg, logger, evaluator))


def _report_option_a(logger, cmc, mAP, limit=50, extra=None):
    """the result lines of the TTA evaluation (same text as the reference's, processor_uniprompt_stage2.py:676-692: a rank
    that the curve does not reach is reported as such instead of indexed) and its (Rank-1, Rank-5) return value"""
    have = min(len(cmc), limit)
    logger.info("Validation Results (TTPT Option A - Image Features)")
    logger.info("mAP: {:.1%}".format(mAP))
    if extra is not None:   # the TEST.EXTRA_METRICS lines (mINP, TPR@FPR), when on
        extra()
    for r in (1, 5, 10):
        logger.info("CMC curve, Rank-{:<3}:{:.1%}".format(r, cmc[r - 1]) if r <= have else
                    f"Rank-{r} exceeds max_rank ({limit}) or CMC length ({len(cmc)}) ")
    top = [float(cmc[r - 1]) if len(cmc) >= r else 0.0 for r in (1, 5)]
    logger.info("Returning Rank-1: {:.1%}, Rank-5: {:.1%}".format(*top))
    return top[0], top[1]


def _stage2_text_features(model, num_classes, batch):
    """the text features of every identity, in label order (reference :58-73)"""
    out = []
    with torch.no_grad():
        for lo in range(0, num_classes, batch):
            out.append(model(label=torch.arange(lo, min(lo + batch, num_classes)), get_text=True))
    return torch.cat(out, 0).cuda().float().contiguous()


def _check_range(t, n, what):
    if torch.is_tensor(t) and not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise ValueError(f"stage 2: {what} outside 0 .. {n - 1}")


def do_train_stage2(cfg, model, center_criterion, train_loader_stage2, val_loader, optimizer, optimizer_center, scheduler,
                    loss_fn, num_query, local_rank, max_epochs, log_period, checkpoint_period, eval_period):
    from datetime import timedelta
    from utils.meter import AverageMeter
    device = "cuda"
    epochs = max_epochs
    logger = logging.getLogger("transreid.train")
    logger.info('start training')
    moe = bool(getattr(model, "_is_moe", lambda: False)())
    if getattr(model, "_train_encoder", None) is None:
        if moe:   # the caller's marking is kept: it must have frozen every `expert` name, as both stage-2 optimizers do
            model.enable_stage2_moe_training(set_requires_grad=False)
        else:
            model.enable_stage2_training(set_requires_grad=False)
    from model.make_model_uniprompt import LOAD_BALANCE_LOSS_COEFF, load_balancing_loss_func
    aux_meter = AverageMeter()
    model.to(device)
    num_classes = model.num_classes
    loss_meter, acc_meter = AverageMeter(), AverageMeter()
    evaluator = R1_mAP_eval(num_query, max_rank=50, feat_norm=cfg.TEST.FEAT_NORM)
    all_start_time = time.monotonic()

    model.eval()
    text_features = _stage2_text_features(model, num_classes, cfg.SOLVER.STAGE2.IMS_PER_BATCH)
    trainer = model.stage2_trainer(cfg, optimizer, text_features) if isinstance(optimizer, _ops.TensorOptimizer) else None
    logger.info("stage 2: {} identities, {} step".format(
        num_classes, "fused (mpreid.ops.Stage2Trainer)" if trainer is not None else "autograd"))
    sie_rows = model.cv_embed.shape[0] if (cfg.MODEL.SIE_CAMERA or cfg.MODEL.SIE_VIEW) else 0
    rank0 = not (cfg.MODEL.DIST_TRAIN and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0

    for epoch in range(1, epochs + 1):
        start_time = time.time()
        loss_meter.reset()
        acc_meter.reset()
        aux_meter.reset()
        evaluator.reset()
        scheduler.step(epoch)
        model.train()
        pending = []     # (loss, accuracy, batch size, aux loss) of the steps that have not been read back yet: device scalars
        n_batches = len(train_loader_stage2)
        n_iter = -1
        for n_iter, (img, vid, target_cam, target_view) in enumerate(train_loader_stage2):
            vid = torch.as_tensor(vid)
            _check_range(vid, num_classes, "labels")
            target = vid.to(device).long()
            target_cam = torch.as_tensor(target_cam).long() if cfg.MODEL.SIE_CAMERA else None
            target_view = torch.as_tensor(target_view).long() if cfg.MODEL.SIE_VIEW else None
            if sie_rows:
                _check_range(model._sie_index(target_cam, target_view), sie_rows, "SIE rows")
            target_cam = None if target_cam is None else target_cam.to(device)
            target_view = None if target_view is None else target_view.to(device)
            img = img.to(device)
            if trainer is not None:
                st = trainer.step(img, target, model._sie_index(target_cam, target_view))   # (an MoE tower: + 0.01 l_aux inside)
                loss, acc = st.loss.clone(), st.acc
                aux = None if st.aux_loss is None else st.aux_loss.clone()
            else:
                optimizer.zero_grad()
                optimizer_center.zero_grad()
                out = model(x=img, label=target, cam_label=target_cam, view_label=target_view)
                scores, feats_all, image_features_proj = out[:3]
                logits_i2t = image_features_proj @ text_features.t()
                loss = loss_fn(scores[0], feats_all[1], target, target_cam, logits_i2t)
                aux = None
                if len(out) == 4:   # an MoE tower (reference :121-128, on ONE layer of logits [L * B, E])
                    aux = load_balancing_loss_func(out[3], cfg.MODEL.MOE.TOP_K).detach()   # the value logged: the logits are data
                    loss = loss + LOAD_BALANCE_LOSS_COEFF * model.router_aux_loss.sum()    # the same function, differentiable
                loss.backward()
                optimizer.step()
                acc = (logits_i2t.max(1)[1] == target).float().mean()
                loss = loss.detach()
            pending.append((loss, acc, img.shape[0], aux))
            if (n_iter + 1) % log_period == 0 or n_iter + 1 == n_batches:
                for value, a, n, x in pending:
                    loss_meter.update(float(value), n)
                    acc_meter.update(float(a), 1)
                    if x is not None:
                        aux_meter.update(float(x), n)
                pending = []
            if (n_iter + 1) % log_period == 0:
                logger.info("Epoch[{}] Iteration[{}/{}] Loss: {:.3f}, Acc: {:.3f}, Base Lr: {:.2e}"
                            .format(epoch, (n_iter + 1), n_batches, loss_meter.avg, acc_meter.avg, optimizer.param_groups[0]['lr']))
                if moe:   # reference :154-155
                    logger.info("Epoch[{}] Iteration[{}/{}] AuxLoss: {:.4f}".format(epoch, (n_iter + 1), n_batches, aux_meter.avg))
        torch.cuda.synchronize()
        time_per_batch = (time.time() - start_time) / max(n_iter + 1, 1)
        if not cfg.MODEL.DIST_TRAIN:
            batch_size = getattr(train_loader_stage2, "batch_size", None) or cfg.SOLVER.STAGE2.IMS_PER_BATCH
            logger.info("Epoch {} done. Time per batch: {:.3f}[s] Speed: {:.1f}[samples/s]"
                        .format(epoch, time_per_batch, batch_size / time_per_batch))

        if epoch % checkpoint_period == 0 and rank0:
            out_dir = os.path.join(cfg.OUTPUT_DIR, cfg.DATASETS.EXP_SETTING)
            os.makedirs(out_dir, exist_ok=True)
            state = dict(model.state_dict())
            state.update(model.text_state_dict())
            torch.save(state, os.path.join(out_dir, cfg.MODEL.NAME + '_{}.pth'.format(epoch)))

        if epoch % eval_period == 0 and rank0:
            model.eval()
            for img, pid, camid, camids, target_view, _ in val_loader:
                with torch.no_grad():
                    img = img.to(device)
                    camids = camids.to(device) if cfg.MODEL.SIE_CAMERA else None
                    target_view = target_view.to(device) if cfg.MODEL.SIE_VIEW else None
                    feat = model(x=img, cam_label=camids, view_label=target_view)
                    evaluator.update((feat, pid, camid))
            cmc, mAP = evaluator.compute()[:2]
            logger.info("Validation Results - Epoch: {}".format(epoch))
            logger.info("mAP: {:.1%}".format(mAP))
            for r in [1, 5, 10]:
                logger.info("CMC curve, Rank-{:<3}:{:.1%}".format(r, cmc[r - 1]))
            torch.cuda.empty_cache()

    total_time = timedelta(seconds=time.monotonic() - all_start_time)
    logger.info("Total running time: {}".format(total_time))
