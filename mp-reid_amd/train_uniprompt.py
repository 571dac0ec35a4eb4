#!/usr/bin/env python3
"""Training entry point of the HIP build -- the counterpart of the reference's ``train_uniprompt.py`` (:28-215):

    python train_uniprompt.py --config_file configs/ours/cctv_ir_cctv_rgb.yml DATASETS.SYNTH_TRAIN 12936 [KEY VALUE ...]

config (YAML + command-line overrides, frozen) -> ``set_seed(SOLVER.SEED)`` -> logger ("transreid",
<OUTPUT_DIR>/<EXP_SETTING>/train_log.txt) -> ``make_dataloader`` -> ``make_model`` -> ``make_loss`` ->
  stage 1a   ``enable_stage1a_training``, ``make_optimizer_1stage('STAGE1A')``, ``create_scheduler``, ``do_train_stage1``
  stage 1b   the same with ``enable_stage1b_training`` / 'STAGE1B' / ``is_stage1b=True``
  freeze     every parameter trained except ``text_encoder`` / ``expert`` / ``prompt_learner`` names: here
             ``model.enable_stage2_training()``, which applies that rule and builds the training encoder on the module's own
             parameters; an MoE tower (MODEL.MOE.ENABLED) goes through ``enable_stage2_moe_training()``
  stage 2a   ``make_optimizer_2astage``, ``WarmupMultiStepLR``, ``do_train_stage2``
  stage 2b   ``make_optimizer_2bstage`` (the gate and the image tower without the experts), the same schedule and loop
-> ``do_inference``.  The stage-2 batches arrive as decoded uint8 images and go through train_transforms on the GPU
(datasets/make_dataloader.py: RawTrainBatch, mpreid.ops.TrainAugment); the training loaders exist for
DATASETS.SYNTH_TRAIN > 0 (a real dataset: INTEGRATION.md).

Not reproduced: ``peft`` (imported by the reference, never used), MODEL.DIST_TRAIN (one device), the cudnn flags of its
``set_seed``, and ``switch_to_moe_model`` (the tower is built as MODEL.MOE says from the start; stage 1 never trains it).
``main(argv)`` returns what ``do_inference`` returns, (rank1, rank5), so that tests can call it in-process.
"""
import argparse
import logging
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def set_seed(seed):
    import numpy as np
    import torch
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def build_parser():
    p = argparse.ArgumentParser(description="MP-ReID Uni-Prompt training on MI355X (HIP build)")
    p.add_argument("--config_file", default="", type=str, help="path to config file ('' = built-in defaults only)")
    p.add_argument("opts", default=None, nargs=argparse.REMAINDER,
                   help="KEY VALUE pairs overriding config options, e.g. SOLVER.STAGE2.MAX_EPOCHS 60")
    p.add_argument("--local_rank", default=0, type=int)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from config import cfg_base
    cfg = cfg_base.clone()
    cfg.defrost()
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    cfg.freeze()
    if cfg.MODEL.DIST_TRAIN:
        raise NotImplementedError("MODEL.DIST_TRAIN: the training loops drive one device")
    # device selection has to happen before the HIP runtime initialises (the reference sets CUDA_VISIBLE_DEVICES here)
    os.environ.setdefault("HIP_VISIBLE_DEVICES", str(cfg.MODEL.DEVICE_ID))

    set_seed(cfg.SOLVER.SEED)
    output_dir = os.path.join(cfg.OUTPUT_DIR, cfg.DATASETS.EXP_SETTING) if cfg.OUTPUT_DIR else ""
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)

    from utils.logger import setup_logger
    logger = setup_logger("transreid", output_dir, if_train=True)
    try:
        return _train(cfg, args, logger)
    finally:
        for h in [h for h in logger.handlers if isinstance(h, logging.FileHandler)]:   # an in-process caller may run again
            logger.removeHandler(h)
            h.close()


def _train(cfg, args, logger):
    from datasets.make_dataloader_uniprompt import make_dataloader
    from loss.make_loss import make_loss
    from model.make_model_uniprompt import make_model
    from processor.processor_uniprompt_stage1 import do_train_stage1
    from processor.processor_uniprompt_stage2 import do_inference, do_train_stage2
    from solver.lr_scheduler import WarmupMultiStepLR
    from solver.make_optimizer_prompt import make_optimizer_1stage, make_optimizer_2astage, make_optimizer_2bstage
    from solver.scheduler_factory import create_scheduler

    logger.info("Saving model in the path :{}".format(cfg.OUTPUT_DIR))
    logger.info(args)
    if args.config_file:
        logger.info("Loaded configuration file {}".format(args.config_file))
        with open(args.config_file) as fh:
            logger.info("\n" + fh.read())
    logger.info("Running with config:\n{}".format(cfg))

    train_loader_stage2, train_loader_stage1, val_loader, num_query, num_classes, camera_num, view_num = make_dataloader(cfg)
    if train_loader_stage2 is None or train_loader_stage1 is None:
        raise ValueError("no training loaders: set DATASETS.SYNTH_TRAIN to the number of synthetic training images (a real "
                         "dataset hands its own loaders to the stages, INTEGRATION.md)")
    model = make_model(cfg, num_class=num_classes, camera_num=camera_num, view_num=view_num)
    loss_func, center_criterion = make_loss(cfg, num_classes=num_classes)

    # ---- stage 1: prompt learning, every tower weight frozen ----
    for tag, enable, is_1b in (("STAGE1A", model.enable_stage1a_training, False), ("STAGE1B", model.enable_stage1b_training, True)):
        logger.info("===== Configuring and starting Stage {} training =====".format(tag[-2:].lower()))
        enable()
        s1 = getattr(cfg.SOLVER, tag)
        optimizer = make_optimizer_1stage(cfg, model, stage_name=tag)
        scheduler = create_scheduler(optimizer, num_epochs=s1.MAX_EPOCHS, lr_min=s1.LR_MIN, warmup_lr_init=s1.WARMUP_LR_INIT,
                                     warmup_t=s1.WARMUP_EPOCHS, noise_range=None)
        do_train_stage1(cfg, model, train_loader_stage1, optimizer, scheduler, args.local_rank, is_stage1b=is_1b)

    # ---- the stage-2 freeze by name, and the training encoder over the module's own parameters ----
    logger.info("Setting parameter `requires_grad` for Stage 2a fine-tuning: everything but text_encoder, expert and "
                "prompt_learner names")
    if cfg.MODEL.MOE.ENABLED:
        model.enable_stage2_moe_training()
    else:
        model.enable_stage2_training()

    s2 = cfg.SOLVER.STAGE2
    for tag, make_optimizer in (("2a", make_optimizer_2astage), ("2b", make_optimizer_2bstage)):
        logger.info("{} stage, {}".format(tag, "train parameters marked as trainable" if tag == "2a"
                                          else "train gate and image_encoder (except experts)"))
        optimizer, optimizer_center = make_optimizer(cfg, model, center_criterion)
        scheduler = WarmupMultiStepLR(optimizer, s2.STEPS, s2.GAMMA, s2.WARMUP_FACTOR, s2.WARMUP_ITERS, s2.WARMUP_METHOD)
        do_train_stage2(cfg, model, center_criterion, train_loader_stage2, val_loader, optimizer, optimizer_center, scheduler,
                        loss_func, num_query, args.local_rank, max_epochs=s2.MAX_EPOCHS, log_period=s2.LOG_PERIOD,
                        checkpoint_period=s2.CHECKPOINT_PERIOD, eval_period=s2.EVAL_PERIOD)

    return do_inference(cfg, model, val_loader, num_query)


if __name__ == "__main__":
    main()
