#!/usr/bin/env python3
"""Training input benchmark: a stage-2 batch of 64 decoded uint8 images around 128 x 64 (the synthetic training set's ragged
sizes) through the reference's train_transforms on the GPU -- one packed upload, the bicubic resize to 256 x 128, the
augmentation kernel -- beside one Stage2Trainer.step measured in the same process.  Medians of `rounds` after a warm-up.
  upload    mpreid.ops.upload_raw_images (packing on the host is inside the host clock, the copy between device events)
  resize    mpreid_resize_u8 with the bicubic filter alone, on the packed batch (device events)
  augment   mpreid_train_augment_f32 alone, on the resized batch (device events), and its share of the HBM floor
            B * H * W * (3 + 12) bytes at a 6.3 TB/s copy
  total     TrainAugment.apply, draws included (host clock + synchronise)
  step      Stage2Trainer.step on the batch it produced: ViT-B/16, 256 x 128, 751 identities (host clock + synchronise)
  host      the same transforms through PIL + numpy on the host, one image after the other (when PIL is importable)
One JSON line, also written to profiles/train_input_bench.json.  No time is a gate.
Usage: python tools/train_input_bench.py [--rounds 15] [--batch 64] [--no-step]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mpreid import ops  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from stage2_head_bench import _median, _ms  # noqa: E402
from stage2_train_bench import COPY_BYTES_PER_S, _host_ms  # noqa: E402


def _host_pipeline(imgs, table, aug, rng):
    from PIL import Image
    H, W = aug.size_hw
    pad = aug.pad
    m, s = np.asarray(aug.mean, np.float32), np.asarray(aug.std, np.float32)
    out = np.empty((len(imgs), 3, H, W), np.float32)
    for b, (img, r) in enumerate(zip(imgs, table)):
        a = np.asarray(Image.fromarray(img, "RGB").resize((W, H), Image.BICUBIC))
        if r[0]:
            a = a[:, ::-1]
        a = np.pad(a, ((pad, pad), (pad, pad), (0, 0)))[r[1]:r[1] + H, r[2]:r[2] + W]
        t = ((a.astype(np.float32) / np.float32(255.0) - m) / s).transpose(2, 0, 1)
        if r[5]:
            t[:, r[3]:r[3] + r[5], r[4]:r[4] + r[6]] = rng.standard_normal((3, r[5], r[6]), dtype=np.float32)
        out[b] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ids", type=int, default=751)
    ap.add_argument("--no-step", action="store_true", help="skip the Stage2Trainer.step measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_input_bench.json"))
    a = ap.parse_args()
    from datasets.make_dataloader import SyntheticTrainSet
    H, W, B = 256, 128, a.batch
    data = SyntheticTrainSet(B, min(B // 4, a.ids), 4, 1234)
    imgs = [data[i][0] for i in range(B)]
    ids = np.arange(B, dtype=np.int64)
    aug = ops.TrainAugment((H, W), 0.5, 10, 0.5, seed=1)
    torch.manual_seed(0)
    random.seed(0)
    table = aug.draw(B)
    raw_bytes = int(sum(im.size for im in imgs))
    res = {"tool": "train_input_bench", "device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds,
           "size_hw": [H, W], "raw_bytes": raw_bytes, "erased_images": int((table[:, 5] > 0).sum())}

    packed = ops.upload_raw_images(imgs)
    resized = ops.resize_u8(packed, (H, W), "bicubic")
    out = ops.train_augment(resized, aug.pad, table, ids, aug.seed)
    for _ in range(3):
        aug.apply(imgs, ids)
    torch.cuda.synchronize()
    up_dev, up_host, t_rs, t_au, t_tot = [], [], [], [], []
    for _ in range(a.rounds):
        up_dev.append(_ms(lambda: ops.upload_raw_images(imgs)))
        up_host.append(_host_ms(lambda: ops.upload_raw_images(imgs)))
        t_rs.append(_ms(lambda: ops.resize_u8(packed, (H, W), "bicubic")))
        t_au.append(_ms(lambda: ops.train_augment(resized, aug.pad, table, ids, aug.seed, out=out)))
        t_tot.append(_host_ms(lambda: aug.apply(imgs, ids)))
    floor_ms = B * H * W * (3 + 12) / COPY_BYTES_PER_S * 1e3
    au = _median(t_au)
    res["gpu"] = {"upload_events_ms": round(_median(up_dev), 4), "upload_host_ms": round(_median(up_host), 4),
                  "resize_bicubic_ms": round(_median(t_rs), 4), "augment_ms": round(au, 4),
                  "augment_min_max_ms": [round(min(t_au), 4), round(max(t_au), 4)],
                  "augment_hbm_floor_ms": round(floor_ms, 5), "augment_share_of_floor": round(floor_ms / au, 4),
                  "total_ms": round(_median(t_tot), 4), "total_min_max_ms": [round(min(t_tot), 4), round(max(t_tot), 4)]}

    try:
        import PIL
        rng = np.random.default_rng(0)
        _host_pipeline(imgs, table, aug, rng)
        t_h = []
        for _ in range(max(3, a.rounds // 3)):
            t = time.perf_counter()
            _host_pipeline(imgs, table, aug, rng)
            t_h.append((time.perf_counter() - t) * 1e3)
        res["host"] = {"pil_numpy_ms": round(_median(t_h), 3), "pillow": PIL.__version__, "threads": 1}
    except ImportError:
        res["host"] = None

    if not a.no_step:
        from config import cfg_base
        from loss.make_loss import make_loss
        from model import make_model_uniprompt as mu
        from solver.make_optimizer_prompt import make_optimizer_2astage
        cfg = cfg_base.clone()
        cfg.defrost()
        cfg.merge_from_list(["DATALOADER.SAMPLER", "softmax_triplet"])
        cfg.SOLVER.STAGE2.update(BASE_LR=1e-6, IMS_PER_BATCH=B)
        m = mu.make_model(cfg, num_class=a.ids, camera_num=6, view_num=1).enable_stage2_training()
        _, center = make_loss(cfg, a.ids)
        opt, _ = make_optimizer_2astage(cfg, m, center)
        g = torch.Generator().manual_seed(1)
        y = torch.randperm(a.ids, generator=g)[:B // 4].repeat_interleave(4)[torch.randperm(B, generator=g)].cuda()
        with torch.no_grad():
            m.eval()
            text = torch.cat([m(label=torch.arange(lo, min(lo + 64, a.ids)), get_text=True)
                              for lo in range(0, a.ids, 64)]).float().contiguous()
        tr = m.stage2_trainer(cfg, opt, text)
        img = aug.apply(imgs, ids)
        for _ in range(3):
            tr.step(img, y)
        t_step, t_tot2 = [], []
        for _ in range(a.rounds):
            t_tot2.append(_host_ms(lambda: aug.apply(imgs, ids)))
            t_step.append(_host_ms(lambda: tr.step(img, y)))
        st, tt = _median(t_step), _median(t_tot2)
        res["step"] = {"stage2_step_ms": round(st, 3), "input_total_ms_beside_it": round(tt, 4),
                       "input_share_of_step": round(tt / st, 4)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
