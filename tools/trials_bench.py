#!/usr/bin/env python3
"""Multi-trial evaluation (DATASETS.PROTOCOL vehicleid) at a VehicleID-large-like synthetic shape: 18 000 images of 2 400
identities, 256 x 256 input, 10 trials, split precision.  GPU only.

    python tools/trials_bench.py [--images N --ids I --trials T --hw H W --batch B --repeats R]
    python tools/trials_bench.py --compute-only        # no encoder: R1_mAP_eval_splits.compute() on synthetic features

Measured (device-synchronised host clocks, after a warm-up, (a) and (b) alternating):
  (a) do_inference_trials: the pool encoded once, one pool x pool matrix, every trial ranked against it in one launch;
  (b) T calls of do_inference on per-trial query-then-gallery loaders of the same images -- the shape of the reference's loop
      (test.py:46-63), on code this protocol does not touch;
  (c) R1_mAP_eval_splits.compute() alone, on the features of (a).
The ranking kernel's own time comes from a separate ``rocprofv3 --kernel-trace --stats -- python tools/trials_bench.py
--compute-only`` run; the tool prints the kernel's HBM lower bounds from the shapes to put beside it.

The images: a bank of 256 seeded random images, image i = bank[i % 256] + a per-image offset, built per batch on the host
(generating 18 000 x 3 x 256 x 256 fresh random floats per pass would time numpy's generator, not the evaluation).  Features
of images that share a bank entry are close, so the printed mAPs mean nothing; the work done does not depend on them."""
import argparse
import contextlib
import io
import json
import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mp-reid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class BankLoader:
    """the samples `order` (pool positions) of the synthetic pool, in that order, `batch` per batch, in the loaders' batch
    format (img, pids, camids, camids tensor, viewids tensor, paths)"""

    def __init__(self, bank, pids, camids, order, batch):
        self.bank, self.pids, self.camids, self.order, self.batch = bank, pids, camids, np.asarray(order), batch
        self.n = len(self.order)

    def __len__(self):
        return (self.n + self.batch - 1) // self.batch

    def __iter__(self):
        nb = self.bank.shape[0]
        for s in range(0, self.n, self.batch):
            idx = self.order[s:s + self.batch]
            img = self.bank[torch.from_numpy(idx % nb)]
            img += torch.from_numpy((idx // nb).astype(np.float32) * np.float32(2e-3))[:, None, None, None]
            cams = tuple(int(c) for c in self.camids[idx])
            yield (img, tuple(int(p) for p in self.pids[idx]), cams, torch.tensor(cams, dtype=torch.int64),
                   torch.zeros(len(idx), dtype=torch.int64), tuple(f"synthetic/{i:07d}.jpg" for i in idx))


def kernel_bounds(n, splits):
    """HBM lower bounds of the splits ranking kernel, bytes: (gathered distances + labels, the same with every gathered
    distance charged its whole 128-byte line when the split's columns are spread over the row)"""
    pairs = sum(len(q) for q, _ in splits)
    gathered = sum(4 * len(q) * len(g) for q, g in splits)
    labels = sum((8 + 4) * len(g) for _, g in splits) + pairs * (8 + 4 + 4)      # g_pids + g_idx once per split; q_pids, q_row, q_split
    lines = sum(len(q) * min(4 * n, 128 * len(np.unique(np.asarray(g) // 32))) for q, g in splits)
    return pairs, gathered + labels, lines + labels


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ts):
    return {"min_ms": round(min(ts), 2), "median_ms": round(sorted(ts)[len(ts) // 2], 2), "max_ms": round(max(ts), 2),
            "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=18000)
    ap.add_argument("--ids", type=int, default=2400)
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--hw", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--compute-only", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON result to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/trials_bench.py needs an MI355X: no HIP device visible")
    torch.cuda.set_device(0)
    from datasets.make_dataloader import vehicleid_trial_splits
    from mpreid import synth
    from utils.metrics import R1_mAP_eval_splits
    logging.getLogger("transreid.test").setLevel(logging.WARNING)
    n = a.images
    rng = np.random.default_rng(1234)
    pids = rng.permutation(np.arange(n) % a.ids).astype(np.int64)
    camids = np.zeros(n, np.int64)
    splits = vehicleid_trial_splits(pids, trials=a.trials, seed=0)
    pairs, b_gather, b_lines = kernel_bounds(n, splits)
    res = {"images": n, "ids": a.ids, "trials": a.trials, "hw": a.hw, "pairs": pairs, "gallery_per_trial": len(splits[0][1]),
           "kernel_hbm_bytes_gathered": b_gather, "kernel_hbm_bytes_whole_lines": b_lines,
           "pool_matrix_bytes": 4 * n * n, "gathered_submatrices_bytes": sum(4 * len(q) * len(g) for q, g in splits)}

    if a.compute_only:
        f, _ = synth.clustered_features(n, 512, 3.0, seed=2)
        ft = torch.from_numpy(f).cuda()
        ev = R1_mAP_eval_splits(splits, feat_norm=True)
        ts = []
        for it in range(a.repeats + 1):
            ev.reset()
            for s in range(0, n, 512):
                ev.update((ft[s:s + 512], pids[s:s + 512], camids[s:s + 512]))
            ms, out = timed(lambda: quiet(ev.compute))
            if it:
                ts.append(ms)
        res["compute_only"] = spread(ts)
        res["mean_mAP"] = float(np.mean(out[1]))
    else:
        from config import cfg_base
        from model.make_model import make_model
        from processor.processor import do_inference, do_inference_trials
        cfg = cfg_base.clone()
        cfg.defrost()
        cfg.merge_from_list(["INPUT.SIZE_TEST", list(a.hw), "INPUT.SIZE_TRAIN", list(a.hw), "MODEL.ENCODER_PRECISION", "split",
                             "TEST.IMS_PER_BATCH", a.batch, "DATASETS.SYNTH_IDS", a.ids])
        cfg.freeze()
        model = make_model(cfg, num_class=a.ids, camera_num=6, view_num=1)
        bank = torch.from_numpy(synth.synthetic_images(256, a.hw[0], a.hw[1], seed=77))
        pool = BankLoader(bank, pids, camids, np.arange(n), a.batch)
        per_trial = [(BankLoader(bank, pids, camids, np.concatenate([q, g]), a.batch), len(q)) for q, g in splits]
        seen = []
        forward = model.forward

        def counting(x, *args, **kw):
            seen.append(len(x))
            return forward(x, *args, **kw)
        model.forward = counting

        def run_a():
            return quiet(lambda: do_inference_trials(cfg, model, pool, splits))

        def run_b():
            return quiet(lambda: [do_inference(cfg, model, ld, nq) for ld, nq in per_trial])
        # warm-up: both paths once at a reduced size (kernel caches, workspaces, pinned pages)
        small = BankLoader(bank, pids, camids, np.arange(min(n, 1024)), a.batch)
        quiet(lambda: do_inference(cfg, model, small, min(n, 1024) // 2))
        t_a, t_b = [], []
        for _ in range(a.repeats):
            seen.clear()
            ms, out_a = timed(run_a)
            t_a.append(ms)
            images_a = sum(seen)
            seen.clear()
            ms, out_b = timed(run_b)
            t_b.append(ms)
            images_b = sum(seen)
        ev = do_inference_trials.last_evaluator
        t_c = [timed(lambda: quiet(ev.compute))[0] for _ in range(a.repeats + 1)][1:]
        res.update({"a_do_inference_trials": spread(t_a), "b_do_inference_per_trial": spread(t_b),
                    "c_compute_alone": spread(t_c), "images_encoded_a": images_a, "images_encoded_b": images_b,
                    "rank1_a": [float(x) for x in out_a[0]], "rank1_b": [float(r[0]) for r in out_b],
                    "speedup_median": round(spread(t_b)["median_ms"] / spread(t_a)["median_ms"], 2)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
