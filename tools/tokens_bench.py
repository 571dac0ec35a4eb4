#!/usr/bin/env python3
"""Long-token geometries on one GPU: device-resident images/s of the encoders at 256 x 256 (ViT-B/16 L = 257 split and fp16,
RN50 split) next to 256 x 128 (L = 129) from the same process, and the attention kernel's time per launch and TF/s at
L = 129, 257 and 442 (4 * L^2 * 64 * heads * B FLOP per full launch; mpreid_profile_* hooks: hipEvents around each launch).

    python tools/tokens_bench.py [--reps 5] [--csv profiles/tokens_attention.csv]

Batches are make_model's encode_group (65536 // tokens images for the ViT, 256 for RN50); images are device-resident
(the host pipeline is not part of the figure).  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]

import torch  # noqa: E402

from mpreid import _lib, ops, synth  # noqa: E402


def rate(enc, x, reps):
    enc(x)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        enc(x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return x.shape[0] / best


def vit(hw, stride, prec):
    h, w = (hw[0] - 16) // stride + 1, (hw[1] - 16) // stride + 1
    cfg = dict(synth.VIT_B16, h_res=h, w_res=w, stride=stride)
    L = h * w + 1
    B = max(64, 65536 // L)
    enc = ops.VitEncoder(cfg, synth.vit_state_dict(cfg, seed=7, std=0.02), hw, precision=prec, ws_tag="tb")
    x = torch.from_numpy(synth.synthetic_images(min(B, 64), hw[0], hw[1], seed=1)).cuda()
    x = x.repeat((B + x.shape[0] - 1) // x.shape[0], 1, 1, 1)[:B].contiguous()
    return enc, x, L, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--csv", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    Lb = _lib.load()
    res = {"device": torch.cuda.get_device_name(0)}
    for prec in ("split", "fp16"):
        for hw, key in (((256, 128), "256x128"), ((256, 256), "256x256")):
            enc, x, L, B = vit(hw, 16, prec)
            res[f"vit_{prec}_{key}_img_s"] = round(rate(enc, x, a.reps), 1)
            ops.release_workspaces("tb")
        res[f"vit_{prec}_ratio_256x256_vs_256x128"] = round(res[f"vit_{prec}_256x256_img_s"] / res[f"vit_{prec}_256x128_img_s"], 3)
    for hw, key in (((256, 128), "256x128"), ((256, 256), "256x256")):
        cfg = dict(synth.RN50, h_res=hw[0] // 16, w_res=hw[1] // 16)
        enc = ops.Rn50Encoder(cfg, synth.rn50_state_dict(cfg, seed=11), hw, precision="split", ws_tag="tb")
        x = torch.from_numpy(synth.synthetic_images(64, hw[0], hw[1], seed=2)).cuda().repeat(4, 1, 1, 1).contiguous()
        res[f"rn50_split_{key}_img_s"] = round(rate(enc, x, a.reps), 1)
        ops.release_workspaces("tb")
    res["rn50_split_ratio_256x256_vs_256x128"] = round(res["rn50_split_256x256_img_s"] / res["rn50_split_256x128_img_s"], 3)
    # attention kernel per launch: full (not CLS-only) launches of one encoder call, profiled
    rows = []
    for prec in ("split", "fp16"):
        for hw, stride in (((256, 128), 16), ((256, 256), 16), ((256, 256), 12)):
            enc, x, L, B = vit(hw, stride, prec)
            enc(x)
            torch.cuda.synchronize()
            Lb.mpreid_profile_reset()
            Lb.mpreid_profile_enable(1)
            enc(x)
            torch.cuda.synchronize()
            Lb.mpreid_profile_enable(0)
            ents = (_lib.ProfileEntry * 48)()
            n = Lb.mpreid_profile_query(ents, 48)
            for i in range(n):
                e = ents[i]
                if e.epilogue == 101 and e.n == 0:
                    us = e.total_ms / e.launches * 1e3
                    tf = 4.0 * L * L * 64 * 12 * B / (us * 1e-6) / 1e12
                    kern = "attention_long_kernel" if L > 256 else ("attention_split_kernel" if prec == "split" else "attention_kernel")
                    rows.append(dict(precision=prec, L=L, batch=B, kernel=kern, launches=int(e.launches), us_per_launch=round(us, 1),
                                     tflops=round(tf, 1)))
            ops.release_workspaces("tb")
    res["attention"] = rows
    if a.csv:
        with open(a.csv, "w") as fh:
            fh.write("precision,L,batch,kernel,launches,us_per_launch,tflops\n")
            for r in rows:
                fh.write(",".join(str(r[k]) for k in ("precision", "L", "batch", "kernel", "launches", "us_per_launch", "tflops")) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
