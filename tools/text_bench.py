#!/usr/bin/env python3
"""Text tower micro-benchmark (random-init weights): milliseconds for the identity prompts of Market-1501 (751 prompts of 77
tokens) through ops.TextEncoder, and the causal attention kernel alone against the unmasked split dispatcher
(mpreid_vit_attention) at the same shape, launches interleaved in one run and timed with device events.
Usage: python tools/text_bench.py [--prompts 751] [--steps 5] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
from mpreid import ops, synth  # noqa: E402


def _median_ms(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=751)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    cfg = synth.CLIP_TEXT
    B, L, W, H = a.prompts, cfg["tokens"], cfg["width"], cfg["heads"]
    enc = ops.TextEncoder(cfg, synth.text_state_dict(cfg, seed=21))
    g = torch.Generator().manual_seed(1)
    prompts = (torch.randn((B, L, W), generator=g) * 0.02).cuda()
    eot = [19] * B
    out = torch.empty((B, cfg["out_dim"]), device="cuda")
    enc.forward(prompts, eot, out=out)
    torch.cuda.synchronize()
    tower = sorted(_median_ms(lambda: enc.forward(prompts, eot, out=out), 1) for _ in range(a.steps))[a.steps // 2]
    # the two attention kernels on the same q | k | v, interleaved; warm-up first (LDS attribute, code objects)
    qkv = torch.randn((B * L, 3 * W), generator=g).cuda()
    o = torch.empty((B * L, 2 * W), dtype=torch.float16, device="cuda")
    causal = lambda: ops.text_attention(qkv, B, L, H, out=o)   # noqa: E731
    plain = lambda: ops.vit_attention(qkv, B, L, H, out=o)     # noqa: E731
    causal(), plain()
    torch.cuda.synchronize()
    tc_, tp_ = [], []
    for _ in range(a.reps):
        tc_.append(_median_ms(causal, 1))
        tp_.append(_median_ms(plain, 1))
    c, p = sorted(tc_)[a.reps // 2], sorted(tp_)[a.reps // 2]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "prompts": B, "tokens": L, "tower_ms": round(tower, 3),
                      "attention_causal_us": round(c * 1e3, 1), "attention_unmasked_us": round(p * 1e3, 1),
                      "causal_over_unmasked": round(c / p, 3)}))


if __name__ == "__main__":
    main()
