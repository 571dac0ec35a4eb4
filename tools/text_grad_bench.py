#!/usr/bin/env python3
"""Prompt-gradient micro-benchmark (random-init weights): the identity prompts of Market-1501 (751 prompts of 77 tokens) through
ops.TextEncoder.forward and ops.TextEncoder.backward, alternating in one process and timed with device events after a warm-up;
reports the medians and the backward / forward ratio.  Also the causal attention backward kernel alone at the same shape, beside
the forward's causal kernel.  The result is printed as one JSON line and written to profiles/text_grad_bench.json.
No rate is a gate.
Usage: python tools/text_grad_bench.py [--prompts 751] [--steps 7] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
from mpreid import ops, synth  # noqa: E402


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=751)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_grad_bench.json"))
    a = ap.parse_args()
    cfg = synth.CLIP_TEXT
    B, L, W, H = a.prompts, cfg["tokens"], cfg["width"], cfg["heads"]
    enc = ops.TextEncoder(cfg, synth.text_state_dict(cfg, seed=21))
    g = torch.Generator().manual_seed(1)
    prompts = (torch.randn((B, L, W), generator=g) * 0.02).cuda()
    grad_out = torch.randn((B, cfg["out_dim"]), generator=g).cuda()
    eot = [19] * B
    fwd = lambda: enc.forward(prompts, eot)               # noqa: E731
    bwd = lambda: enc.backward(prompts, eot, grad_out)    # noqa: E731
    fwd(), bwd()    # warm-up: workspaces, transposed weights, LDS attribute, code objects
    torch.cuda.synchronize()
    tf, tb = [], []
    for _ in range(a.steps):
        tf.append(_ms(fwd))
        tb.append(_ms(bwd))
    f, b = _median(tf), _median(tb)
    # the attention kernels alone on the same q | k | v, interleaved
    qkv = torch.randn((B * L, 3 * W), generator=g).cuda()
    d_o = torch.randn((B * L, W), generator=g).cuda()
    o = torch.empty((B * L, 2 * W), dtype=torch.float16, device="cuda")
    dq = torch.empty((B * L, 3 * W), dtype=torch.float32, device="cuda")
    att_f = lambda: ops.text_attention(qkv, B, L, H, out=o)                   # noqa: E731
    att_b = lambda: ops.text_attention_backward(qkv, d_o, B, L, H, out=dq)    # noqa: E731
    att_f(), att_b()
    torch.cuda.synchronize()
    af, ab = [], []
    for _ in range(a.reps):
        af.append(_ms(att_f))
        ab.append(_ms(att_b))
    af, ab = _median(af), _median(ab)
    # the backward call's arithmetic: the forward, the recompute without FC2 (5/6 of a forward), the gradient GEMMs (a forward's
    # worth in fp32), 2 M K N each over 12 W^2 weights per layer
    gemm_flop = 2.0 * B * L * 12 * W * W * cfg["layers"]
    res = {"device": torch.cuda.get_device_name(0), "prompts": B, "tokens": L, "forward_ms": round(f, 3), "backward_ms": round(b, 3),
           "backward_over_forward": round(b / f, 3), "attention_forward_us": round(af * 1e3, 1),
           "attention_backward_us": round(ab * 1e3, 1),
           "attention_backward_share_of_backward": round(cfg["layers"] * ab / b, 4),
           "linear_tflop_forward": round(gemm_flop / 1e12, 3), "linear_tflop_backward": round((1.0 + 5.0 / 6.0 + 1.0) * gemm_flop / 1e12, 3)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
