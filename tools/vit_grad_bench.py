#!/usr/bin/env python3
"""Image-tower gradient micro-benchmark (random-init weights): the Market-1501 shape (256 x 128, 129 tokens), batch 64, CLIP
ViT-B/16.  In one process, interleaved turn by turn and timed with device events after a warm-up, medians of 15:
  * ops.VitEncoder.forward (no neck), forward_train, and forward_train + backward with every gradient, beside the same tower
    as a plain torch fp32 module (written here) under autograd on the same device, forward and forward + backward;
  * backward with no parameter gradient (tokens only): the difference is the share of the weight-gradient GEMMs, transposes
    and column sums;
  * the unmasked attention gradient alone (ops.vit_attention_backward) per layer at 129 and at 257 tokens, beside the forward's
    split-precision attention kernel on the same q | k | v, and beside torch's fp32 scaled_dot_product_attention forward +
    backward.
Each figure carries the (min, max) of its interleaved series.  The result is printed as one JSON line and written to
profiles/vit_grad_bench.json.  No rate is a gate.
Usage: python tools/vit_grad_bench.py [--batch 64] [--reps 15]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
from mpreid import ops, synth  # noqa: E402


class TorchTower:
    """the same tower as plain torch fp32 operations on the encoder's own master tensors (tests/vit_grad_cases.py: tower)"""

    def __init__(self, cfg, masters):
        self.cfg, self.g = cfg, masters
        self.params = list(masters.values())

    def __call__(self, imgs):
        import torch.nn.functional as F
        cfg, g = self.cfg, self.g
        w, heads = cfg["width"], cfg["heads"]
        B = imgs.shape[0]
        tok = F.conv2d(imgs, g["conv1.weight"], stride=cfg["stride"]).flatten(2).transpose(1, 2)
        x = torch.cat([g["class_embedding"].expand(B, 1, w), tok], dim=1) + g["positional_embedding"]
        x = F.layer_norm(x, (w,), g["ln_pre.weight"], g["ln_pre.bias"], 1e-5)
        L = x.shape[1]
        f_last = x[:, 0]
        for i in range(cfg["layers"]):
            b = f"transformer.resblocks.{i}"
            f_last = x[:, 0]
            h = F.layer_norm(x, (w,), g[b + ".ln_1.weight"], g[b + ".ln_1.bias"], 1e-5)
            qkv = F.linear(h, g[b + ".attn.in_proj_weight"], g[b + ".attn.in_proj_bias"])
            q, k, v = (t.reshape(B, L, heads, 64).transpose(1, 2) for t in qkv.split(w, dim=2))
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, w)
            x = x + F.linear(a, g[b + ".attn.out_proj.weight"], g[b + ".attn.out_proj.bias"])
            h = F.layer_norm(x, (w,), g[b + ".ln_2.weight"], g[b + ".ln_2.bias"], 1e-5)
            h = F.linear(h, g[b + ".mlp.c_fc.weight"], g[b + ".mlp.c_fc.bias"])
            h = h * torch.sigmoid(1.702 * h)
            x = x + F.linear(h, g[b + ".mlp.c_proj.weight"], g[b + ".mlp.c_proj.bias"])
        f = F.layer_norm(x[:, 0], (w,), g["ln_post.weight"], g["ln_post.bias"], 1e-5)
        return f_last, f, f @ g["proj"]


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(v):
    return sorted(v)[len(v) // 2]


def _interleaved(fns, reps):
    """every function once per turn, `reps` turns -> per function (median, min, max) in ms"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(_ms(fn))
    return [(_median(v), min(v), max(v)) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_grad_bench.json"))
    a = ap.parse_args()
    cfg = synth.VIT_B16
    B, W, H = a.batch, cfg["width"], cfg["heads"]
    enc = ops.VitEncoder(cfg, synth.vit_state_dict(cfg, seed=7), (256, 128), ws_tag="vit_grad_bench")
    img = torch.from_numpy(synth.synthetic_images(B, 256, 128, seed=3)).cuda()
    enc.enable_training()
    seeds = [torch.randn((B, n), device="cuda") * 0.1 for n in (W, W, cfg["out_dim"])]
    ref = TorchTower(cfg, enc.masters)
    ref_seeds = seeds

    def ours_fb():
        enc.forward_train(img)
        enc.backward(img, None, *seeds)

    def ours_fb_data_only():
        enc.forward_train(img)
        enc.backward(img, None, *seeds, want=["tokens"])

    def torch_f():
        with torch.no_grad():
            ref(img)

    def torch_fb():
        for p in ref.params:
            p.grad = None
        feats = ref(img)
        torch.autograd.backward(feats, ref_seeds)

    names = ["forward", "forward_train", "forward_train_backward", "forward_train_backward_no_weight_grads", "torch_fp32_forward",
             "torch_fp32_forward_backward"]
    series = _interleaved([lambda: enc.forward(img), lambda: enc.forward_train(img), ours_fb, ours_fb_data_only, torch_f, torch_fb],
                          a.reps)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "reps": a.reps}
    for n, (med, lo, hi) in zip(names, series):
        res[n + "_ms"] = round(med, 3)
        res[n + "_ms_range"] = [round(lo, 3), round(hi, 3)]
    t = {n: v[0] for n, v in zip(names, series)}
    bwd = t["forward_train_backward"] - t["forward_train"]
    res["backward_ms"] = round(bwd, 3)
    res["backward_over_forward"] = round(bwd / t["forward_train"], 3)
    res["weight_gradient_share_of_backward"] = round((t["forward_train_backward"] - t["forward_train_backward_no_weight_grads"]) / bwd, 3)
    res["torch_fp32_backward_over_forward"] = round((t["torch_fp32_forward_backward"] - t["torch_fp32_forward"]) / t["torch_fp32_forward"], 3)
    res["forward_backward_over_torch_fp32"] = round(t["forward_train_backward"] / t["torch_fp32_forward_backward"], 3)
    # the spread between the interleaved series: the widest (max - min) / median of any of them
    res["largest_spread"] = round(max((hi - lo) / med for med, lo, hi in series), 4)
    g = torch.Generator().manual_seed(1)
    for L in (129, 257):
        qkv = torch.randn((B * L, 3 * W), generator=g).cuda()
        d_o = torch.randn((B * L, W), generator=g).cuda()
        o = torch.empty((B * L, 2 * W), dtype=torch.float16, device="cuda")
        dq = torch.empty((B * L, 3 * W), dtype=torch.float32, device="cuda")
        q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2).contiguous().requires_grad_(True) for t in qkv.split(W, dim=1))
        go = d_o.reshape(B, L, H, 64).transpose(1, 2).contiguous()

        def torch_fb():
            out = torch.nn.functional.scaled_dot_product_attention(q, k, v)
            torch.autograd.grad(out, (q, k, v), grad_outputs=go)
        (af, _, _), (ab, ab_lo, ab_hi), (tfb, _, _) = _interleaved(
            [lambda: ops.vit_attention(qkv, B, L, H, out=o), lambda: ops.vit_attention_backward(qkv, d_o, B, L, H, out=dq), torch_fb],
            a.reps)
        # the gradient's arithmetic: s, dP in both passes, dQ, dK, dV = 7 products of L x L x 64 per (image, head)
        flop = 2.0 * 7 * B * H * L * L * 64
        res["tokens_%d" % L] = {"attention_forward_us": round(af * 1e3, 1), "attention_backward_us": round(ab * 1e3, 1),
                                "attention_backward_us_range": [round(ab_lo * 1e3, 1), round(ab_hi * 1e3, 1)],
                                "attention_backward_tflops": round(flop / ab / 1e9, 2),
                                "torch_sdpa_fp32_forward_backward_us": round(tfb * 1e3, 1)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
