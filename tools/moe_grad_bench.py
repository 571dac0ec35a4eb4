#!/usr/bin/env python3
"""MoE training-step benchmark (random-init weights, ViT-B/16 at 256 x 128, batch 64, E = 4, K = 2, with 2 and 12 MoE blocks).

Per configuration, in one process with the dense tower beside it (interleaved rounds, device events): the training forward
(VitEncoder.forward_train) and the backward sweep (VitEncoder.backward, every master, aux_coef 0.01) of the MoE tower and of the
dense tower -- the two parts of tools/stage2_train_bench.py's step that differ between the towers; per-kernel milliseconds of
the MoE gradient kernels from the library's per-launch profile; the two grouped exact-fp32 GEMMs in TFLOP/s on the routed slot
count (2 * slots * N * K), measured through the unit seam (ops.moe_mlp_backward on random rows routed by block 0's gate), beside
the exact-fp32 distance GEMM at the same M x N x K (ops.euclidean_distance: the kernel whose tile and staging the grouped one
shares and mpreid_gemm_f32_linear's; the call also computes the row norms) and beside the 157 TF fp32 matrix peak.  Writes
profiles/moe_grad_bench.json.
Usage: python tools/moe_grad_bench.py [--batch 64] [--steps 5] [--layers 2,12]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mpreid import _lib, ops, synth  # noqa: E402

PROF = {115: "u_recompute", 112: "fc1", 113: "fc2", 116: "d_w", 117: "grad_dt", 118: "grad_dh", 119: "grad_combine", 120: "router_grad"}
FP32_MATRIX_PEAK_TF = 157.0


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _profile(L, fn, reps=1):
    L.mpreid_profile_reset()
    L.mpreid_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    L.mpreid_profile_enable(0)
    ents = (_lib.ProfileEntry * 128)()
    n = L.mpreid_profile_query(ents, 128)
    out = {}
    for e in list(ents)[:n]:
        if e.epilogue in PROF:
            out[PROF[e.epilogue]] = out.get(PROF[e.epilogue], 0.0) + e.total_ms / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", default="2,12")
    a = ap.parse_args()
    L = _lib.load()
    E, K = 4, 2
    base = dict(synth.VIT_B16)
    W = base["width"]
    B = a.batch
    rows = B * 129
    imgs = torch.from_numpy(synth.synthetic_images(B, 256, 128, seed=3)).cuda()
    g = torch.Generator().manual_seed(1)
    d_f, d_fp = (torch.randn((B, n), generator=g).cuda() * 0.1 for n in (W, base["out_dim"]))
    dense = ops.VitEncoder(base, synth.vit_state_dict(base, seed=7), (256, 128), ws_tag="gbench_dense")
    dense.enable_training()
    dense_names = [k for k, _, _ in dense._param_fields()]
    results = []
    for ML in (int(v) for v in a.layers.split(",")):
        cfg = dict(base, num_experts=E, top_k=K, moe_layers=ML)
        sd = synth.vit_moe_state_dict(cfg, seed=7, std=0.02, ln_jitter=0.0)
        enc = ops.VitEncoder(cfg, sd, (256, 128), ws_tag="gbench_moe")
        enc.enable_training()
        names = [k for k, _, _ in enc._param_fields()]
        fwd_m = lambda: enc.forward_train(imgs, want_router=True)                                  # noqa: E731
        bwd_m = lambda: enc.backward(imgs, None, None, d_f, d_fp, want=names, aux_coef=0.01)       # noqa: E731
        fwd_d = lambda: dense.forward_train(imgs)                                                  # noqa: E731
        bwd_d = lambda: dense.backward(imgs, None, None, d_f, d_fp, want=dense_names)              # noqa: E731
        for fn in (fwd_m, bwd_m, fwd_d, bwd_d):
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ("moe_forward", "moe_backward", "dense_forward", "dense_backward")}
        for _ in range(a.steps):   # interleaved rounds in one process
            for k, fn in zip(t, (fwd_m, bwd_m, fwd_d, bwd_d)):
                t[k].append(_ms(fn))
        res = {"device": torch.cuda.get_device_name(0), "batch": B, "num_experts": E, "top_k": K, "moe_layers": ML,
               "ms": {k: round(_median(v), 3) for k, v in t.items()},
               "backward_kernel_ms": {k: round(v, 4) for k, v in _profile(L, bwd_m).items()}}
        # the grouped fp32 GEMMs through the unit seam: the slot count is known on the host there
        p0 = "transformer.resblocks.0."
        h = torch.randn((rows, W), generator=torch.Generator().manual_seed(5)).cuda()
        dy = torch.randn((rows, W), generator=torch.Generator().manual_seed(6)).cuda()
        sel, wts, _ = ops.moe_route(h, torch.from_numpy(sd[p0 + "gate.weight"]), K)
        counts = torch.bincount(sel.flatten().long().cpu(), minlength=E)
        slots = int(((counts + 127) // 128 * 128).sum())
        mats = [np.stack([sd[f"{p0}experts.{e}.{nm}"] for e in range(E)])
                for nm in ("c_fc.weight", "c_fc.bias", "c_proj.weight", "c_proj.bias")]
        layer, keep = ops.pack_moe_layer(*mats)
        layer_t, keep_t = ops.pack_moe_layer_t(mats[0], mats[2])
        pairs = ops.split_pairs_f32(h)
        seam_fn = lambda: ops.moe_mlp_backward(pairs, sel, wts, layer, layer_t, dy, E)             # noqa: E731
        seam_fn()
        seam = _profile(L, seam_fn, reps=7)
        res["slots"] = slots
        res["seam_kernel_ms"] = {k: round(v, 4) for k, v in seam.items()}
        for name, N, Kd in (("grad_dt", 4 * W, W), ("grad_dh", W, 4 * W)):
            res[name + "_tflops"] = round(2.0 * slots * N * Kd / seam[name] / 1e9, 1)
            A = torch.rand((slots, Kd), device="cuda") * 2 - 1
            Bm = torch.rand((N, Kd), device="cuda") * 2 - 1
            ref = lambda: ops.euclidean_distance(A, Bm)   # the same exact-fp32 MFMA GEMM kernel (distance epilogue), M x N x K  # noqa: E731
            ref()
            res["exact_f32_gemm_tflops_%dx%dx%d" % (slots, N, Kd)] = round(
                2.0 * slots * N * Kd / _median([_ms(ref) for _ in range(7)]) / 1e9, 1)
        res["fp32_matrix_peak_tflops"] = FP32_MATRIX_PEAK_TF
        print(json.dumps(res), flush=True)
        results.append(res)
        del enc, layer, keep, layer_t, keep_t
        ops.release_workspaces()
        torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "moe_grad_bench.json"), "w") as fh:
        json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
