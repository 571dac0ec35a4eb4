#!/usr/bin/env python3
"""MoE image-encoder benchmark (random-init weights, ViT-B/16 at 256 x 128).

Images/s of the MoE tower for (num_experts, top_k, moe_layers) in {(1, 1, 12), (4, 2, 12), (8, 2, 12), (8, 2, 6)} with the dense
tower beside it in the same process (interleaved rounds, device events); per-kernel milliseconds of the router, the dispatch,
the two grouped GEMMs and the combine from the library's per-launch profile; the grouped GEMMs' TFLOP/s on
2 * slots * N * 3 * kseg, measured through the unit seams (ops.moe_route + ops.moe_mlp on random rows with block 0's gate and
experts, slots = the experts' host-counted rows padded to the 128-row tile), next to the
dense split FC1 / FC2 GEMMs (mpreid_gemm_f16_split_nt, the classes tools/gemm_bench.py reports) at the same row count.
Usage: python tools/moe_bench.py [--batch 64] [--steps 5] [--configs 4,2,12;8,2,6]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mpreid import _lib, ops, synth  # noqa: E402

CONFIGS = [(1, 1, 12), (4, 2, 12), (8, 2, 12), (8, 2, 6)]
PROF = {110: "router", 111: "dispatch", 112: "fc1", 113: "fc2", 114: "combine"}


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def dense_split_gemm_ms(L, rows_pad, N, kseg, epi, reps):
    """the dense tower's split FC1 (epilogue 12) / FC2 (11) at rows_pad rows, as tools/gemm_bench.py times them"""
    dev = _lib.require_gpu()
    A = ops.split_pairs_f32(torch.rand((rows_pad, kseg), device=dev) * 2 - 1)
    W = ops.split_pairs_f32((torch.rand((N, kseg), device=dev) * 2 - 1) * 400.0)
    bias = torch.randn(N, device=dev)
    out = torch.zeros((rows_pad, 2 * N), device=dev, dtype=torch.float16) if epi == 12 else torch.zeros((rows_pad, N), device=dev)
    call = lambda: _lib.check(L.mpreid_gemm_f16_split_nt(A.data_ptr(), W.data_ptr(), out.data_ptr(), bias.data_ptr(), rows_pad, N,   # noqa: E731
                                                         kseg, 2.0 ** -13, epi, _lib.stream_ptr()), "gemm")
    call()
    return _median([_ms(call) for _ in range(reps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--configs", default="")
    a = ap.parse_args()
    configs = [tuple(int(v) for v in c.split(",")) for c in a.configs.split(";")] if a.configs else CONFIGS
    L = _lib.load()
    base = dict(synth.VIT_B16)
    imgs = torch.from_numpy(synth.synthetic_images(a.batch, 256, 128, seed=3)).cuda()
    dense = ops.VitEncoder(base, synth.vit_state_dict(base, seed=7), (256, 128), ws_tag="bench_dense")
    dense(imgs)
    rows = a.batch * 129
    W = base["width"]
    for E, K, ML in configs:
        cfg = dict(base, num_experts=E, top_k=K, moe_layers=ML)
        sd = synth.vit_moe_state_dict(cfg, seed=7, std=0.02, ln_jitter=0.0)
        enc = ops.VitEncoder(cfg, sd, (256, 128), ws_tag="bench_moe")
        enc(imgs)
        torch.cuda.synchronize()
        tm, td = [], []
        for _ in range(a.steps):   # interleaved rounds in one process
            tm.append(_ms(lambda: enc(imgs)))
            td.append(_ms(lambda: dense(imgs)))
        # per-kernel times from the per-launch profile of one forward
        L.mpreid_profile_reset()
        L.mpreid_profile_enable(1)
        enc(imgs)
        torch.cuda.synchronize()
        L.mpreid_profile_enable(0)
        ents = (_lib.ProfileEntry * 64)()
        n = L.mpreid_profile_query(ents, 64)
        per = {PROF[e.epilogue]: e.total_ms / e.launches for e in list(ents)[:n] if e.epilogue in PROF}
        res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "num_experts": E, "top_k": K, "moe_layers": ML,
               "moe_images_per_s": round(a.batch / _median(tm) * 1e3, 1), "dense_images_per_s": round(a.batch / _median(td) * 1e3, 1),
               "tower_kernel_ms": {k: round(v, 4) for k, v in per.items()}}
        # The grouped GEMMs' rate, through the unit seams so that the slot count is known on the host: block 0's gate and experts,
        # h ~ N(0, 1) rows routed by ops.moe_route, slots = the experts' counts padded to the 128-row tile, FC1 / FC2 timed by
        # the same per-launch profile.
        p0 = "transformer.resblocks.0."
        h = torch.randn((rows, W), generator=torch.Generator().manual_seed(5)).cuda()
        sel, wts, _ = ops.moe_route(h, torch.from_numpy(sd[p0 + "gate.weight"]), K)
        counts = torch.bincount(sel.flatten().long().cpu(), minlength=E)
        slots = int(((counts + 127) // 128 * 128).sum())
        layer, keep = ops.pack_moe_layer(*(np.stack([sd[f"{p0}experts.{e}.{nm}"] for e in range(E)])
                                           for nm in ("c_fc.weight", "c_fc.bias", "c_proj.weight", "c_proj.bias")))
        pairs, x = ops.split_pairs_f32(h), torch.zeros((rows, W), device="cuda")
        ops.moe_mlp(pairs, sel, wts, layer, x, E)
        torch.cuda.synchronize()
        L.mpreid_profile_reset()
        L.mpreid_profile_enable(1)
        for _ in range(7):
            ops.moe_mlp(pairs, sel, wts, layer, x, E)
        torch.cuda.synchronize()
        L.mpreid_profile_enable(0)
        n = L.mpreid_profile_query(ents, 64)
        seam = {PROF[e.epilogue]: e.total_ms / e.launches for e in list(ents)[:n] if e.epilogue in PROF}
        res["slots"] = slots
        rows_pad = (slots + 255) // 256 * 256
        for name, N, kseg, epi in (("fc1", 4 * W, W, 12), ("fc2", W, 4 * W, 11)):
            res[name + "_tflops"] = round(2.0 * slots * N * 3 * kseg / seam[name] / 1e9, 1)
            dms = dense_split_gemm_ms(L, rows_pad, N, kseg, epi, 7)
            res["dense_" + name + "_tflops_at_%d_rows" % rows_pad] = round(2.0 * rows_pad * N * 3 * kseg / dms / 1e9, 1)
        del layer, keep
        print(json.dumps(res), flush=True)
        del enc
        ops.release_workspaces("bench_moe_moe")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
