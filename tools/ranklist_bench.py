#!/usr/bin/env python3
"""rank_topk_kernel (csrc/ranklist.hip) at Market-1501 and MSMT17 shape, beside the existing one-pass ranking kernel, plus
ops.search_topk against the full matrix and R1_mAP_eval.compute() with and without ranked lists.

    python tools/ranklist_bench.py [--out profiles/ranklist_bench.json] [--skip-msmt17] [--skip-compute]

Device events after a warm-up, seeded random matrices, one process.  Per shape, k in (50, 1024) and filter off / on:
mpreid_rank_topk ms and 4*nq*ng bytes over that time (GB/s; the copy rate measured on this chip is 6.29 TB/s), and
mpreid_eval_rank_positions (mpreid_eval_rank_positions_cam with the filter) on the same matrix in the same run with the
ratio of the two.  Nothing here is a gate; a leg that was not run is written as "not measured"."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mp-reid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mpreid import _lib, ops, synth  # noqa: E402
from utils.metrics import R1_mAP_eval, rank_lists  # noqa: E402

COPY_RATE_GBS = 6290.0
SHAPES = {"market1501": (3368, 15913), "msmt17": (11659, 82161)}


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"min_ms": min(ts), "median_ms": sorted(ts)[len(ts) // 2], "max_ms": max(ts), "reps": reps}


def kernel_legs(name, nq, ng, dev):
    L = _lib.load()
    rng = np.random.default_rng(1234)
    pids = rng.integers(0, max(ng // 21, 1), size=nq + ng).astype(np.int64)
    cams = rng.integers(0, 6, size=nq + ng).astype(np.int64)
    g = torch.Generator(device=dev).manual_seed(4321)
    dist = torch.randn((nq, ng), device=dev, generator=g)
    lab = [torch.from_numpy(a).to(dev) for a in (pids[:nq], pids[nq:], cams[:nq], cams[nq:])]
    rcap = int(np.unique(pids[nq:], return_counts=True)[1].max())
    pos = torch.empty((nq, rcap), dtype=torch.int32, device=dev)
    pcnt = torch.empty(nq, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    nbytes = 4.0 * nq * ng
    out = {"nq": nq, "ng": ng, "matrix_bytes": nbytes, "legs": []}

    def positions(cam):
        if cam:
            _lib.check(L.mpreid_eval_rank_positions_cam(ptr(dist), dist.stride(0), nq, ng, ptr(lab[0]), ptr(lab[1]), ptr(lab[2]),
                                                        ptr(lab[3]), rcap, ptr(pos), ptr(pcnt), _lib.stream_ptr()), "positions_cam")
        else:
            _lib.check(L.mpreid_eval_rank_positions(ptr(dist), dist.stride(0), nq, ng, ptr(lab[0]), ptr(lab[1]), rcap, ptr(pos),
                                                    ptr(pcnt), _lib.stream_ptr()), "positions")

    d8 = dist[:8].cpu().numpy()
    for k in (50, 1024):
        for cam in (False, True):
            labels = lab if cam else None
            idx, val, cnt = ops.rank_topk(dist, k, labels=labels)          # host check of rows 0-7
            want = rank_lists(d8, k, pids[:8], pids[nq:], cams[:8], cams[nq:], remove_same_cam=cam)
            assert np.array_equal(idx[:8].cpu().numpy(), want[0]) and np.array_equal(cnt[:8].cpu().numpy(), want[2])
            assert np.array_equal(val[:8].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
            a = timed(lambda: ops.rank_topk(dist, k, labels=labels))
            b = timed(lambda: positions(cam))
            leg = {"k": k, "filter": cam, "rank_topk": a, "rank_topk_GBs": nbytes / a["median_ms"] / 1e6,
                   "fraction_of_copy_rate": nbytes / a["median_ms"] / 1e6 / COPY_RATE_GBS,
                   "eval_rank_positions": b, "ratio_to_eval_rank_positions": a["median_ms"] / b["median_ms"]}
            out["legs"].append(leg)
            print("%-10s k=%-4d filter=%-5s rank_topk %.3f ms (%.0f GB/s of 4*nq*ng, %.1f %% of the copy rate)  positions kernel "
                  "%.3f ms  ratio %.1f" % (name, k, cam, a["median_ms"], leg["rank_topk_GBs"],
                                           100 * leg["fraction_of_copy_rate"], b["median_ms"],
                                           leg["ratio_to_eval_rank_positions"]), flush=True)
    return out


def search_leg(nq, ng, d, dev, k=50):
    g = torch.Generator(device=dev).manual_seed(99)
    qf = ops.l2_normalize(torch.randn((nq, d), device=dev, generator=g))
    gf = ops.l2_normalize(torch.randn((ng, d), device=dev, generator=g))
    chunk = max((256 << 20) // (4 * nq), 1)

    def full():
        return ops.rank_topk(ops.euclidean_distance(qf, gf), k)

    def blocked():
        return ops.search_topk(qf, gf, k)
    a, b = full(), blocked()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    del a, b
    res = {"full": [], "search_topk": []}
    for _ in range(3):                                # alternating
        res["full"].append(timed(full, reps=2)["min_ms"])
        res["search_topk"].append(timed(blocked, reps=2)["min_ms"])
    out = {"nq": nq, "ng": ng, "d": d, "k": k, "default_chunk": chunk, "lists_equal": bool(same),
           "euclidean_distance_plus_rank_topk_ms": res["full"], "search_topk_ms": res["search_topk"]}
    print("search_topk %d x %d, d = %d, k = %d, chunk %d: full matrix + rank_topk %s ms, search_topk %s ms, equal lists: %s"
          % (nq, ng, d, k, chunk, ["%.1f" % t for t in res["full"]], ["%.1f" % t for t in res["search_topk"]], same), flush=True)
    return out


def compute_leg(nq, ng, dev):
    f, pid = synth.clustered_features(nq + ng, 1280, 3.5, seed=2)
    ft = torch.from_numpy(f).to(dev)
    cam = np.zeros(nq + ng, np.int64)
    res = {0: [], 50: []}
    for rep in range(4):                              # alternating; the first round is the warm-up
        for list_k in (0, 50):
            ev = R1_mAP_eval(nq, feat_norm=True)
            ev.rank_list_k = list_k
            ev.reset()
            for s in range(0, nq + ng, 512):
                ev.update((ft[s:s + 512], pid[s:s + 512], cam[s:s + 512]))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as nul:
                so, sys.stdout = sys.stdout, nul
                try:
                    ev.compute()
                finally:
                    sys.stdout = so
            if rep:
                res[list_k].append((time.perf_counter() - t0) * 1e3)
    print("compute() at %d x %d: rank_list_k = 0 %s ms, rank_list_k = 50 %s ms"
          % (nq, ng, ["%.1f" % t for t in res[0]], ["%.1f" % t for t in res[50]]), flush=True)
    return {"nq": nq, "ng": ng, "rank_list_k_0_ms": res[0], "rank_list_k_50_ms": res[50]}


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "ranklist_bench.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    name = C.create_string_buffer(128)
    _lib.check(_lib.load().mpreid_device_info(name, 128, None, None), "mpreid_device_info")
    result = {"device": name.value.decode(), "copy_rate_GBs": COPY_RATE_GBS, "kernel": {}, "search_topk": "not measured",
              "compute": "not measured"}
    for shape, (nq, ng) in SHAPES.items():
        if shape == "msmt17" and "--skip-msmt17" in argv:
            result["kernel"][shape] = "not measured"
            continue
        result["kernel"][shape] = kernel_legs(shape, nq, ng, dev)
        torch.cuda.empty_cache()
    if "--skip-msmt17" not in argv:
        result["search_topk"] = search_leg(*SHAPES["msmt17"], 1280, dev)
        torch.cuda.empty_cache()
    if "--skip-compute" not in argv:
        result["compute"] = compute_leg(*SHAPES["market1501"], dev)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
