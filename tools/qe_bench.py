#!/usr/bin/env python3
"""Query expansion in feature space (ops.expand_features: csrc/qexpand.hip behind ops.search_topk) at Market-1501 shape
(N = 19 281, D = 1280) and at N = 100 000, D = 768, k = 10, alpha = 3.

    python tools/qe_bench.py [--out profiles/qe_bench.json] [--skip-100k]

Device events after a warm-up, seeded clustered features generated on the device, one process.  Per shape: milliseconds of
the neighbour search (l2_normalize + search_topk of the stack against itself, default chunk) and of the aggregation kernel
(mpreid_qe_aggregate_f32, timed over windows of several launches), and the aggregation's ALGORITHMIC bytes -- rows * kk * D * 4
gathered, rows * D * 4 written, the lists -- over its time, against the 6.29 TB/s copy rate measured on this chip.  Rows that
many lists name are served from the caches, so that figure is a rate of bytes asked for, not of HBM traffic.  Rows 0-7 of the
timed result are compared with the host definition bit for bit.  Nothing here is a gate; a leg that was not run is written as
"not measured"."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mp-reid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mpreid import _lib, ops  # noqa: E402
from utils.metrics import qe_aggregate  # noqa: E402

COPY_RATE_GBS = 6290.0
SHAPES = {"market1501": (19281, 1280), "n100k_d768": (100000, 768)}
K, ALPHA = 10, 3.0


def timed(fn, reps=5, inner=1):
    """median / min / max over `reps` event windows of `inner` calls each, per call, after a warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"min_ms": min(ts), "median_ms": sorted(ts)[len(ts) // 2], "max_ms": max(ts), "reps": reps, "calls_per_window": inner}


def features(n, d, dev, per_id=20, sigma=0.5, seed=77):
    """clustered raw features on the device: n / per_id centroids ~ N(0, I), samples = centroid + sigma N(0, I), random lengths"""
    g = torch.Generator(device=dev).manual_seed(seed)
    cent = torch.randn((max(n // per_id, 1), d), device=dev, generator=g)
    pid = torch.randint(0, cent.shape[0], (n,), device=dev, generator=g)
    x = cent[pid] + sigma * torch.randn((n, d), device=dev, generator=g)
    return (x * (0.5 + 3.0 * torch.rand((n, 1), device=dev, generator=g))).contiguous()


def shape_leg(name, n, d, dev):
    f = features(n, d, dev)

    def search():
        unit = ops.l2_normalize(f)
        return ops.search_topk(unit, unit, K)
    idx, val, cnt = search()
    out = torch.empty_like(f)
    ops.qe_aggregate(f, idx, val, cnt, ALPHA, out=out)
    idx8 = idx[:8].cpu().numpy()
    rows8 = np.unique(idx8[idx8 >= 0])                                   # the host definition on the rows that rows 0-7 name
    want = qe_aggregate(f[torch.from_numpy(rows8).to(dev).long()].cpu().numpy(), np.searchsorted(rows8, idx8),
                        val[:8].cpu().numpy(), cnt[:8].cpu().numpy(), ALPHA)
    assert np.array_equal(out[:8].cpu().numpy().view(np.uint32), want.view(np.uint32)), "rows 0-7 differ from the host definition"
    kk = int(cnt.sum().item())
    named = int(torch.unique(idx).numel())
    t_search = timed(search, reps=3)
    t_agg = timed(lambda: ops.qe_aggregate(f, idx, val, cnt, ALPHA, out=out), reps=7, inner=20)
    nbytes = 4.0 * kk * d + 4.0 * n * d + 8.0 * n * K + 4.0 * n
    rate = nbytes / t_agg["median_ms"] / 1e6
    leg = {"n": n, "d": d, "k": K, "alpha": ALPHA, "list_entries": kk, "distinct_rows_named": named,
           "search_chunk": max((256 << 20) // (4 * n), 1), "search": t_search, "aggregate": t_agg,
           "aggregate_algorithmic_bytes": nbytes, "aggregate_GBs": rate, "fraction_of_copy_rate": rate / COPY_RATE_GBS,
           "source_bytes": 4.0 * n * d}
    print("%-11s N = %d, D = %d, k = %d: search %.1f ms, aggregate %.3f ms (min %.3f, max %.3f): %.0f MB asked for -> %.0f GB/s, "
          "%.0f %% of the copy rate (the %.0f MB of source rows are named %.1f times each)"
          % (name, n, d, K, t_search["median_ms"], t_agg["median_ms"], t_agg["min_ms"], t_agg["max_ms"], nbytes / 1e6, rate,
             100 * rate / COPY_RATE_GBS, 4.0 * n * d / 1e6, kk / max(named, 1)), flush=True)
    return leg


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "qe_bench.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    name = C.create_string_buffer(128)
    _lib.check(_lib.load().mpreid_device_info(name, 128, None, None), "mpreid_device_info")
    result = {"device": name.value.decode(), "copy_rate_GBs": COPY_RATE_GBS, "shapes": {}}
    for shape, (n, d) in SHAPES.items():
        if shape == "n100k_d768" and "--skip-100k" in argv:
            result["shapes"][shape] = "not measured"
            continue
        result["shapes"][shape] = shape_leg(shape, n, d, dev)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
