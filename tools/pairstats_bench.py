#!/usr/bin/env python3
"""pair_bucket_kernel (csrc/pairstats.hip) at Market-1501 and MSMT17 shape beside the existing one-pass ranking kernel,
ops.pair_select at the three default false-positive rates, and R1_mAP_eval.compute() with extra_metrics on against off.

    python tools/pairstats_bench.py [--out profiles/pairstats_bench.json] [--skip-msmt17] [--skip-compute]

Device events after a warm-up, one process.  The matrix holds euclidean_distance of seeded random unit rows (d = 128: the
distances crowd around 2, as normalised features do); bounds are 4096 / 64 evenly spaced thresholds over [0, 4]; filter off /
on.  Per leg: mpreid_pair_bucket_counts ms and 4*nq*ng bytes over that time, and mpreid_eval_rank_positions(_cam) on the same
matrix, alternating in the same process, with the ratio of the two.  pair_select: host wall time of one call (its rounds
synchronise) and the number of passes it made.  No rate is fixed in advance and none is a gate; a leg that was not run is
written as "not measured"."""
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
from utils.metrics import DEFAULT_ROC_FPRS, R1_mAP_eval  # noqa: E402

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
    qf = ops.l2_normalize(torch.randn((nq, 128), device=dev, generator=g))
    gf = ops.l2_normalize(torch.randn((ng, 128), device=dev, generator=g))
    dist = ops.euclidean_distance(qf, gf)
    del qf, gf
    lab = [torch.from_numpy(a).to(dev) for a in (pids[:nq], pids[nq:], cams[:nq], cams[nq:])]
    rcap = int(np.unique(pids[nq:], return_counts=True)[1].max())
    pos = torch.empty((nq, rcap), dtype=torch.int32, device=dev)
    pcnt = torch.empty(nq, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    nbytes = 4.0 * nq * ng
    out = {"nq": nq, "ng": ng, "matrix_bytes": nbytes, "legs": []}

    def positions(cam):
        if cam:
            _lib.check(L.mpreid_eval_rank_positions_cam(ptr(dist), dist.stride(0), nq, ng, ptr(lab[0]), ptr(lab[1]), ptr(lab[2]),
                                                        ptr(lab[3]), rcap, ptr(pos), ptr(pcnt), _lib.stream_ptr()), "positions_cam")
        else:
            _lib.check(L.mpreid_eval_rank_positions(ptr(dist), dist.stride(0), nq, ng, ptr(lab[0]), ptr(lab[1]), rcap, ptr(pos),
                                                    ptr(pcnt), _lib.stream_ptr()), "positions")

    for nb in (4096, 64):
        bk = ops.dist_keys(np.linspace(0.0, 4.0, nb).astype(np.float32))
        bounds = torch.from_numpy(bk.view(np.int32)).to(dev)
        counts = torch.empty((2, nb + 1), dtype=torch.int64, device=dev)
        for cam in (False, True):
            qc, gc = (lab[2], lab[3]) if cam else (None, None)

            def pairs():
                _lib.check(L.mpreid_pair_bucket_counts(ptr(dist), dist.stride(0), nq, ng, ptr(lab[0]), ptr(lab[1]), ptr(qc),
                                                       ptr(gc), ptr(bounds), nb, 0, ptr(counts), _lib.stream_ptr()), "pairs")
            pairs()
            c = counts.cpu().numpy()
            a_ms, b_ms = [], []
            for _ in range(3):                                       # alternating
                a_ms.append(timed(pairs, reps=3)["median_ms"])
                b_ms.append(timed(lambda: positions(cam), reps=3)["median_ms"])
            a, b = sorted(a_ms)[1], sorted(b_ms)[1]
            leg = {"n_bounds": nb, "filter": cam, "pair_bucket_counts_ms": a_ms, "pair_bucket_counts_GBs": nbytes / a / 1e6,
                   "eval_rank_positions_ms": b_ms, "eval_rank_positions_GBs": nbytes / b / 1e6,
                   "ratio_to_eval_rank_positions": a / b, "non_empty_buckets": int((c > 0).sum()),
                   "pairs_counted": int(c.sum())}
            out["legs"].append(leg)
            print("%-10s B=%-4d filter=%-5s pair_bucket_counts %.3f ms (%.0f GB/s of 4*nq*ng)  positions kernel %.3f ms "
                  "(%.0f GB/s)  ratio %.2f  non-empty buckets %d" % (name, nb, cam, a, leg["pair_bucket_counts_GBs"], b,
                                                                   leg["eval_rank_positions_GBs"], a / b,
                                                                   leg["non_empty_buckets"]), flush=True)
    # pair_select at the default rates: wall time (the rounds read small count arrays back) and passes over the matrix
    passes = {"n": 0}
    real = ops.pair_bucket_counts

    def counting(*a, **k):
        passes["n"] += 1
        return real(*a, **k)
    ops.pair_bucket_counts = counting
    try:
        sel = []
        for cam in (False, True):
            qc, gc = (lab[2], lab[3]) if cam else (None, None)
            ops.pair_select(dist, lab[0], lab[1], qc, gc, fprs=DEFAULT_ROC_FPRS)
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                passes["n"] = 0
                t0 = time.perf_counter()
                r = ops.pair_select(dist, lab[0], lab[1], qc, gc, fprs=DEFAULT_ROC_FPRS)
                ts.append((time.perf_counter() - t0) * 1e3)
            sel.append({"filter": cam, "wall_ms": ts, "passes": passes["n"], "tau": [float(t) for t in r["tau"]],
                        "tp": r["tp"].tolist(), "fp": r["fp"].tolist(), "P": r["P"], "Nn": r["Nn"]})
            print("%-10s pair_select filter=%-5s %s ms, %d passes" % (name, cam, ["%.2f" % t for t in ts], passes["n"]),
                  flush=True)
        out["pair_select"] = sel
    finally:
        ops.pair_bucket_counts = real
    return out


def compute_leg(nq, ng, dev):
    f, pid = synth.clustered_features(nq + ng, 1280, 3.5, seed=2)
    ft = torch.from_numpy(f).to(dev)
    cam = np.zeros(nq + ng, np.int64)
    res = {False: [], True: []}
    for rep in range(4):                              # alternating; the first round is the warm-up
        for extra in (False, True):
            ev = R1_mAP_eval(nq, feat_norm=True)
            ev.extra_metrics = extra
            ev.pair_hist_bins = 100 if extra else 0
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
                res[extra].append((time.perf_counter() - t0) * 1e3)
    print("compute() at %d x %d: extra_metrics off %s ms, on (3 rates + 100 bins) %s ms"
          % (nq, ng, ["%.1f" % t for t in res[False]], ["%.1f" % t for t in res[True]]), flush=True)
    return {"nq": nq, "ng": ng, "extra_metrics_off_ms": res[False], "extra_metrics_on_ms": res[True], "pair_hist_bins": 100}


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pairstats_bench.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    name = C.create_string_buffer(128)
    _lib.check(_lib.load().mpreid_device_info(name, 128, None, None), "mpreid_device_info")
    result = {"device": name.value.decode(), "kernel": {}, "compute": "not measured"}
    for shape, (nq, ng) in SHAPES.items():
        if shape == "msmt17" and "--skip-msmt17" in argv:
            result["kernel"][shape] = "not measured"
            continue
        result["kernel"][shape] = kernel_legs(shape, nq, ng, dev)
        torch.cuda.empty_cache()
    if "--skip-compute" not in argv:
        result["compute"] = compute_leg(*SHAPES["market1501"], dev)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
