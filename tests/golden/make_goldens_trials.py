#!/usr/bin/env python3
"""Generate tests/golden/eval_trials.npz: the REFERENCE's eval_func on the sub-matrices of one pool x pool distance matrix,
split by split -- the multi-trial evaluation (VehicleID protocol, reference test.py:46-63) as the reference computes it.

Run in the build container only (needs /root/reference), like make_goldens_samecam.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_trials.py

The reference's eval_func is loaded from its source text in place (make_goldens_samecam.load_eval_funcs: as shipped, and
with its same-camera line :54 restored in memory).  Nothing of the reference is copied into this repository: the fixture
holds the input (a tie-free 240 x 240 matrix, pool pids / camids, the splits) and the reference's outputs per split.

  (i)  four VehicleID trials (datasets.make_dataloader.vehicleid_trial_splits: one gallery image per identity);
  (ii) three general splits: several relevant gallery items per query, a query without any, one split whose queries also
       sit in its gallery, one gallery list in descending order; recorded as shipped AND under the restored filter.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (HERE, os.path.join(ROOT, "mp-reid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_goldens_samecam import load_eval_funcs  # noqa: E402

N, IDS, CAMS = 240, 40, 3


def make_input():
    from datasets.make_dataloader import vehicleid_trial_splits
    rng = np.random.default_rng(23)
    d = (rng.permutation(N * N).astype(np.float32) / np.float32(N * N)).reshape(N, N)     # distinct values: no ties at all
    pids = rng.permutation(np.repeat(np.arange(IDS), N // IDS)).astype(np.int64)
    camids = rng.integers(0, CAMS, N).astype(np.int64)
    trials = vehicleid_trial_splits(pids, trials=4, seed=5)
    pids_g = pids.copy()
    pids_g[0] = 10_000                                      # general splits: pool item 0 is a query without any match
    general = []
    for k in range(3):
        g = np.sort(rng.choice(np.arange(1, N), 120, replace=False))
        rest = np.setdiff1d(np.arange(1, N), g)
        q = np.sort(rng.choice(rest, 60, replace=False))
        if k == 1:
            q = np.sort(np.concatenate([q, g[:20]]))        # queries that also sit in their own gallery list
        if k == 2:
            g = g[::-1].copy()                              # a gallery list in descending pool order
        general.append((np.concatenate([[0], q]).astype(np.int64), g.astype(np.int64)))
    return d, pids, pids_g, camids, trials, general


def run(fn, d, pids, camids, q, g):
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, mAP = fn(d[np.ix_(q, g)], pids[q], pids[g], camids[q], camids[g])
    assert cmc.dtype == np.float32
    return cmc, np.float64(mAP)


def main():
    filtered, shipped = load_eval_funcs()
    d, pids, pids_g, camids, trials, general = make_input()
    assert np.unique(d).size == d.size, "the matrix must be tie-free (np.argsort is unstable)"
    out = dict(d=d, pids=pids, pids_general=pids_g, camids=camids)
    for i, (q, g) in enumerate(trials):
        cmc, mAP = run(shipped, d, pids, camids, q, g)
        out.update({f"t{i}_q": q, f"t{i}_g": g, f"t{i}_cmc": cmc, f"t{i}_mAP": mAP})
    assert len({float(out[f"t{i}_mAP"]) for i in range(4)}) > 1, "the trials must differ"
    for i, (q, g) in enumerate(general):
        per_q = (pids_g[g][None, :] == pids_g[q][:, None]).sum(1)
        assert per_q[0] == 0 and np.median(per_q[1:]) >= 2, "one query without a match, several relevant items for the others"
        cmc, mAP = run(shipped, d, pids_g, camids, q, g)
        cmc_f, mAP_f = run(filtered, d, pids_g, camids, q, g)
        assert mAP != mAP_f, "the filter must matter on the general splits"
        out.update({f"g{i}_q": q, f"g{i}_g": g, f"g{i}_cmc": cmc, f"g{i}_mAP": mAP, f"g{i}_cmc_samecam": cmc_f,
                    f"g{i}_mAP_samecam": mAP_f})
    path = os.path.join(HERE, "eval_trials.npz")
    np.savez_compressed(path, **out)
    kib = os.path.getsize(path) / 1024
    assert kib < 300, kib
    print(f"eval_trials.npz: {kib:.0f} KiB; trial mAPs {[round(float(out[f't{i}_mAP']), 4) for i in range(4)]}, general mAPs "
          f"{[round(float(out[f'g{i}_mAP']), 4) for i in range(3)]} / filtered "
          f"{[round(float(out[f'g{i}_mAP_samecam']), 4) for i in range(3)]}")


if __name__ == "__main__":
    main()
