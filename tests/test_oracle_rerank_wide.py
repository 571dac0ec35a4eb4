"""CPU oracle against the reference at k1 / k2 beyond 256 (tests/golden/rerank_wide.npz, written by
tests/golden/make_goldens_rerank_wide.py from the reference itself): the yardstick of the WIDE re-ranking algorithm.

Same bars as test_oracle.py::test_rerank_unselected_seeds_vs_reference: bit equality when both sides are fed the same
distance matrix; against the reference as called (its own distance GEMM) frac(|d| > 1e-5) <= 1e-4 and max <= 5e-4;
mAP within 1e-5, CMC within 1e-4."""
import hashlib

import numpy as np
import pytest

from oracle import oracle as orc

RR_FRAC, RR_MAX = 1e-4, 5e-4   # tests/test_gpu_rerank.py


def wide_case(g, row):
    """(tag, features, pids, nq, k1, k2, lambda) of one row of rerank_wide.npz, regenerated from the seed recipe"""
    from mpreid import synth
    seed, N, D, sigma, per_id, k1, k2, lam = row
    seed, N, D, per_id, k1, k2 = int(seed), int(N), int(D), int(per_id), int(k1), int(k2)
    raw, pid = synth.clustered_features(N, D, float(sigma), seed=seed, per_id=per_id, normalize=False)
    feat = orc.l2_normalize(raw)
    assert hashlib.sha256(feat.tobytes()).hexdigest() == str(g[f"w{seed}_feat_sha"]), "input drift: seeded features differ"
    return f"w{seed}", feat, pid, N // 5, k1, k2, float(lam)


def check_against_reference(g, tag, pid, nq, got, got_same_d):
    """got: result on the features; got_same_d: result fed the oracle's distance matrix through local_distmat/only_local"""
    idx = g[f"{tag}_idx"].astype(np.int64)
    d = np.abs(got.reshape(-1)[idx] - g[f"{tag}_val"])
    print(tag, "as called: frac(|d| > 1e-5) = %.3g, max = %.3g" % ((d > 1e-5).mean(), d.max()))
    assert (d > 1e-5).mean() <= RR_FRAC and d.max() <= RR_MAX, (tag, (d > 1e-5).mean(), d.max())
    cmc, mAP = orc.eval_func(got, pid[:nq], pid[nq:])
    assert abs(mAP - float(g[f"{tag}_mAP"])) <= 1e-5 and np.abs(cmc - g[f"{tag}_cmc"]).max() <= 1e-4, tag
    assert np.array_equal(got_same_d.reshape(-1)[idx], g[f"{tag}_sameD_val"]), tag
    assert hashlib.sha256(np.ascontiguousarray(got_same_d).tobytes()).hexdigest() == str(g[f"{tag}_sameD_sha"]), tag


@pytest.mark.parametrize("row", range(4))
def test_oracle_rerank_wide_vs_reference(golden, row):
    g = golden("rerank_wide.npz")
    assert len(g["cases"]) == 4
    tag, feat, pid, nq, k1, k2, lam = wide_case(g, g["cases"][row])
    assert max(k1 + 1, k2) > 256, "every case lies beyond the limit of the LDS-resident algorithms"
    got = orc.re_ranking(feat[:nq], feat[nq:], k1, k2, lam)
    d_or = orc.euclidean_distance(feat, feat)
    got2 = orc.re_ranking(feat[:nq], feat[nq:], k1, k2, lam, local_distmat=d_or, only_local=True)
    check_against_reference(g, tag, pid, nq, got, got2)
    m = g[f"{tag}_measured"]   # the generator's full-matrix figures obey the same bounds
    assert m[0] <= RR_FRAC and m[1] <= RR_MAX and m[2] == 0.0 and m[4] <= 1e-5 and m[5] <= 1e-4, (tag, m)
