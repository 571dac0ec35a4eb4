"""Host definitions of the extra metrics (utils/metrics.py: pair_counts, tpr_at_fpr, eval_metrics; mpreid.ops: dist_keys)
against plain Python loops written from the definition, on inputs small enough to read: ties, -0.0, non-finite entries, a
query without a positive, a single pid (no negative pair), the camera filter on and off.  No GPU."""
import math
import struct

import numpy as np
import pytest

from mpreid import ops
from utils import metrics


def _key(x):
    """the 32-bit key of a float32, from the definition (include/mpreid.h)"""
    x = float(np.float32(x)) + 0.0
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def _pairs(d, qp, gp, qc, gc, cam):
    """(positive keys, negative keys) of the kept pairs, by a double loop"""
    pos, neg = [], []
    for i in range(d.shape[0]):
        for j in range(d.shape[1]):
            if not math.isfinite(float(d[i, j])):
                continue
            if cam and qp[i] == gp[j] and qc[i] == gc[j]:
                continue
            (pos if qp[i] == gp[j] else neg).append(_key(d[i, j]))
    return pos, neg


def _cases():
    rng = np.random.default_rng(7)
    d = (np.round(rng.random((6, 17)) * 8) / 8).astype(np.float32)          # eighths: ties everywhere
    d[0, 0], d[1, 3], d[2, 5], d[3, 1], d[4, 4] = -0.0, 0.0, -0.25, np.inf, np.nan
    qp, gp = rng.integers(0, 4, 6), rng.integers(0, 4, 17)
    qp[5] = 99                                                               # a query without a positive
    qc, gc = rng.integers(0, 2, 6), rng.integers(0, 2, 17)
    yield "ties", d, qp, gp, qc, gc
    yield "one_pid", d[:3, :5].copy(), np.zeros(3, np.int64), np.zeros(5, np.int64), qc[:3], gc[:5]   # Nn == 0
    qp2, gp2 = np.array([1, 2]), np.array([1, 1, 2, 3])
    yield "all_junk", d[:2, :4].copy(), qp2, gp2, np.array([0, 0]), np.array([0, 0, 1, 1])  # query 0: every pid hit junk


@pytest.mark.parametrize("cam", [False, True])
def test_pair_counts_against_the_double_loop(cam):
    thr = np.array([-0.5, -0.0, 0.125, 0.5, 0.875, 1.0, 3.0], np.float32)
    for name, d, qp, gp, qc, gc in _cases():
        pos, neg = _pairs(d, qp, gp, qc, gc, cam)
        got = metrics.pair_counts(d, thr, qp, gp, qc, gc, remove_same_cam=cam)
        assert got["P"] == len(pos) and got["Nn"] == len(neg), name
        assert got["tp"].dtype == np.int64 and got["fp"].dtype == np.int64
        for b, t in enumerate(thr):
            assert got["tp"][b] == sum(k <= _key(t) for k in pos), (name, b)
            assert got["fp"][b] == sum(k <= _key(t) for k in neg), (name, b)
        hp, hn = metrics.pair_histograms(got)
        assert hp.sum() == len(pos) and hn.sum() == len(neg) and hp.shape == (thr.size + 1,)
        assert hp[0] == got["tp"][0] and hn[-1] == len(neg) - got["fp"][-1]
    with pytest.raises(ValueError):
        metrics.pair_counts(d, [0.5, 0.5], qp, gp)
    with pytest.raises(ValueError):
        metrics.pair_counts(d, [0.0, -0.0], qp, gp)          # equal keys
    if cam:
        with pytest.raises(ValueError):
            metrics.pair_counts(d, [0.5], qp, gp, None, None, remove_same_cam=True)


@pytest.mark.parametrize("cam", [False, True])
def test_tpr_at_fpr_budget_rule(cam):
    for name, d, qp, gp, qc, gc in _cases():
        pos, neg = _pairs(d, qp, gp, qc, gc, cam)
        neg_sorted = sorted(neg)
        Nn = len(neg)
        budgets = sorted({0, 1, 3, max(Nn - 1, 0), Nn, Nn + 5})
        got = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam, max_fp=budgets)
        assert got["P"] == len(pos) and got["Nn"] == Nn and got["fprs"] is None
        for i, m in enumerate(budgets):
            if m >= Nn:                                   # everything accepted
                assert np.isposinf(got["tau"][i]) and got["tp"][i] == len(pos) and got["fp"][i] == Nn
                continue
            tk = neg_sorted[m]                            # the (m + 1)-th smallest negative, with multiplicity
            assert _key(got["tau"][i]) == tk
            assert got["tp"][i] == sum(k < tk for k in pos) and got["fp"][i] == sum(k < tk for k in neg)
            assert got["fp"][i] <= m
            if neg_sorted.count(tk) == 1:
                assert got["fp"][i] == m
            # the most permissive threshold with at most m false positives: accepting the ties at tau breaks the budget
            assert sum(k <= tk for k in neg) > m
        if len(pos):
            assert np.array_equal(got["tpr"], got["tp"] / np.float64(len(pos)))
        else:
            assert np.isnan(got["tpr"]).all()
        if Nn:
            assert np.array_equal(got["fpr"], got["fp"] / np.float64(Nn))
        # rates: m = int(floor(float64(f) * Nn))
        fprs = [0.0, 1e-2, 0.3, 1.0]
        by_rate = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam, fprs=fprs)
        assert by_rate["budgets"].tolist() == [int(np.floor(np.float64(f) * Nn)) for f in fprs]
        again = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam, max_fp=by_rate["budgets"])
        for k in ("tp", "fp"):
            assert np.array_equal(by_rate[k], again[k])
        assert by_rate["tau"].tobytes() == again["tau"].tobytes()
    default = metrics.tpr_at_fpr(d, qp, gp)
    assert default["fprs"].tolist() == [1e-4, 1e-3, 1e-2]


def test_dist_keys_monotone_and_invertible():
    vals = np.array([-np.inf, -3.5, -1.0, -1e-38, -1.4e-45, -0.0, 0.0, 1.4e-45, 1e-38, 1.17549435e-38, 0.125, 0.375, 1.0,
                     1.0000001, 2.0, 3.4e38, np.inf], np.float32)
    keys = ops.dist_keys(vals)
    assert keys.dtype == np.uint32 and keys.shape == vals.shape
    assert keys.tolist() == [_key(v) for v in vals]
    for a in range(vals.size):
        for b in range(vals.size):
            assert (keys[a] < keys[b]) == bool(vals[a] < vals[b]), (vals[a], vals[b])
            assert (keys[a] == keys[b]) == bool(vals[a] == vals[b])          # -0 == +0
    back = ops.keys_to_dist(keys)
    assert back.dtype == np.float32 and np.array_equal(back, vals)
    assert back[5].tobytes() == np.float32(0.0).tobytes()                  # a zero comes back as +0
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    f = f[~np.isnan(f)]
    k = ops.dist_keys(f)
    o = np.argsort(f, kind="stable")
    assert np.all(np.diff(k[o].astype(np.int64)) >= 0)
    assert np.array_equal(ops.keys_to_dist(k), f + np.float32(0))
    assert ops.dist_keys(np.float32(0.5)).shape == () and ops.keys_to_dist(ops.dist_keys(np.float32(0.5))) == 0.5


@pytest.mark.parametrize("name, cam", [("eval_func.npz", False), ("eval_func_samecam.npz", True)])
def test_eval_metrics_on_the_goldens(golden, name, cam):
    g = golden(name)
    d = g["d"] if "d" in g.files else golden("distance.npz")["euclid"]
    qp, gp, qc, gc = g["q_pid"], g["g_pid"], g["q_cam"], g["g_cam"]
    cmc, mAP = metrics.eval_func(d, qp, gp, qc, gc, remove_same_cam=cam)
    assert np.array_equal(cmc, g["cmc"]) and float(mAP) == float(g["mAP"])
    m = metrics.eval_metrics(d, qp, gp, qc, gc, remove_same_cam=cam)
    assert m["cmc"].dtype == cmc.dtype and np.array_equal(m["cmc"], cmc)
    assert np.float64(m["mAP"]).tobytes() == np.float64(mAP).tobytes()
    assert abs(np.mean(m["all_AP"]) - mAP) < 1e-12
    # INP against the cumulative-match formulation on the argsorted row
    inp, first, valid = [], [], []
    for i in range(d.shape[0]):
        order = np.argsort(d[i], kind="stable")
        if cam:
            order = order[~((gp[order] == qp[i]) & (gc[order] == qc[i]))]
        matches = (gp[order] == qp[i]).astype(np.int64)
        valid.append(bool(matches.any()))
        if not matches.any():
            first.append(-1)
            continue
        last = int(np.nonzero(matches)[0][-1])
        first.append(int(np.nonzero(matches)[0][0]))
        inp.append(np.cumsum(matches)[last] / (last + 1.0))
    assert np.array_equal(m["valid"], valid) and np.array_equal(m["first_hit"], first)
    assert np.array_equal(m["all_INP"], np.array(inp, np.float64))
    assert np.float64(m["mINP"]).tobytes() == np.float64(np.mean(np.array(inp, np.float64))).tobytes()
    assert 0.0 < m["mINP"] <= 1.0 and m["all_AP"].shape == m["all_INP"].shape == (int(np.sum(valid)),)


def test_eval_metrics_tiny_by_hand():
    # query 0: relevant at positions 1 and 3 -> AP = (1/2 + 2/4) / 2, INP = 2/4; query 1 has no relevant item
    d = np.array([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1], [0.5, 0.5, 0.5, 0.5]], np.float32)
    qp, gp = np.array([7, 8, 9]), np.array([1, 7, 9, 7])
    m = metrics.eval_metrics(d, qp, gp, np.zeros(3, int), np.ones(4, int), max_rank=4)
    assert m["valid"].tolist() == [True, False, True] and m["first_hit"].tolist() == [1, -1, 2]
    assert m["all_INP"].tolist() == [0.5, 1.0 / 3.0] and m["all_AP"].tolist() == [0.5, 1.0 / 3.0]
    assert m["mINP"] == np.mean([0.5, 1.0 / 3.0])
    # the camera filter: gallery item 1 shares pid and camera with query 0 -> junk; the hit at column 3 moves up to 2
    m = metrics.eval_metrics(d, qp, gp, np.array([0, 0, 0]), np.array([1, 0, 1, 1]), max_rank=4, remove_same_cam=True)
    assert m["first_hit"].tolist() == [2, -1, 2] and m["all_INP"].tolist() == [1.0 / 3.0, 1.0 / 3.0]


def test_fp_tp_points_lie_on_sklearn_roc_curve():
    sk = pytest.importorskip("sklearn.metrics")
    _, d, qp, gp, qc, gc = next(_cases())
    keep = np.isfinite(d)
    same = (qp[:, None] == gp[None, :])
    scores, labels = -(d[keep] + np.float32(0)), same[keep]
    fpr, tpr, thr = sk.roc_curve(labels, scores, drop_intermediate=False)
    curve = {(round(float(a), 12), round(float(b), 12)) for a, b in zip(fpr, tpr)}
    data_thr = np.unique(d[keep] + np.float32(0))
    c = metrics.pair_counts(d, data_thr, qp, gp)
    for b in range(data_thr.size):
        assert (round(c["fp"][b] / c["Nn"], 12), round(c["tp"][b] / c["P"], 12)) in curve


def test_evaluator_defaults_and_config_keys():
    from config import cfg_base
    ev = metrics.R1_mAP_eval(3)
    assert ev.extra_metrics is False and ev.roc_fprs == (1e-4, 1e-3, 1e-2) and ev.pair_hist_bins == 0
    assert ev.pair_hist_range == (0.0, 4.0) and ev.last_metrics is None
    sp = metrics.R1_mAP_eval_splits([([0], [1])])
    assert sp.extra_metrics is False and sp.last_metrics is None
    assert cfg_base.TEST.EXTRA_METRICS is False and list(cfg_base.TEST.ROC_FPRS) == [1e-4, 1e-3, 1e-2]
    assert cfg_base.TEST.PAIR_HIST_BINS == 0 and list(cfg_base.TEST.PAIR_HIST_RANGE) == [0.0, 4.0]
    c = cfg_base.clone()
    c.defrost()
    c.merge_from_list(["TEST.EXTRA_METRICS", "True", "TEST.PAIR_HIST_BINS", "40", "TEST.ROC_FPRS", "[0.01,0.1]"])
    from processor.processor import configure_extra_metrics
    configure_extra_metrics(c, ev)
    assert ev.extra_metrics is True and ev.pair_hist_bins == 40 and ev.roc_fprs == (0.01, 0.1)
    assert metrics._hist_edges(0, (0.0, 4.0)) is None
    e = metrics._hist_edges(40, (0.0, 4.0))
    assert e.dtype == np.float32 and e.shape == (41,) and e[0] == 0.0 and e[-1] == 4.0
    for bad in ((-1, (0.0, 4.0)), (4096, (0.0, 4.0)), (4, (1.0, 1.0)), (4000, (1.0, 1.0 + 1e-6))):
        with pytest.raises(ValueError):
            metrics._hist_edges(*bad)


def test_bound_and_budget_validation_needs_no_gpu():
    for bad in ([], list(range(4097)), [3, 3], [5, 4], [[1, 2]], [0.5], [-1], [2 ** 32]):
        with pytest.raises(ValueError):
            ops._check_bound_keys(np.asarray(bad))
    assert ops._check_bound_keys([0, 7, 0xFFFFFFFF]).dtype == np.uint32
    for bad in ([], [-1], list(range(17)), [0.5]):
        with pytest.raises(ValueError):
            ops._check_budgets(np.asarray(bad))
