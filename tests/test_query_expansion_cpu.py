"""Query expansion in feature space, host side: utils.metrics.expand_features / qe_aggregate (the numpy definition the GPU
path is compared with), their validation, and the config keys.  No GPU.

The definition is checked twice: against an independent float64 brute force (its own sort, its own sums -- same lists, rows
within a derived rounding bound) and, bit for bit, against a plain Python triple loop in np.float32.

Rounding bound of a row (u = 2^-24, the fp32 unit roundoff; kk list entries; float64 is taken as exact): s = fl(1 - d / 2)
carries one rounding, which w = s^alpha amplifies alpha times, and the alpha - 1 rounded products add alpha - 1 more:
|dw| <= (2 alpha - 1) u w.  Every term w * f is rounded once, the running sum at most kk times, the divide once.  To first
order: ||delta row||_2 <= (kk + 1 + 2 alpha) u * (sum_j w_j ||f_j||_2) / kk.  With np.power in place of the products the
weight's share is 16 ulp (the OpenCL full-profile bound for pow) plus the amplified rounding of s: 16 + alpha."""
import numpy as np
import pytest

U = 2.0 ** -24


def _clustered(n, d, seed, centres=6, spread=0.15):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    f = c[rng.integers(0, centres, n)] + spread * rng.standard_normal((n, d))
    return (f * (0.5 + rng.random((n, 1)) * 3.0)).astype(np.float32)      # raw rows of different lengths


def _unit_distmat(f):
    """squared distances of the L2-normalised rows, float32 (numpy; any plausible matrix serves the host definition)"""
    f = f.astype(np.float32)
    u = f / np.maximum(np.sqrt((f * f).sum(1, dtype=np.float32)), np.float32(1e-12))[:, None]
    sq = (u * u).sum(1, dtype=np.float32)
    return (sq[:, None] + sq[None, :] - np.float32(2) * (u @ u.T)).astype(np.float32)


def _brute_force64(f, dm, k, alpha):
    """float64, independent of the module: sorted() over (distance, index) tuples, math on Python floats"""
    n, d = f.shape
    kk = min(k, n)
    lists, out, scale = [], np.zeros((n, d)), np.zeros(n)
    for i in range(n):
        order = [j for _, j in sorted((float(dm[i, j]) + 0.0, j) for j in range(n))][:kk]
        lists.append(order)
        acc = np.zeros(d)
        for j in order:
            s = max(1.0 - 0.5 * float(dm[i, j]), 0.0)
            w = 1.0 if alpha == 0 else s ** alpha
            acc += w * f[j].astype(np.float64)
            scale[i] += w * float(np.linalg.norm(f[j].astype(np.float64)))
        out[i] = acc / kk
    return lists, out, scale / kk


def _triple_loop32(f, dm, k, alpha):
    """the definition spelled out: every operation on np.float32 scalars, one at a time"""
    n, d = f.shape
    kk = min(k, n)
    out = np.zeros((n, d), np.float32)
    for i in range(n):
        order = np.argsort(dm[i], kind="stable")[:kk]
        for e in range(d):
            acc = np.float32(0)
            for j in order:
                s = max(np.float32(1) - np.float32(0.5) * dm[i, j], np.float32(0))
                if alpha == 0:
                    w = np.float32(1)
                else:
                    w = s
                    for _ in range(alpha - 1):
                        w = np.float32(w * s)
                acc = np.float32(acc + np.float32(w * f[j, e]))
            out[i, e] = np.float32(acc / np.float32(kk))
    return out


@pytest.mark.parametrize("d", [1, 7, 64])
@pytest.mark.parametrize("alpha", [0, 1, 3, 2.5])
def test_definition_against_float64_brute_force(d, alpha):
    from utils.metrics import expand_features, rank_lists
    n, k = 60, 8
    f = _clustered(n, d, 100 + d)
    dm = _unit_distmat(f)
    got = expand_features(f, dm, k, alpha)
    assert got.dtype == np.float32 and got.shape == (n, d)
    lists, want, scale = _brute_force64(f, dm, k, alpha)
    assert rank_lists(dm, k)[0].tolist() == lists
    # integer alpha: (kk + 1 + 2 alpha) u as derived above; np.power: 16 ulp (the OpenCL full-profile bound for pow) + alpha u
    p = 2 * alpha if alpha == int(alpha) else 16 + alpha
    err = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    bound = (k + 1 + p) * U * scale
    print("alpha", alpha, "d", d, "largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert float(err.max()) > 0                     # (fp32 did round somewhere: the comparison is not vacuous)


@pytest.mark.parametrize("alpha", [0, 1, 3])
def test_definition_is_the_float32_triple_loop(alpha):
    from utils.metrics import expand_features
    for n, d, k in ((25, 5, 4), (12, 3, 1), (9, 2, 9)):
        f = _clustered(n, d, 7 * n + alpha)
        dm = _unit_distmat(f)
        got = expand_features(f, dm, k, alpha)
        assert got.view(np.uint32).tolist() == _triple_loop32(f, dm, k, alpha).view(np.uint32).tolist()


def test_alpha_zero_counts_orthogonal_neighbours_and_k_clamps():
    from utils.metrics import expand_features, qe_aggregate
    f = np.array([[1, 0], [0, 2], [-3, 0], [0.5, 0.5]], np.float32)
    dm = _unit_distmat(f)
    assert dm[0, 1] == 2.0 and dm[0, 2] == 4.0                      # s = 0 and s clamped from -1 to 0
    # k > N clamps to N: with alpha = 0 every row becomes the plain mean of all four raw rows, w = 1 also where s == 0
    got = expand_features(f, dm, 50, 0)
    mean = np.zeros(2, np.float32)
    for j in np.argsort(dm[0], kind="stable"):
        mean = mean + f[j]
    assert got[0].tolist() == (mean / np.float32(4)).tolist()
    assert np.allclose(got, f.mean(0)[None, :], atol=1e-6)
    # the same neighbours weigh nothing from alpha = 1 on
    one = expand_features(f, dm, 50, 1)
    s03 = max(np.float32(1) - np.float32(0.5) * dm[0, 3], np.float32(0))
    s00 = max(np.float32(1) - np.float32(0.5) * dm[0, 0], np.float32(0))
    assert one[0].tolist() == ((np.float32(0) + s00 * f[0] + s03 * f[3] + np.float32(0) * f[1] + np.float32(0) * f[2])
                               / np.float32(4)).tolist()
    assert np.array_equal(expand_features(f, dm, 4, 3), expand_features(f, dm, 1024, 3))
    # given lists: counts are clamped to [0, k], entries past them are ignored, an empty list gives zeros
    idx = np.array([[1, 0, -1], [2, 2, 2], [0, 1, 3], [9, 9, 9]], np.int64)
    dist = np.array([[0, 1, np.inf], [0.5, 0.5, 0.5], [3.0, 0, 0], [np.nan, 0, 0]], np.float32)
    got = qe_aggregate(f, idx, dist, np.array([2, 7, -3, 0]), 1)
    assert got[0].tolist() == ((f[1] + np.float32(0.5) * f[0]) / np.float32(2)).tolist()
    t = np.float32(0.75) * f[2]
    assert got[1].tolist() == (((t + t) + t) / np.float32(3)).tolist()       # duplicates count every time
    assert got[2].tolist() == [0, 0] and got[3].tolist() == [0, 0]


def test_validation_raises_value_error():
    from mpreid import ops
    from utils.metrics import expand_features, expand_features_device, qe_aggregate
    f = _clustered(6, 3, 1)
    dm = _unit_distmat(f)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            expand_features(f, dm, k)
    for alpha in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            expand_features(f, dm, 3, alpha)
        with pytest.raises(ValueError):
            qe_aggregate(f, np.zeros((6, 2), np.int64), np.zeros((6, 2), np.float32), np.full(6, 2), alpha)
    with pytest.raises(ValueError):
        expand_features(f, dm[:5], 3)
    with pytest.raises(ValueError):
        expand_features(f[0], dm, 3)
    with pytest.raises(ValueError):
        expand_features(np.zeros((6, 0), np.float32), dm, 3)
    with pytest.raises(ValueError):
        qe_aggregate(f, np.zeros((6, 2), np.int64), np.zeros((6, 3), np.float32), np.full(6, 2), 1)
    with pytest.raises(ValueError):
        qe_aggregate(f, np.zeros((6, 2), np.int64), np.zeros((6, 2), np.float32), np.full(5, 2), 1)
    # the device entry points validate before they look for a device: ValueError with or without one
    import torch
    q, g = torch.zeros((2, 3)), torch.zeros((4, 3))
    for kw in (dict(k=0), dict(k=1025), dict(k=2, alpha=-1.0), dict(k=2, alpha=float("nan")), dict(k=2, alpha=float("inf")),
               dict(k=2, times=-1), dict(k=2, times=1.5)):
        with pytest.raises(ValueError):
            ops.expand_features(q, g, **kw)
        with pytest.raises(ValueError):
            expand_features_device(q.numpy(), g.numpy(), **kw)
    with pytest.raises(ValueError):
        ops.expand_features(q, torch.zeros((4, 5)), 2)
    with pytest.raises(ValueError):
        ops.expand_features(q[0], g, 2)
    with pytest.raises(ValueError):
        ops.expand_features(torch.zeros((2, 0)), torch.zeros((4, 0)), 2)
    i32, f32 = torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 2))
    c32 = torch.zeros(4, dtype=torch.int32)
    for args in ((g, i32, f32, c32, -1.0), (g, i32.long(), f32, c32, 1.0), (g, i32, f32.double(), c32, 1.0),
                 (g, i32, f32[:3], c32, 1.0), (g, i32, f32, c32[:3], 1.0), (g[0], i32, f32, c32, 1.0),
                 (g.double(), i32, f32, c32, 1.0)):
        with pytest.raises(ValueError):
            ops.qe_aggregate(*args)
    with pytest.raises(ValueError):
        ops.qe_aggregate(g, i32, f32, c32, 1.0, out=torch.zeros((3, 3)))


def test_evaluator_attributes_and_validation_order():
    from utils.metrics import R1_mAP_eval, R1_mAP_eval_splits
    for ev in (R1_mAP_eval(4), R1_mAP_eval_splits([([0], [1])])):
        assert (ev.qe_k, ev.qe_alpha, ev.qe_times) == (0, 3.0, 1)
    ev = R1_mAP_eval(4)
    ev.reset()
    for k, alpha, times in ((1025, 3.0, 1), (-2, 3.0, 1), (5, -1.0, 1), (5, float("nan"), 1), (5, 3.0, -1)):
        ev.qe_k, ev.qe_alpha, ev.qe_times = k, alpha, times
        with pytest.raises(ValueError):         # before torch.cat of the (empty) feature list, before any device work
            ev.compute()


def test_config_keys():
    from config import cfg, cfg_base
    for c in (cfg, cfg_base):
        assert c.TEST.QE_K == 0 and c.TEST.QE_ALPHA == 3.0 and c.TEST.QE_TIMES == 1
        assert isinstance(c.TEST.QE_K, int) and isinstance(c.TEST.QE_ALPHA, float) and isinstance(c.TEST.QE_TIMES, int)
    c = cfg_base.clone()
    c.defrost()
    c.merge_from_list(["TEST.QE_K", "10", "TEST.QE_ALPHA", "2.5", "TEST.QE_TIMES", "2"])
    c.freeze()
    assert c.TEST.QE_K == 10 and c.TEST.QE_ALPHA == 2.5 and c.TEST.QE_TIMES == 2
    assert cfg_base.TEST.QE_K == 0
    c = cfg_base.clone()
    c.defrost()
    c.merge_from_list(["TEST.QE_K", 5])
    assert c.TEST.QE_K == 5 and c.TEST.QE_ALPHA == 3.0


def test_processor_reads_the_keys(caplog):
    import logging
    from config import cfg_base
    from processor.processor import configure_query_expansion

    class Ev:
        pass
    ev = Ev()
    with caplog.at_level(logging.INFO, logger="transreid.test"):
        configure_query_expansion(cfg_base, ev)
        assert (ev.qe_k, ev.qe_alpha, ev.qe_times) == (0, 3.0, 1) and not caplog.records
        c = cfg_base.clone()
        c.defrost()
        c.merge_from_list(["TEST.QE_K", 7, "TEST.QE_ALPHA", 2.0, "TEST.QE_TIMES", 3])
        configure_query_expansion(c, ev)
    assert (ev.qe_k, ev.qe_alpha, ev.qe_times) == (7, 2.0, 3)
    assert len(caplog.records) == 1 and "TEST.QE_K" in caplog.records[0].getMessage()
