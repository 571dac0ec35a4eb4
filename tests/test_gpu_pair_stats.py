"""mpreid_pair_bucket_counts (csrc/pairstats.hip) through the C ABI and through mpreid.ops, and ops.pair_select, against the
host definitions of utils/metrics.py (themselves held to plain loops by tests/test_pair_stats_cpu.py).  Everything is
counting, so everything is compared with array_equal, thresholds as bytes.  Shapes are the smallest that reach every path of
the kernel: below one vector / one wave, the 16-byte and the 4-byte load path, several tiles in both grid directions, one
copy of the LDS counters (4096 bounds) and privatised copies (few bounds), every pair in one bucket."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A


def _host_buckets(d, qp, gp, qc, gc, bound_keys):
    """counts [2][B + 1] from the definition: bucket = number of bounds below the key (numpy; the keys' order itself is
    checked against Python loops in the CPU tests)"""
    from mpreid import ops
    keys = ops.dist_keys(d)
    kept = np.isfinite(d)
    same = qp[:, None] == gp[None, :]
    if qc is not None:
        kept &= ~(same & (qc[:, None] == gc[None, :]))
    nb = len(bound_keys) + 1
    b = np.searchsorted(np.asarray(bound_keys, np.uint32), keys, side="left")
    return np.stack([np.bincount(b[kept & same], minlength=nb), np.bincount(b[kept & ~same], minlength=nb)]).astype(np.int64)


def _abi(dt, qp, gp, qc, gc, bound_keys, accumulate=0, counts=None, n_bounds=None, ld=None, nq=None, ng=None):
    """one call through the C ABI on a device tensor view dt; returns (rc, counts tensor with a guard word on either side)"""
    from mpreid import _lib
    L = _lib.load()
    dev = _lib.require_gpu()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)   # noqa: E731
    t = [up(a) for a in (qp, gp, qc, gc)]
    bk = torch.from_numpy(np.ascontiguousarray(bound_keys, dtype=np.uint32).view(np.int32)).to(dev)
    nb = len(bound_keys) if n_bounds is None else n_bounds
    if counts is None:
        counts = torch.full((2 * (len(bound_keys) + 1) + 2,), GUARD, dtype=torch.int64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
    rc = L.mpreid_pair_bucket_counts(p(dt), dt.stride(0) if ld is None else ld, dt.shape[0] if nq is None else nq,
                                     dt.shape[1] if ng is None else ng, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(bk), nb,
                                     accumulate, C.c_void_p(counts.data_ptr() + 8), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, counts


def _unguard(counts, nb):
    c = counts.cpu().numpy()
    assert c[0] == GUARD and c[-1] == GUARD, "a guard word around counts was overwritten"
    return c[1:-1].reshape(2, nb)


def _labels(rng, nq, ng, ids, cams=3):
    return rng.integers(0, ids, nq), rng.integers(0, ids, ng), rng.integers(0, cams, nq), rng.integers(0, cams, ng)


def _eighths(nq, ng, seed):
    rng = np.random.default_rng(seed)
    return (np.round(rng.random((nq, ng)) * 8) / 8).astype(np.float32), rng


@pytest.mark.parametrize("cam", [False, True])
def test_eighths_inclusive_bounds_and_ties(cam):
    from mpreid import ops
    from utils import metrics
    d, rng = _eighths(40, 600, 1)
    qp, gp, qc, gc = _labels(rng, 40, 600, 10)
    qp[0] = 10_000                                                  # a query without a positive
    thr = (np.arange(9) / 8).astype(np.float32)                     # ON the eighths: d <= t must be inclusive
    bk = ops.dist_keys(thr)
    dt = torch.from_numpy(d).cuda()
    cams = (qc, gc) if cam else (None, None)
    want = _host_buckets(d, qp, gp, *cams, bk)
    rc, counts = _abi(dt, qp, gp, *cams, bk)
    assert rc == 0 and np.array_equal(_unguard(counts, 10), want)
    got = ops.pair_bucket_counts(dt, qp, gp, *cams, bound_keys=bk)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    host = metrics.pair_counts(d, thr, qp, gp, qc, gc, remove_same_cam=cam)
    dev = metrics.pair_counts_device(dt, thr, qp, gp, qc, gc, remove_same_cam=cam)
    for k in ("tp", "fp"):
        assert np.array_equal(dev[k], host[k]) and dev[k].dtype == np.int64
    assert (dev["P"], dev["Nn"]) == (host["P"], host["Nn"])
    assert want[:, -1].sum() == 0 and host["tp"][-1] == host["P"]      # nothing above 1.0


@pytest.mark.parametrize("shape", [(3, 1), (5, 37)])
def test_below_one_vector_and_one_wave(shape):
    from mpreid import ops
    d, rng = _eighths(*shape, seed=2)
    qp, gp, qc, gc = _labels(rng, *shape, 3, 2)
    bk = ops.dist_keys(np.array([0.25, 0.5], np.float32))
    dt = torch.from_numpy(d).cuda()
    for cams in ((None, None), (qc, gc)):
        rc, counts = _abi(dt, qp, gp, *cams, bk)
        assert rc == 0 and np.array_equal(_unguard(counts, 3), _host_buckets(d, qp, gp, *cams, bk))


def test_unaligned_column_slice_equals_the_aligned_matrix():
    from mpreid import ops
    d, rng = _eighths(33, 1500, 3)
    qp, gp, qc, gc = _labels(rng, 33, 1500, 7)
    bk = ops.dist_keys((np.arange(1, 8) / 8).astype(np.float32))
    wide = torch.zeros((33, 1503), dtype=torch.float32, device="cuda")
    wide[:, 1:1501] = torch.from_numpy(d).cuda()
    view = wide[:, 1:1501]                                          # starts 4 bytes off, ld = 1503 > ng: the 4-byte path
    assert view.data_ptr() % 16 == 4 and view.stride(0) == 1503
    aligned = torch.from_numpy(d).cuda()                            # ld = 1500, a multiple of 4: the 16-byte path
    assert aligned.data_ptr() % 16 == 0
    want = _host_buckets(d, qp, gp, qc, gc, bk)
    a = ops.pair_bucket_counts(view, qp, gp, qc, gc, bound_keys=bk).cpu().numpy()
    b = ops.pair_bucket_counts(aligned, qp, gp, qc, gc, bound_keys=bk).cpu().numpy()
    assert np.array_equal(a, want) and np.array_equal(b, want)


@pytest.fixture(scope="module")
def big():
    """300 x 5000 random distances in [0, 2): 5 column tiles x several row blocks; 4096 bounds spread over the range"""
    rng = np.random.default_rng(4)
    d = (rng.random((300, 5000)) * 2).astype(np.float32)
    qp, gp, qc, gc = _labels(rng, 300, 5000, 50)
    from mpreid import ops
    bk = np.unique(ops.dist_keys(np.linspace(0.0, 2.0, 4096).astype(np.float32)))
    assert bk.size == 4096
    return d, qp, gp, qc, gc, bk, _host_buckets(d, qp, gp, qc, gc, bk), torch.from_numpy(d).cuda()


def test_several_tiles_both_directions_4096_bounds(big):
    from mpreid import ops
    d, qp, gp, qc, gc, bk, want, dt = big
    rc, counts = _abi(dt, qp, gp, qc, gc, bk)
    assert rc == 0 and np.array_equal(_unguard(counts, 4097), want)
    assert (want > 0).sum() > 4000                                   # precondition: the buckets are really spread
    nocam = ops.pair_bucket_counts(dt, qp, gp, bound_keys=bk).cpu().numpy()
    assert np.array_equal(nocam, _host_buckets(d, qp, gp, None, None, bk))


def test_accumulate_and_column_blocks(big):
    from mpreid import ops
    d, qp, gp, qc, gc, bk, want, dt = big
    rc, counts = _abi(dt, qp, gp, qc, gc, bk)
    rc2, counts = _abi(dt, qp, gp, qc, gc, bk, accumulate=1, counts=counts)
    assert rc == 0 and rc2 == 0 and np.array_equal(_unguard(counts, 4097), 2 * want)
    # two column blocks of a matrix that is never held whole (the second starts at an odd column: its own load path)
    out = ops.pair_bucket_counts(dt[:, :2001], qp, gp[:2001], qc, gc[:2001], bound_keys=bk)
    before = out.data_ptr()
    out2 = ops.pair_bucket_counts(dt[:, 2001:], qp, gp[2001:], qc, gc[2001:], bound_keys=bk, out=out)
    assert out2.data_ptr() == before and np.array_equal(out2.cpu().numpy(), want)
    # accumulate = 0 really zeroes: a dirty buffer gives the plain counts
    dirty = torch.full((2 * 4097 + 2,), GUARD, dtype=torch.int64, device="cuda")
    rc, dirty = _abi(dt, qp, gp, qc, gc, bk, accumulate=0, counts=dirty)
    assert rc == 0 and np.array_equal(_unguard(dirty, 4097), want)


@pytest.mark.parametrize("n_bounds", [1, 4096])
def test_all_equal_matrix_lands_in_one_bucket(n_bounds):
    """64 x 5000 entries of 0.375: every lane of every wave hits one counter (the contention form)"""
    from mpreid import ops
    d = np.full((64, 5000), 0.375, np.float32)
    rng = np.random.default_rng(5)
    qp, gp, qc, gc = _labels(rng, 64, 5000, 9)
    if n_bounds == 1:
        bk = ops.dist_keys(np.array([0.375], np.float32))
    else:
        bk = np.unique(ops.dist_keys(np.linspace(0.0, 1.0, 4096).astype(np.float32)))
    want = _host_buckets(d, qp, gp, qc, gc, bk)
    assert (want > 0).sum() == 2
    got = ops.pair_bucket_counts(torch.from_numpy(d).cuda(), qp, gp, qc, gc, bound_keys=bk).cpu().numpy()
    assert np.array_equal(got, want)


def test_negative_zero_negative_and_non_finite_entries():
    from mpreid import ops
    from utils import metrics
    d, rng = _eighths(9, 130, 6)
    d -= np.float32(0.25)
    d[d == 0] = -0.0
    d[0, :5] = [np.inf, -np.inf, np.nan, -0.0, 0.0]
    d[8, 129] = np.inf
    qp, gp, qc, gc = _labels(rng, 9, 130, 4)
    thr = np.array([-0.25, -0.125, -0.0, 0.125, 3.0e38], np.float32)
    bk = ops.dist_keys(thr)
    dt = torch.from_numpy(d).cuda()
    want = _host_buckets(d, qp, gp, None, None, bk)
    assert want.sum() == 9 * 130 - 4                                 # the four non-finite entries are no pairs
    assert np.array_equal(ops.pair_bucket_counts(dt, qp, gp, bound_keys=bk).cpu().numpy(), want)
    host, dev = metrics.pair_counts(d, thr, qp, gp), metrics.pair_counts_device(dt, thr, qp, gp)
    assert np.array_equal(dev["tp"], host["tp"]) and np.array_equal(dev["fp"], host["fp"])
    zero = thr.tolist().index(0.0)
    assert host["tp"][zero] + host["fp"][zero] == int((d[np.isfinite(d)] <= 0).sum())     # -0 counts as 0


def test_filter_with_a_query_whose_every_pid_hit_is_junk():
    from mpreid import ops
    d, rng = _eighths(4, 300, 7)
    qp, gp, qc, gc = _labels(rng, 4, 300, 5)
    qp[1], qc[1] = 3, 2
    gc[gp == 3] = 2                                                  # query 1: all its pid hits share its camera
    bk = ops.dist_keys(np.array([0.5], np.float32))
    want = _host_buckets(d, qp, gp, qc, gc, bk)
    got = ops.pair_bucket_counts(torch.from_numpy(d).cuda(), qp, gp, qc, gc, bound_keys=bk).cpu().numpy()
    assert np.array_equal(got, want)
    only1 = ops.pair_bucket_counts(torch.from_numpy(d[1:2]).cuda(), qp[1:2], gp, qc[1:2], gc, bound_keys=bk).cpu().numpy()
    assert only1[0].sum() == 0 and only1[1].sum() == int((gp != 3).sum())


def test_empty_matrix_and_argument_errors():
    from mpreid import _lib, ops
    d, rng = _eighths(4, 64, 8)
    qp, gp, qc, gc = _labels(rng, 4, 64, 3)
    bk = ops.dist_keys(np.array([0.25, 0.5], np.float32))
    dt = torch.from_numpy(d).cuda()
    # nq == 0 / ng == 0: zero counts, no launch
    rc, counts = _abi(dt[:0], qp[:0], gp, None, None, bk)
    assert rc == 0 and not _unguard(counts, 3).any()
    rc, counts = _abi(dt[:, :0], qp, gp[:0], None, None, bk, ld=64)
    assert rc == 0 and not _unguard(counts, 3).any()
    assert not ops.pair_bucket_counts(dt[:0], qp[:0], gp, bound_keys=bk).cpu().numpy().any()
    # every MPREID_ERR_ARG case is a return code and nothing else: the guarded buffer is untouched
    for kw, cams in ((dict(n_bounds=0), (None, None)), (dict(n_bounds=4097), (None, None)), (dict(), (qc, None)),
                     (dict(), (None, gc)), (dict(ld=63), (None, None))):
        rc, counts = _abi(dt, qp, gp, *cams, bk, **kw)
        assert rc == _lib.ERR_ARG, kw
        assert (counts.cpu().numpy() == GUARD).all()
    with pytest.raises(ValueError):
        ops.pair_bucket_counts(dt, qp, gp, bound_keys=[5, 5])
    with pytest.raises(ValueError):
        ops.pair_bucket_counts(dt, qp, gp, qc, None, bound_keys=bk)
    with pytest.raises(ValueError):
        ops.pair_bucket_counts(dt, qp, gp, bound_keys=bk, out=torch.zeros((2, 4), dtype=torch.int64, device="cuda"))


def _check_select(d, dt, qp, gp, qc, gc, cam, budgets=None):
    from mpreid import ops
    from utils import metrics
    cams = (qc, gc) if cam else (None, None)
    ref0 = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam, max_fp=[0])
    Nn = ref0["Nn"]
    if budgets is None:
        budgets = sorted({0, 1, max(Nn - 1, 0), Nn, Nn + 5, Nn // 3, Nn // 1000})
    ref = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam, max_fp=budgets)
    got = ops.pair_select(dt, qp, gp, *cams, budgets=budgets)
    assert (got["P"], got["Nn"]) == (ref["P"], ref["Nn"])
    assert np.array_equal(got["tp"], ref["tp"]) and np.array_equal(got["fp"], ref["fp"])
    assert got["tau"].dtype == np.float32 and got["tau"].tobytes() == ref["tau"].tobytes()
    twin = metrics.tpr_at_fpr_device(dt, qp, gp, qc, gc, remove_same_cam=cam, max_fp=budgets)
    for k in ("budgets", "tp", "fp", "tpr", "fpr"):
        assert np.array_equal(twin[k], ref[k], equal_nan=True), k
    assert twin["tau"].tobytes() == ref["tau"].tobytes()
    return ref


@pytest.mark.parametrize("cam", [False, True])
def test_pair_select_on_clustered_unit_features(cam):
    """200 x 1500 distances of clustered unit features: a narrow range, so the selection needs its later rounds"""
    from mpreid import ops
    from utils import metrics
    rng = np.random.default_rng(9)
    centres = rng.standard_normal((30, 64))
    pid = rng.integers(0, 30, 1700)
    f = centres[pid] + 0.35 * rng.standard_normal((1700, 64))
    f = (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)
    cams = rng.integers(0, 4, 1700)
    dt = ops.euclidean_distance(torch.from_numpy(f[:200]).cuda(), torch.from_numpy(f[200:]).cuda())
    d = dt.cpu().numpy()
    qp, gp, qc, gc = pid[:200], pid[200:], cams[:200], cams[200:]
    ref = _check_select(d, dt, qp, gp, qc, gc, cam)
    assert float(d.max()) < 4.0 and ref["Nn"] > 250_000              # precondition: ~3e5 negatives within [0, 4)
    rates = metrics.tpr_at_fpr_device(dt, qp, gp, qc, gc, remove_same_cam=cam)
    host = metrics.tpr_at_fpr(d, qp, gp, qc, gc, remove_same_cam=cam)
    assert rates["fprs"].tolist() == [1e-4, 1e-3, 1e-2]
    for k in ("budgets", "tp", "fp", "tpr", "fpr"):
        assert np.array_equal(rates[k], host[k]), k
    assert rates["tau"].tobytes() == host["tau"].tobytes()


def test_pair_select_with_ties_at_tau_and_on_the_all_equal_matrix():
    d, rng = _eighths(40, 600, 1)
    qp, gp, qc, gc = _labels(rng, 40, 600, 10)
    ref = _check_select(d, torch.from_numpy(d).cuda(), qp, gp, qc, gc, True)
    assert (ref["fp"][ref["budgets"] < ref["Nn"]] < ref["budgets"][ref["budgets"] < ref["Nn"]]).any()   # ties held fp below m
    e = np.full((64, 5000), 0.375, np.float32)
    qp, gp, qc, gc = _labels(np.random.default_rng(5), 64, 5000, 9)
    ref = _check_select(e, torch.from_numpy(e).cuda(), qp, gp, qc, gc, False)
    below = ref["budgets"] < ref["Nn"]
    assert (ref["tau"][below] == np.float32(0.375)).all() and not ref["fp"][below].any() and not ref["tp"][below].any()
