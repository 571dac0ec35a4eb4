"""Query expansion in feature space on the GPU: mpreid_qe_aggregate_f32 (csrc/qexpand.hip) through the C ABI,
ops.qe_aggregate / ops.expand_features, the evaluators' qe_k / qe_alpha / qe_times and test.py's TEST.QE_K.

The yardstick is the host definition (utils.metrics.qe_aggregate / expand_features: numpy, pinned by
tests/test_query_expansion_cpu.py).  For alpha = 0 and the integers 1 ... 8 every comparison is bit for bit (uint32 views); a
non-integer alpha goes through powf and is held to a rounding bound against float64."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

FILL = -7.0
U = 2.0 ** -24
POWF_ULP = 16     # no accuracy table of the HIP math functions ships with the toolchain: the OpenCL full-profile bound for pow


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lists(rng, rows, k, n_src):
    """lists as mpreid_rank_topk writes them, with the rows that matter: an empty list, a short one, duplicate indices,
    distances past 2 (s clamps to 0), a slightly negative self-distance, a count above k (clamped)"""
    idx = rng.integers(0, n_src, (rows, k)).astype(np.int32)
    dist = (rng.random((rows, k)) * 1.8).astype(np.float32)
    dist.sort(axis=1)
    cnt = np.full(rows, k, np.int32)
    cnt[0] = 0
    cnt[1] = k // 2
    idx[2, :] = idx[2, 0]
    dist[3, k // 2:] = np.float32(2.5) + np.arange(k - k // 2, dtype=np.float32) * np.float32(0.125)
    idx[4, 0], dist[4, 0] = 4 % n_src, np.float32(-1e-6)
    cnt[5] = k + 3
    for r in range(rows):                       # past the count: what the ranking kernel leaves there
        c = min(max(int(cnt[r]), 0), k)
        idx[r, c:], dist[r, c:] = -1, np.inf
    return idx, dist, cnt


class _Layout:
    """src / out as column slices of wider buffers one float off a 16-byte boundary (odd leading dimensions), or as aligned
    buffers with leading dimensions that are multiples of four; out is pre-filled, with a guard row behind it"""

    def __init__(self, src, rows, aligned):
        n_src, d = src.shape
        if aligned:
            lds, ldo, off = (d + 3) // 4 * 4 + 4, (d + 3) // 4 * 4 + 8, 0
        else:
            lds, ldo, off = d + 7, d + 5, 1
        self.sbuf = torch.zeros((max(n_src, 1), lds), dtype=torch.float32, device="cuda")
        self.obuf = torch.full((rows + 1, ldo), FILL, dtype=torch.float32, device="cuda")
        self.src = self.sbuf[:n_src, off:off + d]
        self.src.copy_(torch.from_numpy(src))
        self.out = self.obuf[:rows, off:off + d]
        assert self.src.data_ptr() % 16 == 4 * off and self.out.data_ptr() % 16 == 4 * off
        self.lds, self.ldo, self.off, self.rows, self.d = lds, ldo, off, rows, d

    def result(self):
        """the output rows; asserts that nothing outside them was written"""
        torch.cuda.synchronize()
        o = self.obuf.cpu().numpy()
        mask = np.ones(o.shape, bool)
        mask[:self.rows, self.off:self.off + self.d] = False
        assert np.all(o[mask] == FILL), "a store outside the output rows"
        return o[:self.rows, self.off:self.off + self.d]


def _call(src_t, n_src, d, lds, idx_t, dist_t, cnt_t, rows, k, alpha, out_t, ldo):
    from mpreid import _lib
    rc = _lib.load().mpreid_qe_aggregate_f32(_ptr(src_t), n_src, d, lds, _ptr(idx_t), _ptr(dist_t), _ptr(cnt_t), rows, k,
                                             alpha, _ptr(out_t), ldo, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("k", [1, 2, 10, 64, 1024])
@pytest.mark.parametrize("d", [1, 3, 64, 70, 1280, 2050])
def test_abi_bit_for_bit(d, k):
    from utils.metrics import qe_aggregate
    rng = np.random.default_rng(1000 * d + k)
    n_src, rows = (1100 if k == 1024 else 257), 12
    src = (rng.standard_normal((n_src, d)) * (0.25 + 4 * rng.random((n_src, 1)))).astype(np.float32)
    idx, dist, cnt = _lists(rng, rows, k, n_src)
    t_idx, t_dist, t_cnt = _dev(idx, dist, cnt)
    for alpha in (0, 1, 3, 8):
        want = qe_aggregate(src, idx, dist, cnt, alpha)
        assert np.all(want[0] == 0) and (k < 2 or np.any(want[1] != 0))
        for aligned in (False, True):
            lay = _Layout(src, rows, aligned)
            rc = _call(lay.src, n_src, d, lay.lds, t_idx, t_dist, t_cnt, rows, k, float(alpha), lay.out, lay.ldo)
            assert rc == 0
            got = lay.result()
            assert np.array_equal(_bits(got), _bits(want)), (alpha, aligned, np.argwhere(_bits(got) != _bits(want))[:4])


def test_abi_more_rows_than_workgroups():
    """rows past the grid's cap of 2^20 workgroups are taken in a second turn of the kernel's row loop"""
    from mpreid import ops
    from utils.metrics import qe_aggregate
    rng = np.random.default_rng(5)
    rows, n_src, d, k = (1 << 20) + 5, 1000, 3, 2
    src = rng.standard_normal((n_src, d)).astype(np.float32)
    idx = rng.integers(0, n_src, (rows, k)).astype(np.int32)
    dist = rng.random((rows, k)).astype(np.float32)
    cnt = rng.integers(0, k + 1, rows).astype(np.int32)
    got = ops.qe_aggregate(*_dev(src, idx, dist, cnt), 3.0).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(qe_aggregate(src, idx, dist, cnt, 3)))


def test_abi_refusals_launch_nothing():
    from mpreid import _lib
    from utils.metrics import qe_aggregate
    L = _lib.load()
    rng = np.random.default_rng(9)
    n_src, d, rows, k = 40, 6, 8, 4
    src = rng.standard_normal((n_src, d)).astype(np.float32)
    idx, dist, cnt = _lists(rng, rows, k, n_src)
    t_idx, t_dist, t_cnt = _dev(idx, dist, cnt)
    big = torch.zeros((rows, 1025), dtype=torch.int32, device="cuda")
    lay = _Layout(src, rows, False)
    a = dict(src_t=lay.src, n_src=n_src, d=d, lds=lay.lds, idx_t=t_idx, dist_t=t_dist, cnt_t=t_cnt, rows=rows, k=k, alpha=3.0,
             out_t=lay.out, ldo=lay.ldo)
    bad = [dict(k=0), dict(k=-1), dict(d=0), dict(rows=-1), dict(n_src=-1), dict(lds=d - 1), dict(ldo=d - 1), dict(alpha=-0.5),
           dict(alpha=float("nan")), dict(src_t=None), dict(idx_t=None), dict(dist_t=None), dict(cnt_t=None), dict(out_t=None),
           dict(out_t=lay.src, ldo=lay.lds),                                  # in place
           dict(out_t=lay.sbuf[n_src - 1:, 2:], ldo=lay.lds, rows=1)]         # meets the last row of src
    for change in bad:
        assert _call(**dict(a, **change)) == _lib.ERR_ARG, change
        assert L.mpreid_last_error()
    assert _call(**dict(a, k=1025, idx_t=big, dist_t=big.float())) == _lib.ERR_UNSUPPORTED
    assert b"1024" in L.mpreid_last_error()
    assert _call(**dict(a, rows=0)) == 0                                       # a no-op
    assert np.all(lay.obuf.cpu().numpy() == FILL)                              # nothing of all that was launched
    assert np.array_equal(lay.sbuf[:n_src, 1:1 + d].cpu().numpy(), src)
    assert _call(**a) == 0                                                     # the next valid call works
    assert np.array_equal(_bits(lay.result()), _bits(qe_aggregate(src, idx, dist, cnt, 3)))


@pytest.mark.parametrize("d,k", [(70, 64), (1280, 10)])
def test_non_integer_alpha_against_float64(d, k):
    """alpha = 2.5 goes through powf.  Per row: ||delta||_2 <= (kk + 2 + P) 2^-24 sum_j w_j ||f_j||_2 with P = powf's error
    in ulps -- kk - 1 additions, one product per term, the divide, the rounding of s, the power."""
    from mpreid import ops
    rng = np.random.default_rng(d)
    n_src, rows, alpha = 500, 64, 2.5
    src = (rng.standard_normal((n_src, d)) * (0.25 + 4 * rng.random((n_src, 1)))).astype(np.float32)
    idx, dist, cnt = _lists(rng, rows, k, n_src)
    for aligned in (False, True):
        lay = _Layout(src, rows, aligned)
        got = ops.qe_aggregate(lay.src, *_dev(idx, dist, cnt), alpha, out=lay.out)
        assert got is lay.out
        got = lay.result().astype(np.float64)
        worst = 0.0
        for r in range(rows):
            kk = min(max(int(cnt[r]), 0), k)
            if kk == 0:
                assert np.all(got[r] == 0)
                continue
            w = np.maximum(1.0 - 0.5 * dist[r, :kk].astype(np.float64), 0.0) ** alpha
            rows64 = src[idx[r, :kk]].astype(np.float64)
            want = (w[:, None] * rows64).sum(0) / kk
            bound = (kk + 2 + POWF_ULP) * U * float((w * np.linalg.norm(rows64, axis=1)).sum())
            err = float(np.linalg.norm(got[r] - want))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, (r, err, bound)
        print(f"alpha 2.5, d = {d}, k = {k}, aligned = {aligned}: largest ||delta|| / bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------- ops.expand_features
def _host_rounds(f, k, alpha, times):
    """the definition, round by round: Dm from the exact distance kernel (pinned to the oracle by tests/test_gpu_distance.py)
    on the device-normalised rows, copied to the host; lists and sums in numpy"""
    from mpreid import ops
    from utils.metrics import expand_features
    f = np.ascontiguousarray(f, dtype=np.float32)
    for _ in range(times):
        unit = ops.l2_normalize(torch.from_numpy(f).cuda())
        f = expand_features(f, ops.euclidean_distance(unit, unit, mode=ops.GEMM_F32_EXACT).cpu().numpy(), k, alpha)
    return f


def _check_expand(f, nq, k, alpha, times, chunk=None):
    from mpreid import ops
    qf, gf = torch.from_numpy(f[:nq]).cuda(), torch.from_numpy(f[nq:]).cuda()
    q2, g2 = ops.expand_features(qf, gf, k, alpha, times, chunk=chunk)
    assert q2.is_cuda and g2.is_cuda and tuple(q2.shape) == (nq, f.shape[1]) and tuple(g2.shape) == (f.shape[0] - nq, f.shape[1])
    assert np.array_equal(qf.cpu().numpy(), f[:nq]) and np.array_equal(gf.cpu().numpy(), f[nq:])      # inputs are only read
    got = np.concatenate([q2.cpu().numpy(), g2.cpu().numpy()])
    want = _host_rounds(f, k, alpha, times)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
    return got


@pytest.fixture(scope="module")
def clustered():
    from mpreid import synth
    return synth.clustered_features(300, 1280, 0.5, seed=11, normalize=False)[0].astype(np.float32)


@pytest.mark.parametrize("times", [1, 2])
@pytest.mark.parametrize("alpha", [1, 3])
def test_expand_features_clustered(clustered, alpha, times):
    got = _check_expand(clustered, 100, 10, alpha, times)
    assert not np.array_equal(got, clustered)
    if times == 2:
        assert not np.array_equal(got, _host_rounds(clustered, 10, alpha, 1))


@pytest.mark.parametrize("alpha", [1, 3])
def test_expand_features_ties_and_chunks(alpha):
    """small-integer rows, each present several times: whole groups of distances are equal and the index order decides which
    of them a list takes; chunks smaller than k and chunks that do not divide N"""
    from mpreid import ops
    from utils.metrics import rank_lists
    rng = np.random.default_rng(3)
    pool = rng.integers(-2, 3, (40, 16)).astype(np.float32)
    pool[np.all(pool == 0, axis=1), 0] = 1
    f = pool[rng.integers(0, 40, 203)]
    unit = ops.l2_normalize(torch.from_numpy(f).cuda())
    dm = ops.euclidean_distance(unit, unit).cpu().numpy()
    val = rank_lists(dm, 10)[1]
    assert np.mean(val[:, 1:] == val[:, :-1]) > 0.3                                     # precondition: ties inside the lists
    for times in (1, 2):
        for chunk in (3, 77, None):
            _check_expand(f, 60, 10, alpha, times, chunk)


def test_expand_features_edges():
    from mpreid import ops
    rng = np.random.default_rng(8)
    f = rng.standard_normal((9, 5)).astype(np.float32)
    _check_expand(f[:1], 1, 5, 3, 1)                       # N = 1 as one query ...
    got = _check_expand(f[:1], 0, 5, 3, 2)                 # ... and as one gallery row: the row comes back, times its weight twice
    assert np.allclose(got, f[:1], rtol=4e-6, atol=0)      # (|self-distance| <= 1e-6: s within 5e-7 of 1, s^3 within 1.5e-6, twice)
    _check_expand(f, 0, 4, 1, 2)                           # nq = 0
    _check_expand(f, 9, 4, 3, 1)                           # ng = 0
    _check_expand(f, 4, 1024, 0, 1)                        # k > N clamps; alpha = 0: the plain mean
    q, g = torch.from_numpy(f[:4]).cuda(), torch.from_numpy(f[4:]).cuda()
    q0, g0 = ops.expand_features(q, g, 3, times=0)         # no round: copies
    assert q0.data_ptr() != q.data_ptr() and np.array_equal(q0.cpu().numpy(), f[:4]) and np.array_equal(g0.cpu().numpy(), f[4:])
    e = torch.zeros((0, 5), device="cuda")
    q0, g0 = ops.expand_features(e, e, 3)
    assert tuple(q0.shape) == (0, 5) and tuple(g0.shape) == (0, 5)


# ----------------------------------------------------------------------------------------------------------- evaluators
@pytest.fixture(scope="module")
def evalset(golden):
    return golden("r1_map_eval.npz")


def _run_evaluator(z, rerank, same_cam, list_k, qe, drop_attributes=False):
    from utils.metrics import R1_mAP_eval
    ev = R1_mAP_eval(96, feat_norm=True, reranking=rerank)
    ev.remove_same_cam = same_cam
    ev.rank_list_k = list_k
    if drop_attributes:          # an evaluator from before the feature: the attributes were never set
        del ev.qe_k, ev.qe_alpha, ev.qe_times
    elif qe is not None:
        ev.qe_k, ev.qe_alpha, ev.qe_times = qe
    ev.reset()
    for s in range(0, 480, 128):
        ev.update((torch.from_numpy(z["raw"][s:s + 128]).cuda(), tuple(int(p) for p in z["pid"][s:s + 128]),
                   tuple(int(c) for c in z["cam"][s:s + 128])))
    return ev, ev.compute()


def _same_tuple(a, b):
    assert len(a) == len(b) == 7
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and float(a[1]) == float(b[1])
    assert a[2].dtype == b[2].dtype and a[2].tobytes() == b[2].tobytes()
    assert list(a[3]) == list(b[3]) and list(a[4]) == list(b[4])
    assert a[5].numpy().tobytes() == b[5].numpy().tobytes() and a[6].numpy().tobytes() == b[6].numpy().tobytes()


@pytest.mark.parametrize("rerank", [False, True])
@pytest.mark.parametrize("same_cam", [False, True])
def test_evaluator_equals_the_manual_composition(evalset, rerank, same_cam):
    from mpreid import ops
    from utils.metrics import eval_func_device, rank_lists
    from utils.reranking import re_ranking_device
    z = evalset
    pid, cam = z["pid"], z["cam"]
    ev, out = _run_evaluator(z, rerank, same_cam, 20, (5, 3.0, 1))
    raw = torch.from_numpy(z["raw"]).cuda()
    q2, g2 = ops.expand_features(raw[:96], raw[96:], 5, 3.0, 1)
    qn, gn = ops.l2_normalize(q2), ops.l2_normalize(g2)
    if rerank:
        dist = re_ranking_device(qn, gn, k1=50, k2=15, lambda_value=0.3, algo=0)[0]
    else:
        dist = ops.euclidean_distance(qn, gn)
    cmc, mAP = eval_func_device(dist, pid[:96], pid[96:], cam[:96], cam[96:], remove_same_cam=same_cam)
    want = (cmc, mAP, dist.cpu().numpy(), [int(p) for p in pid], [int(c) for c in cam], qn.cpu(), gn.cpu())
    _same_tuple(out, want)
    lists = rank_lists(out[2], 20, pid[:96], pid[96:], cam[:96], cam[96:], remove_same_cam=same_cam)
    for a, b in zip(ev.last_rank_lists, lists):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    plain = _run_evaluator(z, rerank, same_cam, 0, None)[1]
    assert out[2].tobytes() != plain[2].tobytes() and out[5].numpy().tobytes() != plain[5].numpy().tobytes()


@pytest.mark.parametrize("rerank", [False, True])
def test_evaluator_with_qe_off_is_the_evaluator_without_the_feature(evalset, monkeypatch, rerank):
    from mpreid import _lib

    def refuse(*a):
        raise AssertionError("mpreid_qe_aggregate_f32 was called with qe_k = 0")
    monkeypatch.setattr(_lib.load(), "mpreid_qe_aggregate_f32", refuse)
    ev_off, off = _run_evaluator(evalset, rerank, True, 10, (0, 3.0, 1))
    ev_old, old = _run_evaluator(evalset, rerank, True, 10, None, drop_attributes=True)
    assert not hasattr(ev_old, "qe_k")
    _same_tuple(off, old)
    for a, b in zip(ev_off.last_rank_lists, ev_old.last_rank_lists):
        assert a.tobytes() == b.tobytes()


def test_evaluator_two_rounds_and_distance_mode(evalset):
    """qe_times and the evaluator's distance_mode reach the neighbour search"""
    from mpreid import ops
    z = evalset
    raw = torch.from_numpy(z["raw"]).cuda()
    for mode in (ops.GEMM_F32_EXACT, ops.GEMM_F16_SPLIT3):
        from utils.metrics import R1_mAP_eval
        ev = R1_mAP_eval(96)
        ev.qe_k, ev.qe_alpha, ev.qe_times, ev.distance_mode = 4, 1.0, 2, mode
        ev.reset()
        ev.update((raw, tuple(int(p) for p in z["pid"]), tuple(int(c) for c in z["cam"])))
        out = ev.compute()
        q2, g2 = ops.expand_features(raw[:96], raw[96:], 4, 1.0, 2, mode=mode)
        qn, gn = ops.l2_normalize(q2), ops.l2_normalize(g2)
        assert out[5].numpy().tobytes() == qn.cpu().numpy().tobytes() and out[6].numpy().tobytes() == gn.cpu().numpy().tobytes()
        assert out[2].tobytes() == ops.euclidean_distance(qn, gn, mode=mode).cpu().numpy().tobytes()


def _update_all(ev, f, pid, cam, idx, step=128):
    for s in range(0, len(idx), step):
        sel = idx[s:s + step]
        ev.update((torch.from_numpy(f[sel]).cuda(), tuple(int(p) for p in pid[sel]), tuple(int(c) for c in cam[sel])))


@pytest.mark.parametrize("rerank", [False, True])
def test_splits_evaluator_equals_single_split_evaluators(rerank):
    import utils.metrics as M
    from datasets.make_dataloader import vehicleid_trial_splits
    from mpreid import synth
    n = 600
    f, pid = synth.clustered_features(n, 64, 2.5, seed=31, normalize=False)
    cam = synth.labels_for(n)
    splits = vehicleid_trial_splits(pid, trials=3, seed=0)
    ev = M.R1_mAP_eval_splits(splits, feat_norm=True, reranking=rerank)
    ev.qe_k, ev.qe_alpha, ev.qe_times = 5, 3.0, 1
    ev.reset()
    _update_all(ev, f, pid, cam, np.arange(n))
    cmcs, maps, _, _, feats_host = ev.compute()
    assert ev.last_dist is None and tuple(feats_host.shape) == f.shape          # QE depends on the split: no pooled matrix
    plain = M.R1_mAP_eval_splits(splits, feat_norm=True, reranking=rerank)
    plain.reset()
    _update_all(plain, f, pid, cam, np.arange(n))
    maps_plain = plain.compute()[1]
    assert [float(m) for m in maps_plain] != [float(m) for m in maps]            # precondition: QE changes the numbers
    for i, (q, g) in enumerate(splits):
        one = M.R1_mAP_eval(len(q), feat_norm=True, reranking=rerank)
        one.qe_k, one.qe_alpha, one.qe_times = 5, 3.0, 1
        one.reset()
        _update_all(one, f, pid, cam, np.concatenate([q, g]))
        cmc, mAP = one.compute()[:2]
        assert cmcs[i].dtype == cmc.dtype and np.array_equal(cmcs[i], cmc) and float(maps[i]) == float(mAP), i


def test_evaluator_refuses_qe_under_a_process_group(evalset):
    from emulated_group import EmulatedWorld
    from utils.metrics import R1_mAP_eval
    z = evalset
    world = EmulatedWorld(2)

    def rank_fn(rank):
        ev = R1_mAP_eval(96)
        ev.qe_k = 5
        ev.reset()
        ev.update((torch.from_numpy(z["raw"][:64]).cuda(), tuple(int(p) for p in z["pid"][:64]),
                   tuple(int(c) for c in z["cam"][:64])))
        with pytest.raises(NotImplementedError, match="query expansion is single-process"):
            ev.compute()
        return True
    assert world.run(rank_fn) == [True, True]
    assert world.log == []                                                        # raised before any collective


# ------------------------------------------------------------------------------------------------------------------ CLI
OVERRIDES = ["DATASETS.SYNTH_QUERY", 24, "DATASETS.SYNTH_GALLERY", 72, "DATASETS.SYNTH_IDS", 6, "TEST.IMS_PER_BATCH", 32]


def _cli():
    spec = importlib.util.spec_from_file_location("mpreid_test_cli_query_expansion", os.path.join(ROOT, "mp-reid_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_keys(tmp_path):
    from mpreid import ops
    from processor.processor import do_inference
    base = ["--config_file", ""] + [str(x) for x in OVERRIDES] + ["TEST.RANK_LIST_K", "10"]
    _cli().main(base + ["TEST.QE_K", "5", "TEST.QE_ALPHA", "3.0", "OUTPUT_DIR", str(tmp_path / "qe")])
    ev = do_inference.last_evaluator
    assert (ev.qe_k, ev.qe_alpha, ev.qe_times) == (5, 3.0, 1)
    raw = torch.cat(ev.feats, dim=0)
    distmat = ev.compute()[2]
    q2, g2 = ops.expand_features(raw[:24], raw[24:], 5, 3.0, 1)
    composed = ops.euclidean_distance(ops.l2_normalize(q2), ops.l2_normalize(g2)).cpu().numpy()
    assert distmat.tobytes() == composed.tobytes()
    z_qe = np.load(str(tmp_path / "qe" / "rank_lists.npz"))
    # without the keys: the evaluation of the unexpanded features, in the evaluator and in the file it writes
    _cli().main(base + ["OUTPUT_DIR", str(tmp_path / "plain")])
    ev0 = do_inference.last_evaluator
    assert ev0.qe_k == 0
    raw0 = torch.cat(ev0.feats, dim=0)
    assert raw0.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes()
    distmat0 = ev0.compute()[2]
    unit = ops.l2_normalize(raw0)
    assert distmat0.tobytes() == ops.euclidean_distance(unit[:24], unit[24:]).cpu().numpy().tobytes()
    assert distmat0.tobytes() != distmat.tobytes()
    z0 = np.load(str(tmp_path / "plain" / "rank_lists.npz"))
    _cli().main(base + ["TEST.QE_K", "0", "OUTPUT_DIR", str(tmp_path / "zero")])
    z1 = np.load(str(tmp_path / "zero" / "rank_lists.npz"))
    assert sorted(z0.files) == sorted(z1.files) == sorted(z_qe.files)
    for name in z0.files:
        assert z0[name].dtype == z1[name].dtype and z0[name].tobytes() == z1[name].tobytes(), name
    assert z0["distances"].tobytes() != z_qe["distances"].tobytes()
