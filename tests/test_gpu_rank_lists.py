"""Ranked gallery lists on the GPU: mpreid_rank_topk (csrc/ranklist.hip) through the C ABI, ops.rank_topk / search_topk,
utils.metrics.rank_lists_device, R1_mAP_eval.rank_list_k and test.py's TEST.RANK_LIST_K.

The yardstick is always the host: utils.metrics.rank_lists (numpy, stable argsort -- pinned to the reference's line 39 by
tests/test_rank_lists_cpu.py) or np.argsort(kind="stable") itself.  Nothing here has a tolerance: indices and counts are
compared with array_equal, distances as bytes (uint32 views) against the matrix entries."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

FILL = -7


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _abi(dt, k, col0=0, labels=None, carry=None, nq=None, ng=None):
    """one call of mpreid_rank_topk on the device matrix (view) dt -> (rc, idx, val, cnt) as numpy; the output buffers are
    pre-filled with -7 and carry one guard row that must come back untouched"""
    from mpreid import _lib
    L = _lib.load()
    nq = dt.shape[0] if nq is None else nq
    ng = dt.shape[1] if ng is None else ng
    rows, kb = max(nq, 0) + 1, max(k, 1)
    if carry is None:
        idx = torch.full((rows, kb), FILL, dtype=torch.int32, device="cuda")
        val = torch.full((rows, kb), float(FILL), dtype=torch.float32, device="cuda")
        cnt = torch.full((rows,), FILL, dtype=torch.int32, device="cuda")
    else:
        idx, val, cnt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in carry)
    lab = [None] * 4 if labels is None else [None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()
                                             for a in labels]
    rc = L.mpreid_rank_topk(_ptr(dt), dt.stride(0) if dt.dim() == 2 and dt.shape[0] else max(ng, 1), nq, ng, col0, k,
                            _ptr(lab[0]), _ptr(lab[1]), _ptr(lab[2]), _ptr(lab[3]), int(carry is not None), _ptr(idx),
                            _ptr(val), _ptr(cnt), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


def _guard_untouched(idx, val, cnt):
    return np.all(idx[-1] == FILL) and np.all(val[-1] == FILL) and cnt[-1] == FILL


def _same(got, want, col0=0):
    """(idx, val, cnt) of the device against the host's (int64 / float32 / int64): entries, bytes, counts"""
    gi, gv, gc = (np.asarray(a) for a in got)
    wi, wv, wc = want
    wi = np.where(wi >= 0, wi + col0, -1)
    assert np.array_equal(gc.astype(np.int64), wc), (gc[:8], wc[:8])
    assert np.array_equal(gi.astype(np.int64), wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(np.ascontiguousarray(gv).view(np.uint32), np.ascontiguousarray(wv).view(np.uint32))


def _cases():
    rng = np.random.default_rng(20261018)
    out = {}
    out["eighths_40x600_k50"] = ((np.round(rng.random((40, 600)) * 8) / 8).astype(np.float32), 50)
    out["one_column_3x1_k1"] = (rng.random((3, 1)).astype(np.float32), 1)
    out["padded_5x37_k50"] = (rng.random((5, 37)).astype(np.float32), 50)
    out["k1024_8x5000"] = (rng.random((8, 5000)).astype(np.float32), 1024)
    out["all_equal_4x5000_k100"] = (np.full((4, 5000), 0.375, np.float32), 100)
    d = (1.0 + rng.random((4, 6000))).astype(np.float32)
    for i in range(4):                       # 30 + i smaller values, then 3000 copies of 0.5: the 64th falls inside them
        perm = rng.permutation(6000)
        d[i, perm[:3000]] = 0.5
        d[i, perm[3000:3030 + i]] = rng.random(30 + i).astype(np.float32) * 0.25
    out["ties_at_kth_4x6000_k64"] = (d, 64)
    out["msmt17_row_6x82161_k50"] = (rng.random((6, 82161)).astype(np.float32), 50)
    d = rng.standard_normal((3, 300)).astype(np.float32)
    d[:, ::5] = -0.0
    d[:, 1::5] = 0.0
    d[1] = np.where(rng.random(300) < 0.5, -0.0, 0.0)
    out["signed_zeros_3x300_k120"] = (d, 120)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_abi_plain(name):
    from utils.metrics import rank_lists
    d, k = CASES[name]
    rc, idx, val, cnt = _abi(torch.from_numpy(d).cuda(), k)
    assert rc == 0
    assert _guard_untouched(idx, val, cnt)
    _same((idx[:-1], val[:-1], cnt[:-1]), rank_lists(d, k))
    if name.startswith("all_equal"):
        assert np.array_equal(idx[:-1], np.tile(np.arange(k), (4, 1)))
    if name.startswith("signed_zeros"):
        assert np.signbit(val[1, :k]).any() and not np.signbit(val[1, :k]).all()      # the entries' own bits


def test_abi_limits_and_argument_errors():
    from mpreid import _lib
    from utils.metrics import rank_lists
    L = _lib.load()
    d = np.random.default_rng(3).random((4, 90)).astype(np.float32)
    dt = torch.from_numpy(d).cuda()
    q, g = np.zeros(4, np.int64), np.zeros(90, np.int64)
    rc, idx, val, cnt = _abi(dt, 1025)
    assert rc == _lib.ERR_UNSUPPORTED and b"1024" in L.mpreid_last_error()
    assert np.all(idx == FILL) and np.all(cnt == FILL)                       # nothing was launched
    rc, idx, val, cnt = _abi(dt, 1024)                                        # the next valid call works
    assert rc == 0
    _same((idx[:-1], val[:-1], cnt[:-1]), rank_lists(d, 1024))
    assert _abi(dt, 0)[0] == _lib.ERR_ARG
    assert _abi(dt, 5, nq=-1)[0] == _lib.ERR_ARG
    assert _abi(dt, 5, ng=-1)[0] == _lib.ERR_ARG
    assert _abi(dt, 5, labels=(q, g, None, None))[0] == _lib.ERR_ARG
    assert _abi(dt, 5, labels=(q, g, q, None))[0] == _lib.ERR_ARG
    assert _abi(dt, 5, col0=2 ** 31 - 90)[0] == _lib.ERR_ARG
    rc, idx, val, cnt = _abi(dt, 5, col0=2 ** 31 - 91)                        # the largest legal index: 2^31 - 2
    assert rc == 0
    _same((idx[:-1], val[:-1], cnt[:-1]), rank_lists(d, 5), col0=2 ** 31 - 91)
    # empty blocks: nq == 0 and (ng == 0 with carry) are no-ops, ng == 0 without carry writes empty lists
    rc, idx, val, cnt = _abi(dt, 5, nq=0)
    assert rc == 0 and np.all(idx == FILL) and np.all(cnt == FILL)
    rc, idx, val, cnt = _abi(dt, 5, ng=0)
    assert rc == 0 and np.all(idx[:-1] == -1) and np.all(np.isposinf(val[:-1])) and np.all(cnt[:-1] == 0)
    assert _guard_untouched(idx, val, cnt)
    keep = (np.full((4, 5), 3, np.int32), np.full((4, 5), 0.25, np.float32), np.full(4, 2, np.int32))
    rc, idx, val, cnt = _abi(dt, 5, ng=0, carry=keep)
    assert rc == 0 and np.array_equal(idx, keep[0]) and np.array_equal(val, keep[1]) and np.array_equal(cnt, keep[2])


@pytest.fixture(scope="module")
def samecam(golden):
    z = golden("eval_func_samecam.npz")
    return z["d"], z["q_pid"], z["g_pid"], z["q_cam"], z["g_cam"]


def test_leading_dimension_and_alignment(samecam):
    """column slices of a wider matrix: a row pointer 4 and 12 bytes off a 16-byte boundary, ld = 384, odd lengths"""
    from mpreid import ops
    from utils.metrics import rank_lists
    d = samecam[0]
    dt = torch.from_numpy(d).cuda()
    for c0, c1, k in ((1, 202, 50), (3, 384, 50), (1, 202, 300), (2, 7, 3)):
        rc, idx, val, cnt = _abi(dt[:, c0:c1], k, col0=c0)
        assert rc == 0
        _same((idx[:-1], val[:-1], cnt[:-1]), rank_lists(d[:, c0:c1], k), col0=c0)
        got = ops.rank_topk(dt[:, c0:c1], k, col0=c0)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        _same([t.cpu().numpy() for t in got], rank_lists(d[:, c0:c1], k), col0=c0)


def _built_filter_case():
    rng = np.random.default_rng(77)
    nq, ng, k = 6, 500, 40
    d = rng.random((nq, ng)).astype(np.float32)
    q_pid, q_cam = np.arange(nq), np.arange(nq) % 3
    g_pid, g_cam = rng.integers(100, 200, ng), rng.integers(0, 3, ng)
    order = np.argsort(d, axis=1, kind="stable")
    junk0 = order[0, [0, 3, 17, 39, 40]]                         # row 0: junk inside and just past the top-k
    g_pid[junk0], g_cam[junk0] = q_pid[0], q_cam[0]
    same_pid_other_cam = order[0, [1, 5]]                        # pid match alone is not junk
    g_pid[same_pid_other_cam], g_cam[same_pid_other_cam] = q_pid[0], (q_cam[0] + 1) % 3
    return d, q_pid, g_pid, q_cam, g_cam, k


def test_camera_filter(samecam):
    from utils.metrics import rank_lists, rank_lists_device
    d, q_pid, g_pid, q_cam, g_cam = samecam
    dt = torch.from_numpy(d).cuda()
    for k in (1, 50, 384):
        want = rank_lists(d, k, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
        rc, idx, val, cnt = _abi(dt, k, labels=(q_pid, g_pid, q_cam, g_cam))
        assert rc == 0 and _guard_untouched(idx, val, cnt)
        _same((idx[:-1], val[:-1], cnt[:-1]), want)
        got = rank_lists_device(dt, k, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64
        _same(got, want)
        _same(rank_lists_device(dt, k, q_pid, g_pid, q_cam, g_cam), rank_lists(d, k))       # labels given, filter off
    assert not np.array_equal(rank_lists(d, 50)[0], rank_lists(d, 50, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)[0])
    # a built case: junk inside the top-k
    d, q_pid, g_pid, q_cam, g_cam, k = _built_filter_case()
    want = rank_lists(d, k, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    plain = rank_lists(d, k)
    assert not np.array_equal(want[0][0], plain[0][0]) and np.array_equal(want[0][1:], plain[0][1:])   # precondition
    rc, idx, val, cnt = _abi(torch.from_numpy(d).cuda(), k, labels=(q_pid, g_pid, q_cam, g_cam))
    assert rc == 0
    _same((idx[:-1], val[:-1], cnt[:-1]), want)
    # row 0: the whole gallery is junk (cnt 0); row 1: fewer than k kept items; row 2: untouched
    d = np.random.default_rng(5).random((3, 300)).astype(np.float32)
    q_pid, q_cam = np.array([1, 2, 3]), np.array([0, 1, 0])
    g_pid, g_cam = np.full(300, 1), np.zeros(300, np.int64)
    for g_pid_case, counts in ((g_pid, [0, 64, 64]), (np.where(np.arange(300) < 280, 2, 1), [64, 20, 64])):
        g_cam_case = np.where(g_pid_case == 2, 1, 0)
        want = rank_lists(d, 64, q_pid, g_pid_case, q_cam, g_cam_case, remove_same_cam=True)
        assert want[2].tolist() == counts
        rc, idx, val, cnt = _abi(torch.from_numpy(d).cuda(), 64, labels=(q_pid, g_pid_case, q_cam, g_cam_case))
        assert rc == 0
        _same((idx[:-1], val[:-1], cnt[:-1]), want)
    d = np.random.default_rng(6).random((2, 300)).astype(np.float32)
    g_pid, g_cam = np.where(np.arange(300) % 10 == 0, 9, 2), np.ones(300, np.int64)      # row 1 keeps 30 of 300: < k
    want = rank_lists(d, 64, np.array([1, 2]), g_pid, np.array([1, 1]), g_cam, remove_same_cam=True)
    assert want[2].tolist() == [64, 30]
    rc, idx, val, cnt = _abi(torch.from_numpy(d).cuda(), 64, labels=(np.array([1, 2]), g_pid, np.array([1, 1]), g_cam))
    assert rc == 0
    _same((idx[:-1], val[:-1], cnt[:-1]), want)


@pytest.fixture(scope="module")
def carry_case():
    rng = np.random.default_rng(99)
    d = (np.round(rng.random((8, 5000)) * 16) / 16).astype(np.float32)          # ~300 copies of every value
    q_pid, q_cam = np.arange(8) % 4, np.arange(8) % 2
    g_pid, g_cam = rng.integers(0, 4, 5000), rng.integers(0, 2, 5000)
    return d, torch.from_numpy(d).cuda(), (q_pid, g_pid, q_cam, g_cam)


def _blocks(n, width, shuffled):
    b = [(c0, min(c0 + width, n)) for c0 in range(0, n, width)]
    if shuffled:
        b = [b[i] for i in np.random.default_rng(width).permutation(len(b))]
    return b


@pytest.mark.parametrize("width", [7, 64, 1000, 4999])
@pytest.mark.parametrize("shuffled", [False, True])
def test_carry_equals_the_single_call(carry_case, width, shuffled):
    from mpreid import ops
    from utils.metrics import rank_lists
    d, dt, _ = carry_case
    k = 50
    single = [t.cpu().numpy() for t in ops.rank_topk(dt, k)]
    _same(single, rank_lists(d, k))
    out = None
    for c0, c1 in _blocks(5000, width, shuffled):
        out = ops.rank_topk(dt[:, c0:c1], k, col0=c0, carry=out)
    for a, b in zip(out, single):
        assert a.cpu().numpy().tobytes() == b.tobytes()


def test_carry_with_the_filter(carry_case):
    from mpreid import ops
    from utils.metrics import rank_lists
    d, dt, (q_pid, g_pid, q_cam, g_cam) = carry_case
    k = 50
    want = rank_lists(d, k, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    assert not np.array_equal(want[0], rank_lists(d, k)[0])
    single = [t.cpu().numpy() for t in ops.rank_topk(dt, k, labels=(q_pid, g_pid, q_cam, g_cam))]
    _same(single, want)
    out = None
    for c0, c1 in _blocks(5000, 64, True):
        out = ops.rank_topk(dt[:, c0:c1], k, col0=c0, labels=(q_pid, g_pid[c0:c1], q_cam, g_cam[c0:c1]), carry=out)
    for a, b in zip(out, single):
        assert a.cpu().numpy().tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def feats(golden):
    from mpreid import ops
    z = golden("r1_map_eval.npz")
    f = ops.l2_normalize(torch.from_numpy(z["raw"]).cuda())
    return f[:96].contiguous(), f[96:].contiguous(), z


def _blocked_matrix(qf, gf, chunk, mode):
    from mpreid import ops
    return np.concatenate([ops.euclidean_distance(qf, gf[c0:c0 + chunk], mode=mode).cpu().numpy()
                           for c0 in range(0, gf.shape[0], chunk)], axis=1)


@pytest.mark.parametrize("mode_name", ["exact", "split3", "f16"])
def test_search_topk_small(feats, mode_name):
    from mpreid import ops
    from utils.metrics import rank_lists
    qf, gf, _ = feats
    mode = {"exact": ops.GEMM_F32_EXACT, "split3": ops.GEMM_F16_SPLIT3, "f16": ops.GEMM_F16_FAST}[mode_name]
    k = 60
    full = rank_lists(ops.euclidean_distance(qf, gf, mode=mode).cpu().numpy(), k)
    for chunk in (1, 50, 383, 384, 1000):
        got = [t.cpu().numpy() for t in ops.search_topk(qf, gf, k, mode=mode, chunk=chunk)]
        assert got[0].shape == (96, k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
        _same(got, rank_lists(_blocked_matrix(qf, gf, chunk, mode), k))
        same_as_full = np.array_equal(got[0].astype(np.int64), full[0]) and \
            np.array_equal(got[1].view(np.uint32), full[1].view(np.uint32))
        print(f"search_topk mode={mode_name} chunk={chunk}: lists equal those of the unblocked matrix: {same_as_full}")
        if mode == ops.GEMM_F32_EXACT:
            assert same_as_full
    _same([t.cpu().numpy() for t in ops.search_topk(qf, gf, k, mode=mode)], full)          # default chunk: one block


def test_search_topk_with_labels_and_default_chunk(feats):
    from mpreid import ops
    from utils.metrics import rank_lists
    qf, gf, z = feats
    pid, cam = z["pid"], z["cam"]
    d = ops.euclidean_distance(qf, gf).cpu().numpy()
    want = rank_lists(d, 25, pid[:96], pid[96:], cam[:96], cam[96:], remove_same_cam=True)
    assert not np.array_equal(want[0], rank_lists(d, 25)[0])
    for chunk in (None, 100):
        got = ops.search_topk(qf, gf, 25, chunk=chunk, q_pids=pid[:96], g_pids=pid[96:], q_camids=cam[:96], g_camids=cam[96:])
        _same([t.cpu().numpy() for t in got], want)


def test_search_topk_20000():
    from mpreid import ops
    from utils.metrics import rank_lists
    g = torch.Generator().manual_seed(1234)
    qf = ops.l2_normalize(torch.randn((64, 256), generator=g).cuda())
    gf = ops.l2_normalize(torch.randn((20000, 256), generator=g).cuda())
    got = [t.cpu().numpy() for t in ops.search_topk(qf, gf, 100, chunk=3000)]
    _same(got, rank_lists(_blocked_matrix(qf, gf, 3000, ops.GEMM_F32_EXACT), 100))
    _same(got, rank_lists(ops.euclidean_distance(qf, gf).cpu().numpy(), 100))


def _run_evaluator(z, rerank, same_cam, list_k):
    from utils.metrics import R1_mAP_eval
    ev = R1_mAP_eval(96, feat_norm=True, reranking=rerank)
    ev.remove_same_cam = same_cam
    ev.rank_list_k = list_k
    ev.reset()
    for s in range(0, 480, 128):
        ev.update((torch.from_numpy(z["raw"][s:s + 128]).cuda(), tuple(int(p) for p in z["pid"][s:s + 128]),
                   tuple(int(c) for c in z["cam"][s:s + 128])))
    return ev, ev.compute()


@pytest.mark.parametrize("rerank", [False, True])
@pytest.mark.parametrize("same_cam", [False, True])
def test_evaluator_lists(feats, monkeypatch, rerank, same_cam):
    from mpreid import _lib
    from utils.metrics import rank_lists
    z = feats[2]
    ev, out = _run_evaluator(z, rerank, same_cam, 20)
    distmat = out[2]
    want = rank_lists(distmat, 20, z["pid"][:96], z["pid"][96:], z["cam"][:96], z["cam"][96:], remove_same_cam=same_cam)
    assert len(ev.last_rank_lists) == 3
    for a, b in zip(ev.last_rank_lists, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()

    def refuse(*a):
        raise AssertionError("mpreid_rank_topk was called with rank_list_k = 0")
    monkeypatch.setattr(_lib.load(), "mpreid_rank_topk", refuse)
    ev0, out0 = _run_evaluator(z, rerank, same_cam, 0)
    assert ev0.last_rank_lists is None and len(out) == len(out0) == 7
    assert np.array_equal(out[0], out0[0]) and out[0].dtype == out0[0].dtype and float(out[1]) == float(out0[1])
    assert out[2].tobytes() == out0[2].tobytes() and list(out[3]) == list(out0[3]) and list(out[4]) == list(out0[4])
    assert out[5].numpy().tobytes() == out0[5].numpy().tobytes() and out[6].numpy().tobytes() == out0[6].numpy().tobytes()


def test_evaluator_refuses_lists_under_a_process_group(feats):
    from emulated_group import EmulatedWorld
    from utils.metrics import R1_mAP_eval
    z = feats[2]

    def rank_fn(rank):
        ev = R1_mAP_eval(96)
        ev.rank_list_k = 5
        ev.reset()
        ev.update((torch.from_numpy(z["raw"][:64]).cuda(), tuple(int(p) for p in z["pid"][:64]),
                   tuple(int(c) for c in z["cam"][:64])))
        with pytest.raises(NotImplementedError, match="ranked lists are single-process"):
            ev.compute()
        return True
    assert EmulatedWorld(2).run(rank_fn) == [True, True]


OVERRIDES = ["DATASETS.SYNTH_QUERY", 24, "DATASETS.SYNTH_GALLERY", 72, "DATASETS.SYNTH_IDS", 6, "TEST.IMS_PER_BATCH", 32]


def _cli():
    spec = importlib.util.spec_from_file_location("mpreid_test_cli_rank_lists", os.path.join(ROOT, "mp-reid_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_writes_the_lists(tmp_path):
    from config import cfg_base
    from datasets.make_dataloader import make_dataloader
    from processor.processor import do_inference
    from utils.metrics import rank_lists
    base = ["--config_file", ""] + [str(x) for x in OVERRIDES]
    with_dir, without = tmp_path / "with", tmp_path / "without"
    res = _cli().main(base + ["TEST.RANK_LIST_K", "10", "OUTPUT_DIR", str(with_dir)])
    ev = do_inference.last_evaluator
    name = with_dir / "rank_lists.npz"
    assert name.exists()
    z = np.load(str(name))
    assert z["indices"].shape == (24, 10) and z["indices"].dtype == np.int32 and z["distances"].shape == (24, 10)
    assert z["counts"].shape == (24,) and np.all(z["counts"] == 10) and int(z["k"]) == 10
    assert z["q_pids"].shape == (24,) and z["g_pids"].shape == (72,) and z["q_paths"].shape == (24,) and z["g_paths"].shape == (72,)
    assert bool(z["remove_same_cam"]) is False and bool(z["reranking"]) is False
    distmat = ev.compute()[2]
    want = rank_lists(distmat, 10)
    assert np.array_equal(z["indices"], want[0]) and np.array_equal(z["distances"].view(np.uint32), want[1].view(np.uint32))
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(OVERRIDES)
    cfg.freeze()
    paths = [p for batch in make_dataloader(cfg)[2] for p in batch[5]]
    assert z["q_paths"].tolist() == [str(p) for p in paths[:24]] and z["g_paths"].tolist() == [str(p) for p in paths[24:]]
    assert z["g_paths"][z["indices"][0, 0]] == str(paths[24 + want[0][0, 0]])
    assert np.array_equal(z["g_pids"], np.asarray(ev.pids[24:]))
    # without the key: no file, the same result
    res0 = _cli().main(base + ["OUTPUT_DIR", str(without)])
    assert not (without / "rank_lists.npz").exists() and do_inference.last_evaluator.last_rank_lists is None
    assert float(res0[0]) == float(res[0]) and float(res0[1]) == float(res[1])
    # an explicit file name wins over OUTPUT_DIR
    mine = tmp_path / "elsewhere" / "mine.npz"
    _cli().main(base + ["TEST.RANK_LIST_K", "3", "TEST.RANK_LIST_FILE", str(mine), "TEST.REMOVE_SAME_CAM", "True"])
    z = np.load(str(mine))
    assert z["indices"].shape == (24, 3) and bool(z["remove_same_cam"]) is True
