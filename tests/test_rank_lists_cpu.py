"""Ranked gallery lists, host side: utils.metrics.rank_lists (the numpy definition) against the reference's own line
(utils/metrics.py:39, ``np.argsort(distmat, axis=1)``) on a reference-derived fixture, the tie / signed-zero / junk rules,
the argument errors of the device entry points (raised before a device is needed), the config keys and the .npz writer."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def fixture(golden):
    z = golden("eval_func_samecam.npz")
    return z["d"], z["q_pid"], z["g_pid"], z["q_cam"], z["g_cam"]


def _row_definition(row, k, junk=None):
    """one row, written from the definition: ascending (distance, index), junk dropped, first k, padded"""
    items = sorted((float(v) + 0.0, j) for j, v in enumerate(row) if junk is None or not junk[j])
    items = items[:k]
    idx = np.full(k, -1, np.int64)
    val = np.full(k, np.inf, np.float32)
    for t, (_, j) in enumerate(items):
        idx[t], val[t] = j, row[j]
    return idx, val, len(items)


@pytest.mark.parametrize("k", [1, 50, 384, 500])
def test_host_lists_are_reference_line_39(fixture, k):
    from utils.metrics import rank_lists
    d = fixture[0]
    assert d.shape == (48, 384)
    assert np.array_equal(np.argsort(d, axis=1), np.argsort(d, axis=1, kind="stable"))   # tie-free: the default is a yardstick
    idx, val, cnt = rank_lists(d, k)
    assert idx.dtype == np.int64 and val.dtype == np.float32 and cnt.dtype == np.int64
    assert idx.shape == (48, k) and val.shape == (48, k) and cnt.shape == (48,)
    kk = min(k, 384)
    want = np.argsort(d, axis=1)[:, :k]
    assert np.array_equal(idx[:, :kk], want) and np.array_equal(cnt, np.full(48, kk))
    assert np.array_equal(val[:, :kk].view(np.uint32), np.take_along_axis(d, want, axis=1).view(np.uint32))
    assert np.all(idx[:, kk:] == -1) and np.all(np.isposinf(val[:, kk:]))


@pytest.mark.parametrize("k", [1, 50, 384])
def test_host_lists_same_camera_filter(fixture, k):
    from utils.metrics import rank_lists
    d, q_pid, g_pid, q_cam, g_cam = fixture
    junk = (g_pid[None, :] == q_pid[:, None]) & (g_cam[None, :] == q_cam[:, None])
    per_row = junk.sum(1)
    assert per_row.min() == 0 and per_row.max() == 10
    idx, val, cnt = rank_lists(d, k, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    for i in range(d.shape[0]):
        wi, wv, wc = _row_definition(d[i], k, junk[i])
        assert np.array_equal(idx[i], wi) and np.array_equal(val[i].view(np.uint32), wv.view(np.uint32)) and cnt[i] == wc
    # labels given, filter off: the unfiltered lists
    plain = rank_lists(d, k)
    off = rank_lists(d, k, q_pid, g_pid, q_cam, g_cam)
    assert all(np.array_equal(a, b) for a, b in zip(plain, off))


def test_host_ties_and_signed_zeros():
    from utils.metrics import rank_lists
    rng = np.random.default_rng(7)
    d = (np.round(rng.random((12, 300)) * 8) / 8).astype(np.float32)      # eighths: ~33 copies of each value
    d[3, ::3] = -0.0
    d[3, 1::3] = 0.0
    d[5] = np.where(rng.random(300) < 0.5, -0.0, 0.0).astype(np.float32)
    d[7, :10] = [-1.5, -0.0, 0.0, -1.5, 2.0, -0.0, -3.0, 0.0, 0.0, -0.0]
    for k in (1, 40, 300):
        idx, val, cnt = rank_lists(d, k)
        for i in range(d.shape[0]):
            wi, wv, wc = _row_definition(d[i], k)
            assert np.array_equal(idx[i], wi) and cnt[i] == wc
            assert np.array_equal(val[i].view(np.uint32), wv.view(np.uint32))      # -0 stays -0, +0 stays +0
    idx, val, _ = rank_lists(d, 300)
    assert np.array_equal(idx[5], np.arange(300))                                   # all zeros of either sign: index order
    assert np.signbit(val[5]).any() and not np.signbit(val[5]).all()


def test_host_all_junk_row_and_short_row():
    from utils.metrics import rank_lists
    rng = np.random.default_rng(11)
    d = rng.random((3, 20)).astype(np.float32)
    q_pid, q_cam = np.array([1, 2, 3]), np.array([0, 0, 0])
    g_pid, g_cam = np.full(20, 1), np.zeros(20, np.int64)       # row 0: every gallery item is junk; rows 1, 2: none is
    idx, val, cnt = rank_lists(d, 18, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    assert cnt.tolist() == [0, 18, 18]
    assert np.all(idx[0] == -1) and np.all(np.isposinf(val[0]))
    assert np.array_equal(idx[2], np.argsort(d[2], kind="stable")[:18])
    g_pid[15:] = 2                                              # row 0: 15 junk items, 5 kept; row 1: 5 junk, 15 kept
    idx, val, cnt = rank_lists(d, 18, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    assert cnt.tolist() == [5, 15, 18]
    assert np.array_equal(idx[0, :5], 15 + np.argsort(d[0, 15:], kind="stable")) and np.all(idx[0, 5:] == -1)
    assert np.array_equal(idx[1, :15], np.argsort(d[1, :15], kind="stable")) and np.all(idx[1, 15:] == -1)
    assert np.all(np.isposinf(val[1, 15:])) and np.array_equal(val[1, :15], d[1, idx[1, :15]])


def test_argument_errors_need_no_device():
    from mpreid import ops
    from utils.metrics import rank_lists, rank_lists_device
    d = torch.zeros((4, 9))
    q, g = np.zeros(4, np.int64), np.zeros(9, np.int64)
    assert ops.RANK_TOPK_MAX == 1024
    for fn in (lambda k: ops.rank_topk(d, k), lambda k: ops.search_topk(d, torch.zeros((5, 9)), k),
               lambda k: rank_lists(d.numpy(), k), lambda k: rank_lists_device(d, k)):
        for k in (0, -3):
            with pytest.raises(ValueError, match="at least one"):
                fn(k)
        with pytest.raises(ValueError, match="1024"):
            fn(1025)
    # partial label sets
    with pytest.raises(ValueError, match="all four"):
        ops.rank_topk(d, 3, labels=(q, g, None, None))
    with pytest.raises(ValueError, match="all four"):
        ops.search_topk(d, torch.zeros((9, 9)), 3, q_pids=q, g_pids=g)
    for fn in (rank_lists, rank_lists_device):
        with pytest.raises(ValueError, match="remove_same_cam"):
            fn(d if fn is rank_lists_device else d.numpy(), 3, q, g, remove_same_cam=True)
    # shapes
    with pytest.raises(ValueError, match="g_pids"):
        ops.rank_topk(d, 3, labels=(q, g[:8], q, g))
    with pytest.raises(ValueError, match="q_camids"):
        rank_lists(d.numpy(), 3, q, g, q[:2], g, remove_same_cam=True)
    with pytest.raises(ValueError, match="same number of columns"):
        ops.search_topk(d, torch.zeros((5, 8)), 3)
    with pytest.raises(ValueError, match="2-D"):
        ops.rank_topk(torch.zeros(9), 3)
    with pytest.raises(ValueError, match="chunk"):
        ops.search_topk(d, torch.zeros((5, 9)), 3, chunk=0)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.rank_topk(d, 3, col0=2 ** 31 - 9)
    with pytest.raises(ValueError, match="carry"):
        ops.rank_topk(d, 3, carry=(torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 3)),
                                   torch.zeros(4, dtype=torch.int32)))


def test_config_defaults_and_evaluator_attributes():
    from config import cfg_base
    from utils.metrics import R1_mAP_eval
    assert cfg_base.TEST.RANK_LIST_K == 0 and cfg_base.TEST.RANK_LIST_FILE == ""
    ev = R1_mAP_eval(10)
    assert ev.rank_list_k == 0 and ev.last_rank_lists is None


def test_rank_list_file_name_rule():
    from config import cfg_base
    from processor.processor import rank_list_file
    cfg = cfg_base.clone()
    cfg.defrost()
    assert rank_list_file(cfg) == ""                                 # no file name, no OUTPUT_DIR: nothing is written
    cfg.OUTPUT_DIR = "some_dir"
    assert rank_list_file(cfg).replace("\\", "/") == "some_dir/rank_lists.npz"
    cfg.TEST.RANK_LIST_FILE = "lists/mine.npz"
    assert rank_list_file(cfg) == "lists/mine.npz"


def test_writer_round_trip(tmp_path, fixture):
    from processor.processor import write_rank_lists
    from utils.metrics import rank_lists
    d, q_pid, g_pid, q_cam, g_cam = fixture
    lists = rank_lists(d, 400, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)       # padded: k > kept items
    pids, cams = np.concatenate([q_pid, g_pid]), np.concatenate([q_cam, g_cam])
    paths = ["img_%04d.jpg" % i for i in range(pids.size)]
    name = write_rank_lists(str(tmp_path / "sub" / "lists"), lists, list(pids), list(cams), paths, 48, True, False)
    assert name.endswith("lists.npz")
    z = np.load(name)
    assert set(z.files) == {"indices", "distances", "counts", "q_pids", "q_camids", "g_pids", "g_camids", "q_paths",
                            "g_paths", "k", "remove_same_cam", "reranking"}
    assert z["indices"].dtype == np.int32 and z["distances"].dtype == np.float32 and z["counts"].dtype == np.int32
    assert np.array_equal(z["indices"], lists[0]) and np.array_equal(z["counts"], lists[2])
    assert np.array_equal(z["distances"].view(np.uint32), lists[1].view(np.uint32))
    assert np.array_equal(z["q_pids"], q_pid) and np.array_equal(z["g_pids"], g_pid)
    assert np.array_equal(z["q_camids"], q_cam) and np.array_equal(z["g_camids"], g_cam)
    assert z["q_paths"].tolist() == paths[:48] and z["g_paths"].tolist() == paths[48:]
    assert int(z["k"]) == 400 and bool(z["remove_same_cam"]) is True and bool(z["reranking"]) is False
    assert z["g_paths"][z["indices"][0, 0]] == paths[48 + lists[0][0, 0]]
