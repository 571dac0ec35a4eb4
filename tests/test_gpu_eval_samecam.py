"""GPU side of the Market-1501 protocol (same-identity same-camera gallery items removed): the camera-aware ranking kernel
through the C ABI (mpreid_eval_rank_positions_cam), eval_func_device, R1_mAP_eval (single-process and virtual ranks) and
do_inference with TEST.REMOVE_SAME_CAM.  The oracle has no camera argument: the yardsticks are the reference's own
eval_func with its filter line restored (tests/golden/eval_func_samecam.npz; reference utils/metrics.py:28-88, line 54) and
the host eval_func(..., remove_same_cam=True), itself pinned to that golden by tests/test_eval_samecam_cpu.py."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

from emulated_group import EmulatedWorld

pytestmark = pytest.mark.gpu


def _np_positions(d, q_pid, g_pid, q_cam, g_cam, rcap):
    """(pos [nq][rcap] padded with -1, cnt [nq]) from the definition: stable order, junk removed, positions among kept;
    q_cam None: no filter"""
    nq = d.shape[0]
    pos, cnt = np.full((nq, rcap), -1, np.int32), np.zeros(nq, np.int32)
    for q in range(nq):
        order = np.argsort(d[q], kind="stable")
        match = g_pid[order] == q_pid[q]
        junk = match & (g_cam[order] == q_cam[q]) if q_cam is not None else np.zeros_like(match)
        p = (np.cumsum(~junk) - 1)[match & ~junk]
        pos[q, :p.size], cnt[q] = p, p.size
    return pos, cnt


def _abi_positions(d, q_pid, g_pid, q_cam, g_cam, rcap):
    from mpreid import _lib
    L = _lib.load()
    dev = _lib.require_gpu()
    dt = torch.from_numpy(d).to(dev)
    t = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(dev) if x is not None else None
         for x in (q_pid, g_pid, q_cam, g_cam)]
    pos = torch.full((d.shape[0], rcap), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((d.shape[0],), -7, dtype=torch.int32, device=dev)
    p = [C.c_void_p(x.data_ptr()) if x is not None else None for x in t]
    if q_cam is None:
        rc = L.mpreid_eval_rank_positions(C.c_void_p(dt.data_ptr()), dt.stride(0), d.shape[0], d.shape[1], p[0], p[1], rcap,
                                          C.c_void_p(pos.data_ptr()), C.c_void_p(cnt.data_ptr()), _lib.stream_ptr())
    else:
        rc = L.mpreid_eval_rank_positions_cam(C.c_void_p(dt.data_ptr()), dt.stride(0), d.shape[0], d.shape[1], p[0], p[1],
                                              p[2], p[3], rcap, C.c_void_p(pos.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                              _lib.stream_ptr())
    _lib.check(rc, "eval_rank_positions")
    torch.cuda.synchronize()
    return pos.cpu().numpy(), cnt.cpu().numpy()


def test_eval_func_device_samecam_vs_reference_golden(golden):
    from utils.metrics import eval_func, eval_func_device
    g = golden("eval_func_samecam.npz")
    dt = torch.from_numpy(g["d"]).cuda()
    cmc, mAP = eval_func_device(dt, g["q_pid"], g["g_pid"], g["q_cam"], g["g_cam"], remove_same_cam=True)
    print("golden: |dmAP|", abs(mAP - float(g["mAP"])), "max |dcmc|", np.abs(cmc - g["cmc"]).max())
    assert cmc.dtype == np.float32 and np.array_equal(cmc, g["cmc"])
    assert abs(mAP - float(g["mAP"])) < 1e-12
    # non-contiguous rows (a column block of a wider matrix) through the leading dimension, against the host
    cmc2, mAP2 = eval_func_device(dt[:, :200], g["q_pid"], g["g_pid"][:200], g["q_cam"], g["g_cam"][:200],
                                  remove_same_cam=True)
    cmc3, mAP3 = eval_func(g["d"][:, :200], g["q_pid"], g["g_pid"][:200], g["q_cam"], g["g_cam"][:200], remove_same_cam=True)
    assert np.array_equal(cmc2, cmc3) and abs(mAP2 - mAP3) < 1e-12


def _case(name):
    """(d, q_pid, g_pid, q_cam, g_cam): A ties (distances in eighths), B ~1000 pid matches per row (a sort longer than one
    pass of 256 threads), C the 4096-entry LDS size, D the largest one (8192 pid matches, ties in 1/64), E over capacity
    (9000 pid matches: the row is ranked on the host, with the same filter)"""
    if name in ("A", "B"):
        nq, ng, ids, cams = {"A": (40, 600, 10, 3), "B": (64, 3000, 3, 2)}[name]
        rng = np.random.default_rng(nq + ng)
        d = rng.random((nq, ng)).astype(np.float32)
        if name == "A":
            d = np.round(d * 8) / 8
        q_pid, g_pid = rng.integers(0, ids, nq), rng.integers(0, ids, ng)
        q_pid[0] = 10_000
        return d, q_pid, g_pid, rng.integers(0, cams, nq), rng.integers(0, cams, ng)
    nq, ng, big, ties = {"C": (10, 4100, 4000, False), "D": (12, 12000, 8192, True), "E": (12, 20000, 9000, False)}[name]
    rng = np.random.default_rng(ng + big)
    d = rng.random((nq, ng)).astype(np.float32)
    if ties:
        d = np.round(d * 64) / 64
    g_pid = np.full(ng, 7, np.int64)
    g_pid[big:] = rng.integers(100, 140, ng - big)
    g_pid = g_pid[rng.permutation(ng)]
    q_pid = rng.integers(100, 140, nq)
    q_pid[[3, 8]] = 7
    return d, q_pid, g_pid, rng.integers(0, 2, nq), rng.integers(0, 2, ng)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_eval_func_device_samecam_vs_host(name):
    import utils.metrics as M
    d, q_pid, g_pid, q_cam, g_cam = _case(name)
    cmc_h, map_h = M.eval_func(d, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    cmc_u, map_u = M.eval_func(d, q_pid, g_pid, q_cam, g_cam)
    assert not np.array_equal(cmc_h, cmc_u) and map_h != map_u        # precondition: the filter matters on this input
    M._warned_host_ranking = False
    cmc_d, map_d = M.eval_func_device(torch.from_numpy(d).cuda(), q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    print(name, "|dmAP|", abs(map_d - map_h), "max |dcmc|", np.abs(cmc_d - cmc_h).max(), "host rows:", M._warned_host_ranking)
    assert cmc_d.dtype == np.float32 and np.array_equal(cmc_d, cmc_h)
    assert abs(map_d - map_h) < 1e-12
    if name == "D":
        assert M._warned_host_ranking is False      # 8192 pid matches fit the largest LDS size: the row ran on the device


def test_eval_func_device_samecam_all_queries_invalid():
    from utils.metrics import eval_func_device
    d = torch.rand((4, 60), device="cuda")
    q_pid, g_pid = np.array([0, 1, 2, 100]), np.arange(60) % 7
    q_cam, g_cam = np.array([3, 4, 5, 0]), np.full(60, -1)
    for q in range(3):
        g_cam[g_pid == q_pid[q]] = q_cam[q]           # every match sits on the query's camera
    with pytest.raises(AssertionError, match="all query identities do not appear in gallery"):
        eval_func_device(d, q_pid, g_pid, q_cam, g_cam, remove_same_cam=True)
    cmc, mAP = eval_func_device(d, q_pid, g_pid, q_cam, g_cam)     # (valid without the filter)
    assert 0.0 < mAP <= 1.0


def test_remove_same_cam_false_with_camera_ids_is_the_unfiltered_path(monkeypatch):
    """camera ids given, filter off: the bytes of the call without camera ids, through the unfiltered entry point (the
    camera-aware one is not called at all)"""
    from mpreid import _lib
    from utils.metrics import eval_func_device
    d, q_pid, g_pid, q_cam, g_cam = _case("A")
    dt = torch.from_numpy(d).cuda()
    want = eval_func_device(dt, q_pid, g_pid)

    def refuse(*a):
        raise AssertionError("the camera-aware kernel was launched with remove_same_cam=False")
    monkeypatch.setattr(_lib.load(), "mpreid_eval_rank_positions_cam", refuse)
    for got in (eval_func_device(dt, q_pid, g_pid, q_cam, g_cam), eval_func_device(dt, q_pid, g_pid, q_cam, g_cam, 50, None, False)):
        assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype and float(got[1]) == float(want[1])


def test_abi_positions_cam_vs_numpy():
    nq, ng, ids, cams, rcap = 50, 400, 20, 3, 40
    rng = np.random.default_rng(nq + ng)
    d = rng.random((nq, ng)).astype(np.float32)
    q_pid, g_pid = rng.integers(0, ids, nq), rng.integers(0, ids, ng)
    q_cam, g_cam = rng.integers(0, cams, nq), rng.integers(0, cams, ng)
    q_pid[0] = 10_000                                   # no pid match: cnt 0
    q_pid[1], g_pid[:4], g_cam[:4] = 5_000, 5_000, q_cam[1]     # only junk matches: cnt 0 after the filter
    assert np.unique(g_pid, return_counts=True)[1].max() <= rcap
    pos, cnt = _abi_positions(d, q_pid, g_pid, q_cam, g_cam, rcap)
    pos_np, cnt_np = _np_positions(d, q_pid, g_pid, q_cam, g_cam, rcap)
    assert cnt_np[0] == 0 and cnt_np[1] == 0 and (cnt_np > 0).sum() == nq - 2
    assert np.array_equal(cnt, cnt_np) and np.array_equal(pos, pos_np)       # incl. the -1 padding of every row
    # the unfiltered entry point: unchanged results; and the camera-aware one agrees with it when nothing is junk
    pos_u, cnt_u = _abi_positions(d, q_pid, g_pid, None, None, rcap)
    pos_un, cnt_un = _np_positions(d, q_pid, g_pid, None, None, rcap)
    assert np.array_equal(cnt_u, cnt_un) and np.array_equal(pos_u, pos_un) and not np.array_equal(pos_u, pos)
    pos_c, cnt_c = _abi_positions(d, q_pid, g_pid, q_cam + 100, g_cam, rcap)
    assert np.array_equal(cnt_c, cnt_u) and np.array_equal(pos_c, pos_u)
    # more pid matches than rcap: the row is handed back (-1), relevant or junk alike
    pos_s, cnt_s = _abi_positions(d, q_pid, g_pid, q_cam, g_cam, 8)
    counts = (g_pid[None, :] == q_pid[:, None]).sum(1)
    assert np.array_equal(cnt_s < 0, counts > 8) and np.array_equal(cnt_s[counts <= 8], cnt_np[counts <= 8])
    assert np.array_equal(pos_s[counts <= 8], pos_np[counts <= 8, :8])


@pytest.mark.parametrize("rerank", [False, True])
def test_r1_map_eval_attribute(rerank):
    from mpreid import synth
    from utils.metrics import R1_mAP_eval, eval_func
    n, nq = 600, 100
    f, pid = synth.clustered_features(n, 64, 2.5, seed=31)
    cam = synth.labels_for(n)
    out = {}
    for on in (False, True):
        ev = R1_mAP_eval(nq, feat_norm=True, reranking=rerank)
        assert ev.remove_same_cam is False
        ev.remove_same_cam = on
        ev.reset()
        for s in range(0, n, 128):
            ev.update((torch.from_numpy(f[s:s + 128]).cuda(), tuple(int(p) for p in pid[s:s + 128]),
                       tuple(int(c) for c in cam[s:s + 128])))
        out[on] = ev.compute()
    cmc, mAP, distmat = out[True][:3]
    assert distmat.dtype == np.float32 and distmat.tobytes() == out[False][2].tobytes()
    cmc_h, map_h = eval_func(distmat, pid[:nq], pid[nq:], cam[:nq], cam[nq:], remove_same_cam=True)
    assert np.array_equal(cmc, cmc_h) and abs(mAP - map_h) < 1e-12
    cmc_u, map_u = eval_func(distmat, pid[:nq], pid[nq:], cam[:nq], cam[nq:])
    assert np.array_equal(out[False][0], cmc_u) and abs(out[False][1] - map_u) < 1e-12
    assert map_h != map_u                              # precondition: the attribute changes the answer here


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", [(643, 41, 64, True), (900, 150, 192, False)])
def test_evaluator_samecam_with_virtual_ranks(world, case):
    """rank 0's 7-tuple with the attribute on == the single-process one byte for byte (ragged shards: 41 queries, 602
    gallery rows over 2 and 3 ranks)"""
    from mpreid import distributed as D, synth
    from utils.metrics import R1_mAP_eval
    n, nq, d, rerank = case
    f, pid = synth.clustered_features(n, d, 2.5, seed=77 + n, per_id=6, normalize=False)
    cam = synth.labels_for(n)

    def evaluator():
        ev = R1_mAP_eval(nq, max_rank=50, feat_norm='yes', reranking=rerank)
        ev.remove_same_cam = True
        ev.reset()
        return ev
    ev = evaluator()
    ev.update((torch.from_numpy(f).cuda(), tuple(int(p) for p in pid), tuple(int(c) for c in cam)))
    want = ev.compute()
    ev.remove_same_cam = False
    assert float(ev.compute()[1]) != float(want[1])      # precondition: the filter matters on this input
    W = EmulatedWorld(world)

    def rank_fn(r):
        q_lo, q_hi = D.shard_range(nq, r, world)
        g_lo, g_hi = D.shard_range(n - nq, r, world)
        idx = list(range(q_lo, q_hi)) + list(range(nq + g_lo, nq + g_hi))
        ev = evaluator()
        for s in range(0, len(idx), 64):
            sel = idx[s:s + 64]
            ev.update((torch.from_numpy(f[sel]).cuda(), tuple(int(p) for p in pid[sel]), tuple(int(c) for c in cam[sel])))
        return ev.compute()

    res = W.run(rank_fn)
    cmc, mAP, distmat, pids, camids, qf, gf = res[0]
    assert np.array_equal(cmc, want[0]) and cmc.dtype == want[0].dtype and float(mAP) == float(want[1])
    assert distmat.dtype == np.float32 and np.array_equal(distmat, want[2])
    assert list(pids) == [int(p) for p in want[3]] and list(camids) == [int(c) for c in want[4]]
    assert np.array_equal(qf.numpy(), want[5].numpy()) and np.array_equal(gf.numpy(), want[6].numpy())
    for r in range(1, world):
        assert res[r][2] is None and np.array_equal(res[r][0], want[0]) and float(res[r][1]) == float(want[1])


def test_do_inference_with_the_config_key(caplog):
    from config import cfg_base
    from datasets.make_dataloader import make_dataloader
    from model.make_model import make_model
    from processor.processor import do_inference
    from utils.metrics import eval_func
    results = {}
    for on in (True, False):
        cfg = cfg_base.clone()
        cfg.defrost()
        cfg.merge_from_list(["DATASETS.SYNTH_QUERY", 24, "DATASETS.SYNTH_GALLERY", 72, "DATASETS.SYNTH_IDS", 6,
                             "TEST.IMS_PER_BATCH", 32, "TEST.REMOVE_SAME_CAM", str(on)])
        cfg.freeze()
        _, _, val_loader, num_query, num_classes, cam_num, view_num = make_dataloader(cfg)
        model = make_model(cfg, num_class=num_classes, camera_num=cam_num, view_num=view_num)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.test"):
            r1, r5 = do_inference(cfg, model, val_loader, num_query)
        ev = do_inference.last_evaluator
        assert ev.remove_same_cam is on
        note = [r for r in caplog.records if "same identity from the same camera are removed" in r.getMessage()]
        assert len(note) == (1 if on else 0), caplog.text
        _, _, distmat, pids, camids, _, _ = ev.compute()
        pids, camids = np.asarray(pids), np.asarray(camids)
        cmc_h, map_h = eval_func(distmat, pids[:num_query], pids[num_query:], camids[:num_query], camids[num_query:],
                                 remove_same_cam=on)
        assert float(r1) == float(cmc_h[0]) and float(r5) == float(cmc_h[4])
        results[on] = (cmc_h, map_h, distmat)
    assert results[True][2].tobytes() == results[False][2].tobytes()
    assert results[True][1] != results[False][1]       # precondition: the key changes the answer on this loader
