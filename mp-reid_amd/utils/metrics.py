"""Drop-in for the reference's ``utils/metrics.py``: distance matrices, CMC/mAP and the
``R1_mAP_eval`` accumulator, with the heavy steps on the MI355X (libmpreid_hip.so).

Signatures kept (reference utils/metrics.py): euclidean_distance(qf, gf) :7, cosine_similarity(qf, gf) :15,
eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50) :28 (+ remove_same_cam=False, below),
R1_mAP_eval(num_query, max_rank=50, feat_norm=True, reranking=False) with reset/update/compute :91-134.

Differences that are deliberate and invisible to callers:
  * update() keeps a device-resident copy of each feature batch instead of ``feat.cpu()``; the
    whole of compute(), including the ranking behind CMC/mAP (eval_func_device), runs on the GPU.
    ``eval_func`` itself (numpy in, numpy out) stays a host function with the reference's signature.
  * ties in eval_func's ranking are broken by ascending gallery index (the reference's
    np.argsort is unstable, so it has no defined order on ties).

Market-1501 protocol (opt-in, not in the reference's eval_func as shipped): the reference's docstring (:29-31) promises
that, for each query, the gallery images of the same identity from the same camera are discarded, and line :54 that does
it is commented out; its other evaluation tail (processor/processor_uniprompt_stage2.py:476-505) runs it.  By default the
camera ids are therefore accepted and unused, like upstream.  With ``remove_same_cam=True`` (eval_func, eval_func_device,
eval_func_sharded; ``R1_mAP_eval.remove_same_cam``; config key TEST.REMOVE_SAME_CAM) a gallery item j is JUNK for query
q when g_pids[j] == q_pids[q] and g_camids[j] == q_camids[q]: junk items leave the ranking, the other pid matches are
the relevant ones, a relevant item's position counts the kept items with a smaller (distance, gallery index) key, and
a query is valid iff a relevant item is left.  That is eval_func with its line :54 restored.  max_rank is clamped by the
gallery size before the filter (:36-38); a row that keeps fewer than max_rank items continues its CMC at 1 after its
first hit (the reference could not stack such ragged rows).

Multi-trial protocols (VehicleID's ten trials, reference test.py:46-63 + datasets/vehicleid.py:137-144; RegDB's trials and
MMMP's exp_setting pairs are of the same kind) evaluate several (query set, gallery set) pairs over ONE set of images.  The
reference re-encodes everything per trial; here the pool is encoded once and the trials are DATA: a split is a pair
(q_idx, g_idx) of integer arrays indexing the pool in update() order -- non-empty, in [0, N), g_idx without duplicates
(ValueError naming the split otherwise; a query that is also in its own gallery list is allowed).  eval_func_splits (host
definition), eval_func_splits_device (one ranking launch over the resident pool x pool matrix) and R1_mAP_eval_splits.

Ranked lists (not in the reference, which keeps np.argsort's result inside eval_func, :39): rank_lists (host definition:
the first k entries of a stable argsort of every row, junk removed with remove_same_cam=True), rank_lists_device (the same
on a resident matrix, mpreid_rank_topk) and ``R1_mAP_eval.rank_list_k`` / ``last_rank_lists`` (TEST.RANK_LIST_K).

Query expansion in feature space (not in the reference): every row of the stack query || gallery is replaced by the
similarity-weighted mean of its first k neighbours before distances are computed -- "average / alpha-weighted query
expansion" on the query rows, "database-side augmentation" on the gallery rows.  expand_features / qe_aggregate (host
definition of one round, numpy), expand_features_device (ops.expand_features: no N x N matrix) and ``R1_mAP_eval.qe_k`` /
``qe_alpha`` / ``qe_times`` (TEST.QE_K / QE_ALPHA / QE_TIMES; also on R1_mAP_eval_splits, where every split expands its own
query + gallery set and is therefore evaluated split by split).  Single-process.

Extra metrics (not in the reference): mINP and verification statistics over ALL query x gallery pairs.
  * mINP: for a valid query with R relevant items, the last of them at 0-based position p_last of the kept ranking,
    INP = R / (p_last + 1); mINP = np.mean over the valid queries in query order.  eval_metrics (host definition) /
    eval_metrics_device return it with the per-query AP, INP, first-hit position and validity mask.
  * Pairs: (i, j) with distmat[i, j] finite; with remove_same_cam the same-identity same-camera pairs are dropped; a kept
    pair is positive iff the pids are equal; P / Nn = number of kept positive / negative pairs.  Distances compare through
    the 32-bit key of mpreid.ops.dist_keys (ascending distance, -0 equal to +0).  pair_counts: tp[b] / fp[b] = positive /
    negative pairs with d <= t_b for ascending thresholds -- the ROC curve is (fp / Nn, tp / P), a histogram the difference
    of consecutive counts.  tpr_at_fpr: for an integer budget m, tau = the (m + 1)-th smallest negative distance, the
    operating point is "accept d < tau" (the most permissive threshold with at most m false positives; m >= Nn accepts
    everything, tau = +inf); a rate f means m = int(np.floor(np.float64(f) * Nn)).  pair_counts_device / tpr_at_fpr_device
    count on the resident matrix (mpreid_pair_bucket_counts); all counts are integers and equal the host's bit for bit.
  * ``R1_mAP_eval.extra_metrics`` / ``roc_fprs`` / ``pair_hist_bins`` / ``pair_hist_range`` -> ``last_metrics``
    (TEST.EXTRA_METRICS / ROC_FPRS / PAIR_HIST_BINS / PAIR_HIST_RANGE); R1_mAP_eval_splits keeps per-split mINP only.
"""
import numpy as np
import torch

from mpreid import ops as _ops
from utils.reranking import re_ranking, re_ranking_device


def _as_tensor(x):
    return torch.from_numpy(x) if isinstance(x, np.ndarray) else x


def euclidean_distance(qf, gf):
    """Squared Euclidean distance |q|^2 + |g|^2 - 2 q.g  ->  np.float32 [m, n]."""
    return _ops.euclidean_distance(_as_tensor(qf), _as_tensor(gf)).cpu().numpy()


def cosine_similarity(qf, gf):
    """arccos of the clipped cosine  ->  np.float32 [m, n]."""
    return _ops.cosine_similarity(_as_tensor(qf), _as_tensor(gf)).cpu().numpy()


def _need_camids(q_camids, g_camids):
    if q_camids is None or g_camids is None:
        raise ValueError("remove_same_cam=True needs q_camids and g_camids")


def _eval_func_samecam(distmat, q_pids, g_pids, q_camids, g_camids, max_rank):
    """eval_func under the Market-1501 protocol (module docstring): host, numpy, stable order."""
    q_camids = np.asarray(q_camids)
    g_camids = np.asarray(g_camids)
    num_q, num_g = distmat.shape
    order = np.argsort(distmat, axis=1, kind="stable")
    match = (g_pids[order] == q_pids[:, None])
    junk = match & (g_camids[order] == q_camids[:, None])
    hit = match & ~junk
    valid = hit.any(axis=1)
    num_valid_q = float(valid.sum())
    assert num_valid_q > 0, "Error: all query identities do not appear in gallery"
    hit, junk = hit[valid], junk[valid]
    kept_rank = np.cumsum(~junk, axis=1)               # 1-based rank among the kept items (at kept entries)
    running = np.cumsum(hit, axis=1)
    first = kept_rank[np.arange(hit.shape[0]), hit.argmax(axis=1)] - 1
    cmc_rows = (np.arange(max_rank)[None, :] >= first[:, None]).astype(np.float32)
    all_cmc = cmc_rows.sum(0) / num_valid_q
    prec_at_hit = (running / np.maximum(kept_rank, 1)) * hit     # (kept_rank is 0 only in front of the first kept item)
    all_AP = prec_at_hit.sum(axis=1) / hit.sum(axis=1)
    return all_cmc, np.mean(all_AP)


def eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50, remove_same_cam=False):
    """Market-1501 style CMC and mAP exactly as the reference computes them: gallery samples that
    share pid AND camera with the query are NOT removed (that filter is disabled upstream), so by default the
    camera ids are accepted and unused.  remove_same_cam=True removes them (module docstring).
    Host-side, vectorised over queries."""
    distmat = np.asarray(distmat)
    q_pids = np.asarray(q_pids)
    g_pids = np.asarray(g_pids)
    if remove_same_cam:
        _need_camids(q_camids, g_camids)
    num_q, num_g = distmat.shape
    if num_g < max_rank:
        max_rank = num_g
        print("Note: number of gallery samples is quite small, got {}".format(num_g))
    if remove_same_cam:
        return _eval_func_samecam(distmat, q_pids, g_pids, q_camids, g_camids, max_rank)
    order = np.argsort(distmat, axis=1, kind="stable")
    hit = (g_pids[order] == q_pids[:, None])
    valid = hit.any(axis=1)
    num_valid_q = float(valid.sum())
    assert num_valid_q > 0, "Error: all query identities do not appear in gallery"
    hit = hit[valid]
    running = np.cumsum(hit, axis=1)
    # CMC: 1 from the first correct match on
    cmc_rows = (running[:, :max_rank] > 0).astype(np.float32)
    all_cmc = cmc_rows.sum(0) / num_valid_q
    # AP = mean over relevant ranks k of (hits up to k) / k
    ranks = np.arange(1, num_g + 1) * 1.0
    prec_at_hit = (running / ranks) * hit
    all_AP = prec_at_hit.sum(axis=1) / hit.sum(axis=1)
    mAP = np.mean(all_AP)
    return all_cmc, mAP


_warned_host_ranking = False


def _finish_positions(pos, cnt, fetch_rows, q_pids, g_pids, max_rank, rcap, q_camids=None, g_camids=None, extra=None):
    """The host tail of the device ranking, shared by the single-split and the multi-split paths: from the kernel's
    positions (pos [rows, rcap] int64 padded with -1, cnt [rows] int64) to (cmc hit counts, AP of every valid row, number of
    valid rows) in float64.  Rows handed back with cnt < 0 (more relevant items than the kernel holds in LDS) are ranked
    here: ``fetch_rows(over)`` returns their distance rows [len(over), ng] as numpy, aligned with g_pids / g_camids.
    `extra`: a dict that also receives, for ALL rows, ``valid`` (bool), ``R`` (relevant items), ``first`` and ``last`` (0-based
    position of the first / last relevant item, -1 for a row without one) -- what mINP needs; the return value is unchanged."""
    num_q = pos.shape[0]
    cam = q_camids is not None
    over = np.nonzero(cnt < 0)[0]          # queries with more relevant items than the kernel handles: host ranking
    if over.size:
        global _warned_host_ranking
        if not _warned_host_ranking:
            _warned_host_ranking = True
            import logging
            logging.getLogger("transreid.test").warning(
                "eval_func: %d of %d queries have more than %d relevant gallery items; their rows are ranked on the host "
                "(np.argsort per row, same result)", over.size, num_q, rcap)
        pos = np.concatenate([pos, np.full((num_q, 0), -1, np.int64)], axis=1)
        rows = fetch_rows(over)
        wide = max(int((g_pids[None, :] == q_pids[over, None]).sum(1).max()), pos.shape[1])
        pos = np.pad(pos, ((0, 0), (0, wide - pos.shape[1])), constant_values=-1)
        for r, qi in enumerate(over):
            order = np.argsort(rows[r], kind="stable")
            match = g_pids[order] == q_pids[qi]
            if cam:   # the same filter as the kernel: positions among the kept items
                junk = match & (g_camids[order] == q_camids[qi])
                p = (np.cumsum(~junk) - 1)[match & ~junk]
            else:
                p = np.nonzero(match)[0]
            pos[qi, :] = -1
            pos[qi, :p.size] = p
            cnt[qi] = p.size
    valid = cnt > 0
    num_valid = int(valid.sum())
    if extra is not None:
        rows = np.arange(num_q)
        extra["valid"], extra["R"] = valid.copy(), np.where(valid, cnt, 0).astype(np.int64)
        extra["first"] = np.where(valid, pos[:, 0], -1).astype(np.int64) if pos.shape[1] else np.full(num_q, -1, np.int64)
        extra["last"] = np.where(valid, pos[rows, np.maximum(cnt, 1) - 1], -1).astype(np.int64) if pos.shape[1] \
            else np.full(num_q, -1, np.int64)
    if num_valid == 0:
        return np.zeros(max_rank, np.float32), np.zeros(0, np.float64), 0
    pos, cnt = pos[valid], cnt[valid]
    first = pos[:, 0]
    cmc_rows = (np.arange(max_rank)[None, :] >= first[:, None]).astype(np.float32)
    t = np.arange(1, pos.shape[1] + 1, dtype=np.float64)[None, :]
    terms = np.where(pos >= 0, t / np.maximum(pos + 1.0, 1.0), 0.0)
    return cmc_rows.sum(0), terms.sum(axis=1) / cnt, num_valid


def _eval_rows_device(dist, q_pids, g_pids, max_rank, after_launch=None, q_camids=None, g_camids=None, extra=None):
    """Ranking statistics of the query ROWS in `dist` (device tensor [rows, ng] fp32): (cmc hit counts [max_rank] float32
    summed over the valid rows, AP of every valid row in row order (float64), number of valid rows).  Sums of 0/1 values
    are exact in float32, so hit counts of row shards add up to the unsharded counts bit for bit.
    `after_launch()` is called once the ranking kernel is queued and before the host waits for it (compute() starts the
    matrix's D2H copy there, ordered BEHIND the kernel).
    With camera ids (both or neither) the rows are ranked under the Market-1501 protocol: same-identity same-camera gallery
    items are removed, a row is valid iff a relevant item is left (mpreid_eval_rank_positions_cam)."""
    import ctypes as C
    from mpreid import _lib
    dev = _lib.require_gpu()
    L = _lib.load()
    dist = dist.detach()
    assert dist.is_cuda and dist.dtype == torch.float32 and dist.dim() == 2 and (dist.stride(1) == 1 or dist.shape[0] == 0)
    num_q, num_g = dist.shape
    q_pids = np.ascontiguousarray(q_pids, dtype=np.int64)
    g_pids = np.ascontiguousarray(g_pids, dtype=np.int64)
    cam = q_camids is not None
    if cam:
        q_camids = np.ascontiguousarray(q_camids, dtype=np.int64)
        g_camids = np.ascontiguousarray(g_camids, dtype=np.int64)
        assert q_camids.shape == q_pids.shape and g_camids.shape == g_pids.shape
    if num_q == 0:
        if after_launch is not None:
            after_launch()
        if extra is not None:
            extra.update(valid=np.zeros(0, bool), R=np.zeros(0, np.int64), first=np.zeros(0, np.int64),
                         last=np.zeros(0, np.int64))
        return np.zeros(max_rank, np.float32), np.zeros(0, np.float64), 0
    rcap = _pid_rcap(g_pids)
    qp, gp = torch.from_numpy(q_pids).to(dev), torch.from_numpy(g_pids).to(dev)
    pos = torch.empty((num_q, rcap), dtype=torch.int32, device=dev)
    cnt = torch.empty(num_q, dtype=torch.int32, device=dev)
    if cam:   # rcap from the pid counts bounds the relevant AND the junk items: both live in the kernel's sorted list
        qc, gc = torch.from_numpy(q_camids).to(dev), torch.from_numpy(g_camids).to(dev)
        _lib.check(L.mpreid_eval_rank_positions_cam(C.c_void_p(dist.data_ptr()), dist.stride(0), num_q, num_g,
                                                    C.c_void_p(qp.data_ptr()), C.c_void_p(gp.data_ptr()),
                                                    C.c_void_p(qc.data_ptr()), C.c_void_p(gc.data_ptr()), rcap,
                                                    C.c_void_p(pos.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                    _lib.stream_ptr()), "mpreid_eval_rank_positions_cam")
    else:
        _lib.check(L.mpreid_eval_rank_positions(C.c_void_p(dist.data_ptr()), dist.stride(0), num_q, num_g,
                                                C.c_void_p(qp.data_ptr()), C.c_void_p(gp.data_ptr()), rcap,
                                                C.c_void_p(pos.data_ptr()), C.c_void_p(cnt.data_ptr()), _lib.stream_ptr()),
                   "mpreid_eval_rank_positions")
    if after_launch is not None:
        after_launch()
    pos, cnt = pos.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64)
    return _finish_positions(pos, cnt, lambda over: dist[torch.from_numpy(over).to(dev)].cpu().numpy(), q_pids, g_pids,
                             max_rank, rcap, q_camids, g_camids, extra)


def eval_func_device(dist, q_pids, g_pids, q_camids=None, g_camids=None, max_rank=50, after_launch=None,
                     remove_same_cam=False, extra=None):
    """eval_func with the ranking done on the GPU (dist: device tensor [nq, ng] fp32, left on the device).

    Per query the kernel returns the positions of the relevant gallery items in the ascending (distance, index)
    order of the row — what the reference reads off np.argsort — in one pass over the row; CMC and AP are
    finished here in float64.  CMC is identical to eval_func's; AP sums the same terms (hits up to k) / k in a
    different order than numpy's pairwise reduction over the dense row, i.e. |delta mAP| ~ 1e-16.

    remove_same_cam=True: the Market-1501 protocol (module docstring) through mpreid_eval_rank_positions_cam; without it
    the camera ids are unused and the call is what it was before the option existed.

    Under a process group (one rank per GPU) `dist` may be this rank's ROW block and q_pids its rows' pids: see
    eval_func_sharded.

    extra: a dict that also receives the per-query statistics of the SAME ranking launch (``valid``, ``R``, ``first``,
    ``last``: _finish_positions; ``all_AP``: the AP of the valid queries) -- eval_metrics_device builds mINP from them."""
    if remove_same_cam:
        _need_camids(q_camids, g_camids)
    num_g = dist.shape[1]
    if num_g < max_rank:
        max_rank = num_g
        print("Note: number of gallery samples is quite small, got {}".format(num_g))
    if remove_same_cam:
        hits, ap, num_valid = _eval_rows_device(dist, q_pids, g_pids, max_rank, after_launch, q_camids, g_camids, extra)
    else:
        hits, ap, num_valid = _eval_rows_device(dist, q_pids, g_pids, max_rank, after_launch, extra=extra)
    assert num_valid > 0, "Error: all query identities do not appear in gallery"
    if extra is not None:
        extra["all_AP"] = ap
    return hits / float(num_valid), np.mean(ap)


def eval_func_sharded(dist_rows, q_pids_local, g_pids, max_rank=50, q_camids_local=None, g_camids=None,
                      remove_same_cam=False):
    """eval_func over query rows sharded across the ranks of the default process group (SURVEY.md section 8e, row
    `eval_func`): every rank ranks its own rows [q_lo, q_hi) on its GPU; the hit counts (exact small integers) are
    summed and the per-query AP lists are concatenated in rank = query order, so every rank ends up with the cmc / mAP
    of the unsharded call BIT FOR BIT (integer sums; np.mean over the same float64 list in the same order).
    remove_same_cam=True (with this rank's rows' camera ids and all gallery camera ids): the Market-1501 protocol, row by
    row as in eval_func_device."""
    import torch.distributed  # noqa: F401  (ReduceOp)
    from mpreid import distributed as D
    if remove_same_cam:
        _need_camids(q_camids_local, g_camids)
    rank, world = D.rank_world()
    num_g = dist_rows.shape[1]
    if num_g < max_rank:
        max_rank = num_g
        if rank == 0:
            print("Note: number of gallery samples is quite small, got {}".format(num_g))
    if remove_same_cam:
        hits, ap, num_valid = _eval_rows_device(dist_rows, q_pids_local, g_pids, max_rank, None, q_camids_local, g_camids)
    else:
        hits, ap, num_valid = _eval_rows_device(dist_rows, q_pids_local, g_pids, max_rank)
    if D.sharded_active():
        staged = D._pg().get_backend() == "gloo"
        dev = "cpu" if staged else dist_rows.device
        # one small all-gather: [hit counts (max_rank) | number of valid rows | AP of the valid rows, NaN padded]
        cap = torch.tensor([ap.size], dtype=torch.int64, device=dev)
        D._pg().all_reduce(cap, op=torch.distributed.ReduceOp.MAX)
        cap = int(cap.item())
        msg = np.full(max_rank + 1 + cap, np.nan, np.float64)
        msg[:max_rank] = hits
        msg[max_rank] = num_valid
        msg[max_rank + 1: max_rank + 1 + ap.size] = ap
        parts = [torch.empty(msg.size, dtype=torch.float64, device=dev) for _ in range(world)]
        D._pg().all_gather(parts, torch.from_numpy(msg).to(dev))
        parts = [p.cpu().numpy() for p in parts]
        hits = np.sum([p[:max_rank] for p in parts], axis=0).astype(np.float32)   # exact: integers < 2^24
        num_valid = int(sum(p[max_rank] for p in parts))
        ap = np.concatenate([p[max_rank + 1: max_rank + 1 + int(p[max_rank])] for p in parts])
    assert num_valid > 0, "Error: all query identities do not appear in gallery"
    return hits / float(num_valid), np.mean(ap)


def _check_splits(splits, n):
    """the splits [(q_idx, g_idx), ...] as int64 arrays, validated against a pool of n items (module docstring)"""
    out = []
    if len(splits) == 0:
        raise ValueError("splits: no split given")
    for i, split in enumerate(splits):
        try:
            q, g = split
            q, g = np.asarray(q), np.asarray(g)
        except (TypeError, ValueError):
            raise ValueError(f"split {i}: not a (q_idx, g_idx) pair") from None
        for name, a in (("q_idx", q), ("g_idx", g)):
            if a.ndim != 1 or a.size == 0:
                raise ValueError(f"split {i}: {name} is empty (or not a 1-D list)")
            if a.dtype.kind not in "iu":
                raise ValueError(f"split {i}: {name} is not an integer array")
            if int(a.min()) < 0 or int(a.max()) >= n:
                raise ValueError(f"split {i}: {name} has an index outside [0, {n})")
        if np.unique(g).size != g.size:
            raise ValueError(f"split {i}: g_idx has duplicates")
        out.append((q.astype(np.int64), g.astype(np.int64)))
    return out


def eval_func_splits(distmat_pool, pids, camids, splits, max_rank=50, remove_same_cam=False):
    """CMC and mAP of several (query set, gallery set) pairs over ONE pool x pool distance matrix (multi-trial protocols:
    module docstring).  By definition eval_func on every split's sub-matrix:
    ``eval_func(distmat_pool[np.ix_(q, g)], pids[q], pids[g], camids[q], camids[g], max_rank, remove_same_cam)``.
    Returns (list of S float32 cmc arrays -- each min(max_rank, len(g)) long, eval_func's own rule -- , float64 mAP [S]).
    Host, numpy."""
    distmat_pool = np.asarray(distmat_pool)
    pids = np.asarray(pids)
    camids = None if camids is None else np.asarray(camids)
    if remove_same_cam and camids is None:
        raise ValueError("remove_same_cam=True needs camids")
    splits = _check_splits(splits, pids.shape[0])
    cmcs, maps = [], np.zeros(len(splits), np.float64)
    for i, (q, g) in enumerate(splits):
        cmc, maps[i] = eval_func(distmat_pool[np.ix_(q, g)], pids[q], pids[g], None if camids is None else camids[q],
                                 None if camids is None else camids[g], max_rank, remove_same_cam)
        cmcs.append(cmc)
    return cmcs, maps


def _pid_rcap(pids):
    return int(min(max(np.unique(pids, return_counts=True)[1].max(), 1), 8192))   # (the kernel's LDS limit, include/mpreid.h)


def eval_func_splits_device(dist_pool, pids, camids, splits, max_rank=50, remove_same_cam=False, extras=None):
    """eval_func_splits with the ranking on the GPU: `dist_pool` is the pool x pool matrix as a device fp32 tensor (unit
    column stride, rows through dist_pool.stride(0); left on the device).  ONE launch of mpreid_eval_rank_positions_splits
    ranks every (split, query) pair -- a pair reads its row of the matrix through its split's gallery index list, no
    sub-matrix is gathered -- and ONE D2H copy brings the positions back; per split, CMC / AP are then finished by the
    float64 tail eval_func_device uses (_finish_positions), so a split's numbers are those of eval_func_device on its
    sub-matrix.  Rows over the kernel's capacity are ranked on the host from the gathered row.
    extras: a list that receives one dict per split with the per-query statistics of _finish_positions plus ``all_AP``
    (host tail only: the positions are already here) -- R1_mAP_eval_splits derives the per-split mINP from them."""
    import ctypes as C
    from mpreid import _lib
    dev = _lib.require_gpu()
    L = _lib.load()
    dist = dist_pool.detach()
    assert dist.is_cuda and dist.dtype == torch.float32 and dist.dim() == 2 and dist.stride(1) == 1
    pids = np.ascontiguousarray(pids, dtype=np.int64)
    n = pids.shape[0]
    assert dist.shape[0] == n and dist.shape[1] == n, f"dist_pool is {tuple(dist.shape)} for a pool of {n}"
    cam = bool(remove_same_cam)
    if cam:
        if camids is None:
            raise ValueError("remove_same_cam=True needs camids")
        camids = np.ascontiguousarray(camids, dtype=np.int64)
        assert camids.shape == pids.shape
    splits = _check_splits(splits, n)
    S = len(splits)
    q_sizes = np.array([q.size for q, _ in splits], np.int64)
    g_off = np.zeros(S + 1, np.int64)
    g_off[1:] = np.cumsum([g.size for _, g in splits])
    q_off = np.zeros(S + 1, np.int64)
    q_off[1:] = np.cumsum(q_sizes)
    nqt = int(q_off[-1])
    assert nqt < 2 ** 31 and int(g_off[-1]) < 2 ** 40
    q_row = np.concatenate([q for q, _ in splits])
    g_idx = np.concatenate([g for _, g in splits])
    q_split = np.repeat(np.arange(S, dtype=np.int32), q_sizes)
    rcap = _pid_rcap(pids)                                    # bounds the pid matches of any row in any split
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    t_qrow, t_qsplit, t_gidx = up(q_row.astype(np.int32)), up(q_split), up(g_idx.astype(np.int32))
    t_qp, t_goff, t_gp = up(pids[q_row]), up(g_off), up(pids[g_idx])
    t_qc, t_gc = (up(camids[q_row]), up(camids[g_idx])) if cam else (None, None)
    out = torch.empty(nqt * (rcap + 1), dtype=torch.int32, device=dev)      # pos [nqt][rcap] | cnt [nqt]: one D2H copy
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    _lib.check(L.mpreid_eval_rank_positions_splits(
        ptr(dist), dist.stride(0), n, n, nqt, ptr(t_qrow), ptr(t_qsplit), ptr(t_qp), ptr(t_qc), S, ptr(t_goff),
        ptr(t_gidx), ptr(t_gp), ptr(t_gc), rcap, ptr(out), C.c_void_p(out.data_ptr() + 4 * nqt * rcap),
        _lib.stream_ptr()), "mpreid_eval_rank_positions_splits")
    host = out.cpu().numpy().astype(np.int64)
    pos_all, cnt_all = host[:nqt * rcap].reshape(nqt, rcap), host[nqt * rcap:]
    cmcs, maps = [], np.zeros(S, np.float64)
    for i, (q, g) in enumerate(splits):
        mr = max_rank
        if g.size < mr:
            mr = g.size
            print("Note: number of gallery samples is quite small, got {}".format(g.size))
        g_pids = pids[g]
        w = _pid_rcap(g_pids)           # the width the single-split call gives its rows: the same float64 sums, bit for bit
        lo, hi = int(q_off[i]), int(q_off[i + 1])
        g_t = t_gidx[int(g_off[i]):int(g_off[i + 1])].long()

        def fetch_rows(over, q=q, g_t=g_t):
            return dist[torch.from_numpy(q[over]).to(dev)].index_select(1, g_t).cpu().numpy()
        extra = None if extras is None else {}
        hits, ap, num_valid = _finish_positions(pos_all[lo:hi, :w].copy(), cnt_all[lo:hi].copy(), fetch_rows, pids[q],
                                                g_pids, mr, w, camids[q] if cam else None, camids[g] if cam else None, extra)
        assert num_valid > 0, f"split {i}: Error: all query identities do not appear in gallery"
        if extras is not None:
            extra["all_AP"] = ap
            extras.append(extra)
        cmcs.append(hits / float(num_valid))
        maps[i] = np.mean(ap)
    return cmcs, maps


def _rank_list_args(shape, k, q_pids, g_pids, q_camids, g_camids, remove_same_cam):
    """validated (k, labels or None) of rank_lists / rank_lists_device: ValueError before any device work"""
    k = _ops._check_topk_k(k)
    if len(shape) != 2:
        raise ValueError(f"distmat has shape {tuple(shape)}: a [nq, ng] matrix is expected")
    if not remove_same_cam:
        return k, None
    if any(a is None for a in (q_pids, g_pids, q_camids, g_camids)):
        raise ValueError("remove_same_cam=True needs q_pids, g_pids, q_camids and g_camids")
    return k, [np.asarray(a) for a in _ops._check_labels((q_pids, g_pids, q_camids, g_camids), shape[0], shape[1])]


def rank_lists(distmat, k, q_pids=None, g_pids=None, q_camids=None, g_camids=None, remove_same_cam=False):
    """Which gallery items come first for each query: the first k entries of ``np.argsort(distmat, axis=1)`` (reference
    utils/metrics.py:39) with ties broken by ascending gallery index (kind="stable"; -0 equals +0).  With
    remove_same_cam=True the gallery items with the query's pid AND the query's camera are junk and do not enter the list
    (module docstring).  Returns (indices int64 [nq, k], distances float32 [nq, k], counts int64 [nq]): counts =
    min(k, kept items), entries past it are -1 / +inf.  1 <= k <= 1024, as on the device.  Host, numpy: the definition."""
    distmat = np.asarray(distmat)
    k, labels = _rank_list_args(distmat.shape, k, q_pids, g_pids, q_camids, g_camids, remove_same_cam)
    nq, ng = distmat.shape
    idx = np.full((nq, k), -1, np.int64)
    val = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.int64)
    order = np.argsort(distmat, axis=1, kind="stable")
    for i in range(nq):
        o = order[i]
        if labels is not None:
            o = o[~((labels[1][o] == labels[0][i]) & (labels[3][o] == labels[2][i]))]
        o = o[:k]
        cnt[i] = o.size
        idx[i, :o.size] = o
        val[i, :o.size] = distmat[i, o]
    return idx, val, cnt


def rank_lists_device(dist, k, q_pids=None, g_pids=None, q_camids=None, g_camids=None, remove_same_cam=False):
    """rank_lists on a RESIDENT matrix (device tensor [nq, ng] fp32, left on the device) through ops.rank_topk: one
    launch, the lists alone come back to the host.  Same return value as rank_lists, byte for byte."""
    k, labels = _rank_list_args(tuple(dist.shape), k, q_pids, g_pids, q_camids, g_camids, remove_same_cam)
    idx, val, cnt = _ops.rank_topk(dist, k, 0, labels)
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)


def _qe_args(k, alpha, times=1):
    """validated (k, alpha, times) of query expansion: ValueError before any device work"""
    return _ops._check_topk_k(k), _ops._check_qe_alpha(alpha), _ops._check_qe_times(times)


def qe_aggregate(feats, idx, dist, cnt, alpha=3.0):
    """The aggregation of query expansion over given lists: row i of the result is the weighted mean of
    feats[idx[i, j]] over j < min(max(cnt[i], 0), k) IN LIST ORDER, every step rounded to float32 on its own --
    s = max(1 - 0.5 * dist[i, j], 0); w = 1 for alpha == 0 (also where s == 0), s multiplied alpha - 1 times left to right
    for an integer alpha 1 ... 8, s ** alpha (np.power, not bit-defined) otherwise; acc = acc + w * row; acc / float32(kk)
    at the end, zeros for an empty list.  Host, numpy: the definition mpreid_qe_aggregate_f32 is compared with bit for bit."""
    alpha = float(np.float32(_qe_args(1, alpha)[1]))      # (the ABI takes a float)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    idx, dist, cnt = np.asarray(idx), np.asarray(dist, dtype=np.float32), np.asarray(cnt)
    if feats.ndim != 2 or idx.ndim != 2 or dist.shape != idx.shape or cnt.shape != idx.shape[:1]:
        raise ValueError(f"feats {feats.shape}, idx {idx.shape}, dist {dist.shape}, cnt {cnt.shape}: [n, d], [rows, k], "
                         "[rows, k] and [rows] are expected")
    rows, k = idx.shape
    kk = np.clip(cnt.astype(np.int64), 0, k)
    one, half, zero = np.float32(1), np.float32(0.5), np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):      # (entries past cnt may hold anything)
        s = np.maximum(one - half * dist, zero)
        if alpha == 0:
            w = np.ones_like(s)
        elif alpha <= 8 and alpha == int(alpha):
            w = s
            for _ in range(int(alpha) - 1):
                w = w * s
        else:
            w = np.power(s, np.float32(alpha))
    acc = np.zeros((rows, feats.shape[1]), np.float32)
    for j in range(int(kk.max()) if rows else 0):
        live = np.nonzero(j < kk)[0]
        acc[live] = acc[live] + w[live, j][:, None] * feats[idx[live, j]]
    some = kk > 0
    acc[some] = acc[some] / kk[some].astype(np.float32)[:, None]
    return acc


def expand_features(feats, distmat, k, alpha=3.0):
    """One round of query expansion in feature space (not in the reference): every row of `feats` [N, D] -- the stack
    query || gallery in update() order, so this is AQE on the query rows and DBA on the gallery rows -- is replaced by the
    similarity-weighted mean of its first min(k, N) neighbours.  `distmat` [N, N] is euclidean_distance of the L2-NORMALISED
    rows against themselves (the way rank_lists takes a matrix): the lists are rank_lists(distmat, k) -- ascending
    (distance, index); the row itself is normally first, with its distance of +-1e-6 used as it is -- and the weights come
    from the listed distances (qe_aggregate), while the RAW rows are averaged.  Returns float32 [N, D], not normalised.
    Host, numpy: the definition ops.expand_features is compared with."""
    k, alpha, _ = _qe_args(k, alpha)
    feats, distmat = np.asarray(feats), np.asarray(distmat)
    if feats.ndim != 2 or feats.shape[1] < 1:
        raise ValueError(f"feats has shape {feats.shape}: an [N, D] matrix with D >= 1 is expected")
    if distmat.shape != (feats.shape[0], feats.shape[0]):
        raise ValueError(f"distmat has shape {distmat.shape} for {feats.shape[0]} rows: [N, N] is expected")
    idx, val, cnt = rank_lists(distmat, k)
    return qe_aggregate(feats, idx, val, cnt, alpha)


def expand_features_device(qf, gf, k, alpha=3.0, times=1, mode=_ops.GEMM_F32_EXACT, chunk=None):
    """`times` rounds of expand_features on the GPU without the N x N matrix (ops.expand_features: search_topk +
    mpreid_qe_aggregate_f32); returns (qf', gf') as float32 numpy arrays."""
    q, g = _ops.expand_features(_as_tensor(qf), _as_tensor(gf), k, alpha, times, mode, chunk)
    return q.cpu().numpy(), g.cpu().numpy()


DEFAULT_ROC_FPRS = (1e-4, 1e-3, 1e-2)


def _pair_classes(distmat, q_pids, g_pids, q_camids, g_camids, remove_same_cam):
    """(keys uint32 [nq, ng], positive mask, negative mask) of the kept pairs (module docstring, "Pairs")"""
    distmat = np.asarray(distmat, dtype=np.float32)
    if distmat.ndim != 2:
        raise ValueError(f"distmat has shape {distmat.shape}: a [nq, ng] matrix is expected")
    q_pids, g_pids = np.asarray(q_pids), np.asarray(g_pids)
    if q_pids.shape != (distmat.shape[0],) or g_pids.shape != (distmat.shape[1],):
        raise ValueError("q_pids / g_pids do not match the matrix")
    kept = np.isfinite(distmat)
    same = q_pids[:, None] == g_pids[None, :]
    if remove_same_cam:
        _need_camids(q_camids, g_camids)
        kept &= ~(same & (np.asarray(q_camids)[:, None] == np.asarray(g_camids)[None, :]))
    return _ops.dist_keys(distmat), kept & same, kept & ~same


def _threshold_keys(thresholds):
    t = np.asarray(thresholds, dtype=np.float32)
    if t.ndim != 1 or t.size < 1 or np.isnan(t).any():
        raise ValueError("thresholds: a non-empty 1-D list of numbers is expected")
    k = _ops.dist_keys(t)
    if k.size > 1 and not bool(np.all(k[1:] > k[:-1])):
        raise ValueError("thresholds must be strictly ascending (as float32, -0 equal to +0)")
    return k


def pair_counts(distmat, thresholds, q_pids, g_pids, q_camids=None, g_camids=None, remove_same_cam=False):
    """Verification counts over all query x gallery pairs (module docstring): for ascending thresholds t_0 < ... < t_{B-1}
    returns {"tp": int64 [B], "fp": int64 [B], "P": int, "Nn": int} with tp[b] / fp[b] = positive / negative pairs with
    d <= t_b (through the key order).  ROC: (fp / Nn, tp / P).  Host, numpy: the definition."""
    tk = _threshold_keys(thresholds)
    keys, pos, neg = _pair_classes(distmat, q_pids, g_pids, q_camids, g_camids, remove_same_cam)
    pk, nk = np.sort(keys[pos]), np.sort(keys[neg])
    return {"tp": np.searchsorted(pk, tk, side="right").astype(np.int64),
            "fp": np.searchsorted(nk, tk, side="right").astype(np.int64), "P": int(pk.size), "Nn": int(nk.size)}


def pair_histograms(counts):
    """(positive, negative) histograms int64 [B + 1] of a pair_counts result over its B thresholds taken as bin edges:
    entry 0 = underflow (d <= t_0), entry b = pairs with t_{b-1} < d <= t_b, entry B = overflow (d > t_{B-1}); they sum
    to P and Nn."""
    out = []
    for c, total in ((counts["tp"], counts["P"]), (counts["fp"], counts["Nn"])):
        out.append(np.diff(np.concatenate([[0], np.asarray(c, np.int64), [total]])).astype(np.int64))
    return out[0], out[1]


def _budgets(fprs, max_fp, Nn):
    """(budgets int64, fprs float64 or None): integer false-positive budgets from rates (floor(f * Nn)) or given directly"""
    if max_fp is not None:
        if fprs is not None:
            raise ValueError("give fprs or max_fp, not both")
        return _ops._check_budgets(np.atleast_1d(np.asarray(max_fp))), None
    fprs = np.atleast_1d(np.asarray(DEFAULT_ROC_FPRS if fprs is None else fprs, dtype=np.float64))
    if fprs.ndim != 1 or fprs.size < 1 or fprs.size > _ops.PAIR_SELECT_MAX or not bool(np.all((fprs >= 0) & (fprs <= 1))):
        raise ValueError(f"fprs: 1 ... {_ops.PAIR_SELECT_MAX} rates in [0, 1] are expected")
    return np.array([int(np.floor(np.float64(f) * Nn)) for f in fprs], np.int64), fprs


def _operating_points(budgets, fprs, tau, tp, fp, P, Nn):
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr = np.asarray(tp, np.float64) / np.float64(P) if P else np.full(len(tp), np.nan)
        fpr = np.asarray(fp, np.float64) / np.float64(Nn) if Nn else np.full(len(fp), np.nan)
    return {"budgets": np.asarray(budgets, np.int64), "fprs": fprs, "tau": np.asarray(tau, np.float32),
            "tp": np.asarray(tp, np.int64), "fp": np.asarray(fp, np.int64), "P": int(P), "Nn": int(Nn), "tpr": tpr,
            "fpr": fpr}


def tpr_at_fpr(distmat, q_pids, g_pids, q_camids=None, g_camids=None, remove_same_cam=False, fprs=None, max_fp=None):
    """TPR at a false-positive budget (module docstring): per budget m (``max_fp``: integers; or ``fprs``: rates, m =
    int(np.floor(np.float64(f) * Nn)); default rates 1e-4, 1e-3, 1e-2) tau = the (m + 1)-th smallest negative distance
    counted with multiplicity, tp / fp = positive / negative pairs with d < tau, everything accepted (tau = +inf) when
    m >= Nn.  Returns a dict: budgets, fprs (None with max_fp), tau (float32: the entry's bits, a zero as +0), tp, fp, P, Nn,
    tpr = tp / P (nan if P == 0), fpr = fp / Nn (the realised rate; nan if Nn == 0).  Host, numpy: the definition."""
    keys, pos, neg = _pair_classes(distmat, q_pids, g_pids, q_camids, g_camids, remove_same_cam)
    pk, nk = np.sort(keys[pos]), np.sort(keys[neg])
    P, Nn = int(pk.size), int(nk.size)
    budgets, fprs = _budgets(fprs, max_fp, Nn)
    tau = np.full(budgets.size, np.inf, np.float32)
    tp, fp = np.full(budgets.size, P, np.int64), np.full(budgets.size, Nn, np.int64)
    for i, m in enumerate(budgets.tolist()):
        if m < Nn:
            tk = nk[m]
            tau[i] = _ops.keys_to_dist(tk)
            tp[i] = np.searchsorted(pk, tk, side="left")
            fp[i] = np.searchsorted(nk, tk, side="left")
    return _operating_points(budgets, fprs, tau, tp, fp, P, Nn)


def _metrics_dict(cmc, mAP, all_AP, extra):
    valid = extra["valid"]
    inp = extra["R"][valid].astype(np.float64) / (extra["last"][valid].astype(np.float64) + 1.0)
    return {"cmc": cmc, "mAP": mAP, "mINP": np.mean(inp), "all_AP": all_AP, "all_INP": inp,
            "first_hit": extra["first"], "valid": valid}


def eval_metrics(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50, remove_same_cam=False):
    """eval_func plus mINP and the per-query statistics: {"cmc", "mAP": eval_func's own return values, to the bit;
    "mINP": np.mean of INP = R / (p_last + 1) over the valid queries in query order; "all_AP", "all_INP": float64 per VALID
    query; "first_hit": int64 [nq], 0-based position of the first relevant item in the kept ranking (-1: none); "valid":
    bool [nq]}.  all_AP sums a query's precision terms over its relevant items alone (the order eval_func_device uses), so
    np.mean(all_AP) may differ from eval_func's mAP -- a sum over the dense row -- in the last bit.  Host, numpy: the
    definition."""
    distmat = np.asarray(distmat)
    q_pids, g_pids = np.asarray(q_pids), np.asarray(g_pids)
    cmc, mAP = eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank, remove_same_cam)
    num_q, num_g = distmat.shape
    max_rank = min(max_rank, num_g)
    cam = bool(remove_same_cam)
    q_c, g_c = (np.asarray(q_camids), np.asarray(g_camids)) if cam else (None, None)
    rcap = _pid_rcap(g_pids)
    order = np.argsort(distmat, axis=1, kind="stable")
    pos = np.full((num_q, rcap), -1, np.int64)
    cnt = np.zeros(num_q, np.int64)
    for i in range(num_q):
        match = g_pids[order[i]] == q_pids[i]
        if int(match.sum()) > rcap:
            cnt[i] = -1                      # over the device kernel's capacity: the shared tail ranks the row itself
            continue
        if cam:
            junk = match & (g_c[order[i]] == q_c[i])
            p = (np.cumsum(~junk) - 1)[match & ~junk]
        else:
            p = np.nonzero(match)[0]
        pos[i, :p.size] = p
        cnt[i] = p.size
    extra = {}
    _, ap, _ = _finish_positions(pos, cnt, lambda over: distmat[over], q_pids, g_pids, max_rank, rcap, q_c, g_c, extra)
    return _metrics_dict(cmc, mAP, ap, extra)


def eval_metrics_device(dist, q_pids, g_pids, q_camids=None, g_camids=None, max_rank=50, remove_same_cam=False,
                        after_launch=None):
    """eval_metrics on a RESIDENT matrix: ONE ranking launch (eval_func_device's; rows over the kernel's capacity go through
    its host ranking), the same float64 tail, so cmc / mAP are eval_func_device's bits and mINP / all_AP / all_INP /
    first_hit / valid equal eval_metrics' on the same matrix."""
    extra = {}
    cmc, mAP = eval_func_device(dist, q_pids, g_pids, q_camids, g_camids, max_rank, after_launch, remove_same_cam, extra)
    return _metrics_dict(cmc, mAP, extra.pop("all_AP"), extra)


def _cam_args(q_camids, g_camids, remove_same_cam):
    if not remove_same_cam:
        return None, None
    _need_camids(q_camids, g_camids)
    return q_camids, g_camids


def pair_counts_device(dist, thresholds, q_pids, g_pids, q_camids=None, g_camids=None, remove_same_cam=False):
    """pair_counts on a RESIDENT matrix (device fp32 tensor [nq, ng], left on the device): one pass of
    mpreid_pair_bucket_counts, at most 4096 thresholds per call; the same dict, equal as integers."""
    tk = _threshold_keys(thresholds)
    qc, gc = _cam_args(q_camids, g_camids, remove_same_cam)
    c = _ops.pair_bucket_counts(dist, q_pids, g_pids, qc, gc, bound_keys=tk).cpu().numpy()
    return {"tp": np.cumsum(c[0])[:-1].astype(np.int64), "fp": np.cumsum(c[1])[:-1].astype(np.int64),
            "P": int(c[0].sum()), "Nn": int(c[1].sum())}


def tpr_at_fpr_device(dist, q_pids, g_pids, q_camids=None, g_camids=None, remove_same_cam=False, fprs=None, max_fp=None):
    """tpr_at_fpr on a RESIDENT matrix through ops.pair_select (exact radix selection over the keys; no sort of the
    nq * ng scores): the same dict, the counts equal as integers and tau as bytes."""
    qc, gc = _cam_args(q_camids, g_camids, remove_same_cam)
    if max_fp is not None:
        budgets, fprs = _budgets(fprs, max_fp, 0)
        r = _ops.pair_select(dist, q_pids, g_pids, qc, gc, budgets=budgets)
    else:
        _, fprs = _budgets(fprs, None, 0)
        r = _ops.pair_select(dist, q_pids, g_pids, qc, gc, fprs=fprs)
    return _operating_points(r["budgets"], fprs, r["tau"], r["tp"], r["fp"], r["P"], r["Nn"])


def _check_finite(feats, collective=False):
    """An encoder whose fp16 operand halves overflowed (|activation| > 65 504 in the 'split' / 'fp16' precision modes:
    include/mpreid.h, mpreid_vit_forward) hands over NaN / inf feature rows; ranking them would print a plausible-looking
    mAP.  Refuse loudly instead (one reduction over [N, D]; compute() synchronises anyway)."""
    import os
    if os.environ.get("MPREID_CHECK_FINITE", "1") == "0":   # opt-out: the reference's behaviour (it ranks whatever it is given)
        return
    bad = int((~torch.isfinite(feats).all(dim=1)).sum()) if feats.numel() else 0
    if collective:   # every rank must take the same branch: a rank that raised alone would leave the others in a collective
        from mpreid import distributed as D
        t = torch.tensor([bad], dtype=torch.int64, device="cpu" if D._pg().get_backend() == "gloo" else feats.device)
        D._pg().all_reduce(t)
        bad = int(t.item())
    if bad:
        raise RuntimeError(f"R1_mAP_eval.compute(): {bad} feature rows are non-finite -- the encoder's "
                           "fp16 operands overflowed (or the model produced NaN); use MODEL.ENCODER_PRECISION fp32 for "
                           "this checkpoint / input range (MPREID_CHECK_FINITE=0 restores the reference's behaviour: "
                           "no check, the rows are ranked as they are)")


_d2h_streams = {}


def _to_host_async(tensors):
    """Start the D2H copies of device tensors into fresh page-locked host tensors on a side stream (ordered after the
    current stream's work so far); returns (host tensors, event to synchronise before reading them).  The host tensors
    come from torch's caching pinned allocator: the caller owns them like any CPU tensor, and repeated evaluations reuse
    the pages.  (A pageable ``.cpu()`` of the 214 MB Market-1501 matrix is staged through a bounce buffer by the runtime and
    blocks the host for its whole duration; this way the copies run while the ranking kernel does.)"""
    dev = tensors[0].device
    side = _d2h_streams.get(dev)
    if side is None:
        side = _d2h_streams[dev] = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    hosts = []
    import os
    cap = int(os.environ.get("MPREID_PINNED_CAP_MB", "1024")) << 20
    with torch.cuda.stream(side):
        for t in tensors:
            # page-locked up to the cap (Market-1501's matrix is 214 MB); a multi-GB matrix (MSMT17: 3.8 GB) is not worth
            # that many locked pages for one copy: pageable memory, staged by the runtime
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=t.numel() * t.element_size() <= cap)
            h.copy_(t, non_blocking=True)
            t.record_stream(side)
            hosts.append(h)
        ev = torch.cuda.Event()
        ev.record(side)
    return hosts, ev


def _qe_setting(ev):
    """None when the evaluator's query expansion is off (qe_k == 0, or an evaluator made before the attribute existed), else
    the validated (k, alpha, times): ValueError before any device work"""
    k = int(getattr(ev, "qe_k", 0) or 0)
    if k == 0:
        return None
    return _qe_args(k, getattr(ev, "qe_alpha", 3.0), getattr(ev, "qe_times", 1))


def _hist_edges(bins, rng):
    """None for bins == 0, else the float32 edges [bins + 1] of the pair-distance histograms: ValueError before device work"""
    if int(bins) != bins or int(bins) < 0 or int(bins) + 1 > _ops.PAIR_BOUNDS_MAX:
        raise ValueError(f"pair_hist_bins = {bins}: an integer 0 ... {_ops.PAIR_BOUNDS_MAX - 1} is expected")
    if int(bins) == 0:
        return None
    lo, hi = (float(x) for x in rng)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"pair_hist_range = {tuple(rng)}: finite lo < hi is expected")
    edges = np.linspace(lo, hi, int(bins) + 1).astype(np.float32)
    _threshold_keys(edges)      # (too many bins for the range in float32: not strictly ascending)
    return edges


class R1_mAP_eval():
    def __init__(self, num_query, max_rank=50, feat_norm=True, reranking=False):
        super(R1_mAP_eval, self).__init__()
        self.num_query = num_query
        self.max_rank = max_rank
        self.feat_norm = feat_norm      # used as a truth value, like upstream ('yes' and 'no' both normalise)
        self.reranking = reranking
        self.distance_mode = _ops.GEMM_F32_EXACT   # _ops.GEMM_F16_SPLIT3 (<= 1e-6) / GEMM_F16_FAST (~1e-4): TEST.DISTANCE_MODE
        self.rerank_algo = _ops.RERANK_AUTO   # _ops.RERANK_SPARSE_SPLIT3: faster at large N, outputs within 1e-6
        self.remove_same_cam = False    # True: Market-1501 protocol (module docstring), TEST.REMOVE_SAME_CAM
        self.last_rerank_stats = None
        self.rank_list_k = 0            # > 0: compute() also keeps every query's first k gallery items (TEST.RANK_LIST_K)
        self.last_rank_lists = None     # (indices int64 [nq, k], distances float32 [nq, k], counts int64 [nq]) of rank_lists
        # qe_k > 0: query expansion (expand_features: AQE + DBA over query || gallery) with k neighbours, weight exponent
        # qe_alpha, qe_times rounds, before normalisation and ranking (TEST.QE_K / QE_ALPHA / QE_TIMES)
        self.qe_k, self.qe_alpha, self.qe_times = 0, 3.0, 1
        # extra_metrics: compute() also fills last_metrics -- the eval_metrics dict (mINP, per-query AP / INP / first hit)
        # from the SAME ranking launch, "tpr_at_fpr" (the tpr_at_fpr dict at roc_fprs) and, with pair_hist_bins > 0,
        # "pair_hist_edges" (float32 [bins + 1] over pair_hist_range) / "pair_hist_pos" / "pair_hist_neg" (int64 [bins + 2]:
        # underflow, the bins (e_{b-1}, e_b], overflow; pair_histograms) -- of the matrix behind `distmat`, while it is
        # resident (TEST.EXTRA_METRICS / ROC_FPRS / PAIR_HIST_BINS / PAIR_HIST_RANGE)
        self.extra_metrics = False
        self.roc_fprs = DEFAULT_ROC_FPRS
        self.pair_hist_bins = 0
        self.pair_hist_range = (0.0, 4.0)
        self.last_metrics = None

    def reset(self):
        self.feats = []
        self.pids = []
        self.camids = []

    def update(self, output):  # called once for each batch
        feat, pid, camid = output
        dev = _ops._lib.require_gpu()
        # own a device-resident fp32 copy: the caller may reuse its buffer
        self.feats.append(feat.detach().to(device=dev, dtype=torch.float32, copy=True))
        self.pids.extend(np.asarray(pid))
        self.camids.extend(np.asarray(camid))

    def compute(self):  # called after each epoch
        from mpreid import distributed as D
        list_k = int(getattr(self, "rank_list_k", 0) or 0)
        self.last_rank_lists = None
        if list_k:
            _ops._check_topk_k(list_k)
            if D.sharded_active():
                raise NotImplementedError("ranked lists are single-process")
        qe = _qe_setting(self)
        if qe and D.sharded_active():
            raise NotImplementedError("query expansion is single-process")
        extra_on = bool(getattr(self, "extra_metrics", False))
        self.last_metrics = None
        if extra_on:
            if D.sharded_active():
                raise NotImplementedError("extra metrics are single-process")
            hist_edges = _hist_edges(getattr(self, "pair_hist_bins", 0), getattr(self, "pair_hist_range", (0.0, 4.0)))
            roc_fprs = _budgets(getattr(self, "roc_fprs", None), None, 0)[1]
        if D.sharded_active():
            return self._compute_sharded()
        feats = torch.cat(self.feats, dim=0)
        _check_finite(feats)
        if qe:   # the RAW rows are expanded; what follows sees the expanded rows as if the encoder had produced them
            print('=> Query expansion: k = {}, alpha = {}, {} round(s)'.format(*qe))
            feats = _ops._expand_rows(feats, qe[0], qe[1], qe[2], self.distance_mode, None)
        if self.feat_norm:
            print("The test feature is normalized")
            feats = _ops.l2_normalize(feats)
        # the features go to the host only because compute() returns them: their D2H copy (98 MB at Market-1501 scale) starts
        # NOW, on a side stream, and runs beside the distance GEMM / the re-ranking (round 6; it used to queue behind them)
        (h_feats,), feats_copied = _to_host_async([feats])
        qf = feats[:self.num_query]
        gf = feats[self.num_query:]
        q_pids = np.asarray(self.pids[:self.num_query])
        q_camids = np.asarray(self.camids[:self.num_query])
        g_pids = np.asarray(self.pids[self.num_query:])
        g_camids = np.asarray(self.camids[self.num_query:])
        if self.reranking:
            print('=> Enter reranking')
            dist, self.last_rerank_stats = re_ranking_device(qf, gf, k1=50, k2=15, lambda_value=0.3,
                                                             algo=getattr(self, "rerank_algo", 0))
            # the evaluator is called once per run: do not keep the re-ranking workspace (GBs at MSMT17 scale)
            # pinned beside the encoder's for the rest of the process
            _ops.release_workspaces("rerank")
        else:
            print('=> Computing DistMat with euclidean_distance')
            dist = _ops.euclidean_distance(qf, gf, mode=self.distance_mode)
        # ranking statistics on the GPU while the matrix is still resident; the matrix's own D2H copy runs on the side stream
        # BESIDE the ranking kernel.  (Measured, tools/evalrank_bench.py at Market-1501 shape: the kernel takes 0.15 ms alone
        # and 0.20 ms beside the copy; queueing the copy BEHIND it makes compute() 0.8 ms slower.  The 5.4 ms average of
        # round 5's rocprofv3 trace was the profiler serialising the two queues -- the kernel's interval there includes the
        # blit kernels it waited for.  MPREID_EVAL_D2H=behind orders the copy after the kernel: used for kernel traces only.)
        import os
        box = {}
        same_cam = bool(getattr(self, "remove_same_cam", False))

        def start_copy():
            box["h"], box["ev"] = _to_host_async([dist])
        extra = {} if extra_on else None     # the per-query statistics of the ONE ranking launch below
        if os.environ.get("MPREID_EVAL_D2H") == "behind":
            cmc, mAP = eval_func_device(dist, q_pids, g_pids, q_camids, g_camids, after_launch=start_copy,
                                        remove_same_cam=same_cam, extra=extra)
        else:
            start_copy()
            cmc, mAP = eval_func_device(dist, q_pids, g_pids, q_camids, g_camids, remove_same_cam=same_cam, extra=extra)
        if extra_on:   # the pair statistics count over the same resident matrix
            m = _metrics_dict(cmc, mAP, extra.pop("all_AP"), extra)
            m["tpr_at_fpr"] = tpr_at_fpr_device(dist, q_pids, g_pids, q_camids, g_camids, same_cam, fprs=roc_fprs)
            if hist_edges is not None:
                c = pair_counts_device(dist, hist_edges, q_pids, g_pids, q_camids, g_camids, same_cam)
                m["pair_hist_edges"] = hist_edges
                m["pair_hist_pos"], m["pair_hist_neg"] = pair_histograms(c)
            self.last_metrics = m
        if list_k:   # the lists of the matrix behind `distmat` (Euclidean or re-ranked), while it is resident
            self.last_rank_lists = rank_lists_device(dist, list_k, q_pids, g_pids, q_camids, g_camids, same_cam)
        (h_dist,), copied = box["h"], box["ev"]
        feats_copied.synchronize()
        copied.synchronize()
        return cmc, mAP, h_dist.numpy(), self.pids, self.camids, h_feats[:self.num_query], h_feats[self.num_query:]

    def _compute_sharded(self):
        """compute() with one evaluator instance per rank of the default process group (one process per GPU; replaces the
        reference's nn.DataParallel branch, processor/processor.py:178-182; partition of SURVEY.md section 8e).

        Contract: `num_query` is the GLOBAL number of queries; rank r was update()d with ITS samples only, in global
        order -- queries shard_range(num_query, r, P) first, then gallery rows shard_range(num_gallery, r, P)
        (processor.do_inference shards the loader that way).  Steps: L2-normalise locally; ONE all-gather of the query
        features over xGMI; the rank's [nq, ng_local] column block of the distance matrix (its gallery shard) -- or, with
        re-ranking, the row-sharded phases of mpreid.distributed.re_ranking_sharded; ranking statistics on every rank's
        own query rows (eval_func_sharded); the blocks concatenated on the host of rank 0.  No floating-point reduction
        crosses ranks: rank 0 returns the 7-tuple of the single-process compute() byte for byte; the other ranks get the
        same cmc / mAP / pids / camids / qf, None for distmat and their own gallery shard for gf."""
        import torch.distributed  # noqa: F401  (ReduceOp)
        from mpreid import distributed as D
        rank, world = D.rank_world()
        dev = _ops._lib.require_gpu()
        nq = self.num_query
        q_lo, q_hi = D.shard_range(nq, rank, world)
        nql = q_hi - q_lo
        n_local = sum(f.shape[0] for f in self.feats)
        assert n_local >= nql, f"rank {rank}: {n_local} samples but {nql} of them must be its query shard"
        dim = torch.tensor([self.feats[0].shape[1] if self.feats else 0], dtype=torch.int64,
                           device="cpu" if D._pg().get_backend() == "gloo" else dev)
        D._pg().all_reduce(dim, op=torch.distributed.ReduceOp.MAX)
        feats = torch.cat(self.feats, dim=0) if self.feats else torch.empty((0, int(dim.item())), device=dev)
        _check_finite(feats, collective=True)
        if self.feat_norm:
            if rank == 0:
                print("The test feature is normalized")
            feats = _ops.l2_normalize(feats)
        meta = [None] * world     # labels (python ints): metadata, not the data path
        D._pg().all_gather_object(meta, ([int(p) for p in self.pids], [int(c) for c in self.camids], n_local - nql))
        ng_sizes = [m[2] for m in meta]
        ng = sum(ng_sizes)
        assert ng_sizes == D.shard_sizes(ng, world), (
            f"gallery shards {ng_sizes} are not shard_sizes({ng}, {world}): feed every rank its shard_range slice")
        q_sizes = D.shard_sizes(nq, world)
        pids = [p for m, k in zip(meta, q_sizes) for p in m[0][:k]] + [p for m, k in zip(meta, q_sizes) for p in m[0][k:]]
        camids = [c for m, k in zip(meta, q_sizes) for c in m[1][:k]] + [c for m, k in zip(meta, q_sizes) for c in m[1][k:]]
        q_pids, g_pids = np.asarray(pids[:nq]), np.asarray(pids[nq:])
        same_cam = bool(getattr(self, "remove_same_cam", False))
        cam_kw = dict(q_camids_local=np.asarray(camids[q_lo:q_hi]), g_camids=np.asarray(camids[nq:]),
                      remove_same_cam=True) if same_cam else {}
        qf_local, gf_local = feats[:nql].contiguous(), feats[nql:].contiguous()
        qf = D.all_gather_rows(qf_local, nq)            # the RCCL all-gather of the query features
        if self.reranking:
            if rank == 0:
                print('=> Enter reranking')
            gf = D.all_gather_rows(gf_local, ng)        # every rank needs all rows of the N x N problem's operands
            rows = D.re_ranking_sharded(qf, gf, 50, 15, 0.3, algo=getattr(self, "rerank_algo", 0))   # [nql, ng]
            _ops.release_workspaces("rerank")
            cmc, mAP = eval_func_sharded(rows, q_pids[q_lo:q_hi], g_pids, **cam_kw)
            distmat = D.gather_row_blocks_to_host(rows, dst=0)
            gf_out = gf
        else:
            if rank == 0:
                print('=> Computing DistMat with euclidean_distance')
            block = _ops.euclidean_distance(qf, gf_local, mode=self.distance_mode)     # [nq, ng_local]
            rows = D.column_to_row_blocks(block, nq, ng_sizes)                         # [nql, ng]
            cmc, mAP = eval_func_sharded(rows, q_pids[q_lo:q_hi], g_pids, **cam_kw)
            distmat = D.gather_column_blocks_to_host(block, dst=0)                     # host concatenation on rank 0
            gf_host = D.gather_row_blocks_to_host(gf_local, dst=0)
            gf_out = torch.from_numpy(gf_host) if rank == 0 else gf_local
        return cmc, mAP, distmat, pids, camids, qf.cpu(), gf_out.cpu()


def _pool_matrix_fits(n):
    """whether the pool x pool fp32 matrix (4 n^2 bytes) stays under a quarter of the device's memory (mpreid_device_info)"""
    import ctypes as C
    from mpreid import _lib
    hbm = C.c_size_t(0)
    _lib.check(_lib.load().mpreid_device_info(None, 0, None, C.byref(hbm)), "mpreid_device_info")
    return 4 * int(n) * int(n) <= int(hbm.value) // 4


class R1_mAP_eval_splits():
    """R1_mAP_eval for protocols that evaluate several (query set, gallery set) pairs over ONE set of images (VehicleID's
    trials, reference test.py:46-63): update() takes the pool once, `splits` is a list of (q_idx, g_idx) index lists into
    the pool in update() order.  compute() -> (cmc_list, mAP [S], pids, camids, feats_host).

    Without re-ranking the pool x pool distance matrix is computed ONCE, stays on the device (``last_dist``) and every
    split is ranked against it in one launch (eval_func_splits_device); an entry D[q, g] has the bits the single-split
    evaluator computes for the same two feature rows.  With re-ranking the matrix depends on the split (the k-reciprocal
    neighbourhoods are those of the split's own query + gallery set), and a pool whose matrix would exceed a quarter of
    the device's memory has no room for it: both go split by split through the single-split code (gather the features,
    re_ranking_device / euclidean_distance, eval_func_device).  Query expansion (qe_k > 0) depends on the split's own set in
    the same way and takes the split-by-split path too; the returned feats_host stay the pool's unexpanded rows.
    Single-process only."""

    def __init__(self, splits, max_rank=50, feat_norm=True, reranking=False):
        self.splits = splits
        self.max_rank = max_rank
        self.feat_norm = feat_norm
        self.reranking = reranking
        self.distance_mode = _ops.GEMM_F32_EXACT
        self.rerank_algo = _ops.RERANK_AUTO
        self.remove_same_cam = False
        self.last_rerank_stats = None
        self.last_dist = None          # the pooled device matrix of the last compute() (None on the split-by-split path)
        self.qe_k, self.qe_alpha, self.qe_times = 0, 3.0, 1   # query expansion, as in R1_mAP_eval
        # extra_metrics: compute() also fills last_metrics = {"mINP": float64 [S], "all_INP": list of S arrays} from the
        # positions it copies back anyway (host tail only; pair statistics are not built for splits)
        self.extra_metrics = False
        self.last_metrics = None

    def reset(self):
        self.feats = []
        self.pids = []
        self.camids = []
        self.last_dist = None

    def update(self, output):  # called once for each batch of the pool
        feat, pid, camid = output
        dev = _ops._lib.require_gpu()
        self.feats.append(feat.detach().to(device=dev, dtype=torch.float32, copy=True))
        self.pids.extend(np.asarray(pid))
        self.camids.extend(np.asarray(camid))

    def compute(self):
        from mpreid import distributed as D
        if D.sharded_active():
            raise NotImplementedError("multi-trial evaluation is single-process")
        qe = _qe_setting(self)
        extras = [] if getattr(self, "extra_metrics", False) else None
        self.last_metrics = None
        feats = torch.cat(self.feats, dim=0)
        _check_finite(feats)
        raw = feats
        if self.feat_norm:
            print("The test feature is normalized")
            feats = _ops.l2_normalize(feats)
        (h_feats,), feats_copied = _to_host_async([feats])
        pids, camids = np.asarray(self.pids), np.asarray(self.camids)
        n = feats.shape[0]
        splits = _check_splits(self.splits, n)
        same_cam = bool(self.remove_same_cam)
        self.last_dist = None
        if not qe and not self.reranking and _pool_matrix_fits(n):
            print('=> Computing the pool DistMat with euclidean_distance')
            dist = _ops.euclidean_distance(feats, feats, mode=self.distance_mode)
            cmcs, maps = eval_func_splits_device(dist, pids, camids, splits, self.max_rank, same_cam, extras)
            self.last_dist = dist
        else:
            dev = feats.device
            cmcs, maps = [], np.zeros(len(splits), np.float64)
            for i, (q, g) in enumerate(splits):
                if qe:   # the split's own query || gallery stack is expanded (raw rows), then normalised like the pool
                    stack = _ops._expand_rows(raw[torch.from_numpy(np.concatenate([q, g])).to(dev)], qe[0], qe[1], qe[2],
                                              self.distance_mode, None)
                    if self.feat_norm:
                        stack = _ops.l2_normalize(stack)
                    qf, gf = stack[:q.size], stack[q.size:]
                else:
                    qf = feats[torch.from_numpy(q).to(dev)]
                    gf = feats[torch.from_numpy(g).to(dev)]
                if self.reranking:
                    print('=> Enter reranking')
                    dist, self.last_rerank_stats = re_ranking_device(qf, gf, k1=50, k2=15, lambda_value=0.3,
                                                                     algo=self.rerank_algo)
                    _ops.release_workspaces("rerank")
                else:
                    dist = _ops.euclidean_distance(qf, gf, mode=self.distance_mode)
                extra = None if extras is None else {}
                try:
                    cmc, maps[i] = eval_func_device(dist, pids[q], pids[g], camids[q], camids[g], self.max_rank,
                                                    remove_same_cam=same_cam, extra=extra)
                except AssertionError as e:
                    raise AssertionError(f"split {i}: {e}") from None
                cmcs.append(cmc)
                if extras is not None:
                    extras.append(extra)
        if extras is not None:
            inps = [_metrics_dict(None, None, e["all_AP"], e)["all_INP"] for e in extras]
            self.last_metrics = {"mINP": np.array([np.mean(x) for x in inps], np.float64), "all_INP": inps}
        feats_copied.synchronize()
        return cmcs, maps, self.pids, self.camids, h_feats
