"""Tensor-level host API over the C ABI (torch is plumbing here: device memory + streams).

Everything in this module runs on the current HIP device through libmpreid_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import GEMM_F16_FAST, GEMM_F16_SPLIT3, GEMM_F32_EXACT  # noqa: F401  (re-exported)
from ._lib import RERANK_AUTO, RERANK_DENSE, RERANK_SPARSE, RERANK_SPARSE_SPLIT3, RERANK_WIDE  # noqa: F401

_ws_cache: Dict[tuple, torch.Tensor] = {}


def _workspace(tag: str, nbytes: int, device) -> torch.Tensor:
    """Grow-only cached byte buffer per (device, tag, current stream); the caller owns nothing.  The stream is part of
    the key: a workspace is scratch memory of ONE in-flight call, and calls issued on different streams may overlap on
    the device (processor.do_inference alternates its encoder calls over two streams)."""
    key = (str(device), tag, int(torch.cuda.current_stream(device).cuda_stream))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            del _ws_cache[key]
            del buf
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def release_workspaces(tag: Optional[str] = None):
    """drop the cached workspace buffers (all of them, or those of one tag on every device)"""
    if tag is None:
        _ws_cache.clear()
        return
    for key in [k for k in _ws_cache if k[1] == tag]:
        del _ws_cache[key]


def _dev_f32(t, device) -> torch.Tensor:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """utils/metrics.py:112-114 — F.normalize(feats, dim=1, p=2)."""
    dev = _lib.require_gpu()
    x = _dev_f32(x, dev)
    out = torch.empty_like(x)
    if x.shape[0]:
        _lib.check(_lib.load().mpreid_l2_normalize_f32(_ptr(x), x.shape[0], x.shape[1], eps, _ptr(out),
                                                       _lib.stream_ptr()), "mpreid_l2_normalize_f32")
    return out


def sqnorm(x: torch.Tensor) -> torch.Tensor:
    dev = _lib.require_gpu()
    x = _dev_f32(x, dev)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=dev)
    if x.shape[0]:
        _lib.check(_lib.load().mpreid_sqnorm_f32(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _lib.stream_ptr()),
                   "mpreid_sqnorm_f32")
    return out


def _distance(fn_name: str, q, g, mode: int, out: Optional[torch.Tensor], col_offset: int) -> torch.Tensor:
    dev = _lib.require_gpu()
    L = _lib.load()
    q, g = _dev_f32(q, dev), _dev_f32(g, dev)
    assert q.dim() == 2 and g.dim() == 2 and q.shape[1] == g.shape[1], (q.shape, g.shape)
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    if out is None:
        out = torch.empty((nq, ng), dtype=torch.float32, device=dev)
        col_offset = 0
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == nq
    ldo = out.shape[1]
    assert col_offset + ng <= ldo
    if nq == 0 or ng == 0:
        return out
    wsb = L.mpreid_distance_workspace_bytes(nq, ng, d, mode)
    ws = _workspace("distance", wsb, dev)
    optr = C.c_void_p(out.data_ptr() + 4 * col_offset)
    _lib.check(getattr(L, fn_name)(_ptr(q), _ptr(g), nq, ng, d, optr, ldo, mode, _ptr(ws), ws.numel(),
                                   _lib.stream_ptr()), fn_name)
    return out


def euclidean_distance(q, g, mode: int = GEMM_F32_EXACT, out: Optional[torch.Tensor] = None,
                       col_offset: int = 0) -> torch.Tensor:
    """utils/metrics.py:7-13 on the GPU; returns a device tensor [nq, ng] (squared L2)."""
    return _distance("mpreid_euclidean_distance_f32", q, g, mode, out, col_offset)


def cosine_similarity(q, g, mode: int = GEMM_F32_EXACT, out: Optional[torch.Tensor] = None,
                      col_offset: int = 0) -> torch.Tensor:
    """utils/metrics.py:15-25 on the GPU; returns a device tensor [nq, ng] (arccos of the cosine)."""
    return _distance("mpreid_cosine_similarity_f32", q, g, mode, out, col_offset)


RANK_TOPK_MAX = _lib.RANK_TOPK_MAX
_SEARCH_BUFFER_BYTES = 256 << 20   # search_topk's default [nq][chunk] distance buffer stays at or below this


def _check_topk_k(k) -> int:
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k}: a ranked list has at least one entry")
    if k > RANK_TOPK_MAX:
        raise ValueError(f"k = {k} exceeds the limit of {RANK_TOPK_MAX} entries per list (MPREID_RANK_TOPK_MAX)")
    return k


def _check_labels(labels, nq: int, ng: int):
    """labels = (q_pids, g_pids, q_camids, g_camids), all four or None -> four int64 numpy / torch arrays of [nq] / [ng]"""
    if labels is None or all(a is None for a in labels):
        return None
    if len(labels) != 4 or any(a is None for a in labels):
        raise ValueError("labels: q_pids, g_pids, q_camids and g_camids go together (all four, or none)")
    out = []
    for name, a, n in zip(("q_pids", "g_pids", "q_camids", "g_camids"), labels, (nq, ng, nq, ng)):
        if not torch.is_tensor(a):
            a = np.asarray(a)
        if tuple(a.shape) != (n,):
            raise ValueError(f"labels: {name} has shape {tuple(a.shape)}, expected ({n},)")
        out.append(a)
    return out


def _dev_i64(a, device) -> torch.Tensor:
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    return a.detach().to(device=device, dtype=torch.int64).contiguous()


def rank_topk(dist: torch.Tensor, k: int, col0: int = 0, labels=None, carry=None):
    """The ranked lists of a resident matrix block (mpreid_rank_topk, include/mpreid.h): dist fp32 [nq, ng] on the device,
    unit column stride, any row stride (a column slice of a wider matrix is fine); column j is global gallery index
    col0 + j.  Returns device tensors (idx int32 [nq, k], val fp32 [nq, k], cnt int32 [nq]): per row the first k items of
    np.argsort(row, kind="stable") with the matrix entries' own bits, padded with -1 / +inf past cnt.
    labels = (q_pids, g_pids, q_camids, g_camids), g_* aligned with the block's columns: same-identity same-camera gallery
    items are junk and leave the lists (Market-1501 protocol).  carry = (idx, val, cnt) of an earlier call over OTHER
    columns: merged with this block IN PLACE and returned."""
    k = _check_topk_k(k)
    if not torch.is_tensor(dist) or dist.dim() != 2:
        raise ValueError("dist: a 2-D fp32 device tensor is expected")
    nq, ng = int(dist.shape[0]), int(dist.shape[1])
    col0 = int(col0)
    if col0 < 0 or col0 + ng >= 2 ** 31:
        raise ValueError(f"col0 = {col0} with {ng} columns: global gallery indices must stay below 2^31")
    labels = _check_labels(labels, nq, ng)
    if carry is not None:
        if len(carry) != 3:
            raise ValueError("carry: the (idx, val, cnt) of an earlier call is expected")
        for name, t, shape, dt in zip(("idx", "val", "cnt"), carry, ((nq, k), (nq, k), (nq,)),
                                      (torch.int32, torch.float32, torch.int32)):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
                raise ValueError(f"carry: {name} must be a {dt} tensor of shape {shape}")
    dev = _lib.require_gpu()
    L = _lib.load()
    dist = dist.detach()
    assert dist.is_cuda and dist.dtype == torch.float32 and (dist.stride(1) == 1 or ng <= 1 or nq == 0), \
        "dist: fp32 on the device with unit column stride"
    if carry is not None:
        idx, val, cnt = carry
        assert all(t.is_cuda and t.is_contiguous() for t in carry)
    else:
        idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
        val = torch.empty((nq, k), dtype=torch.float32, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    lab = [None] * 4 if labels is None else [_dev_i64(a, dev) for a in labels]
    _lib.check(L.mpreid_rank_topk(_ptr(dist), max(int(dist.stride(0)), ng), nq, ng, col0, k, _ptr(lab[0]), _ptr(lab[1]),
                                  _ptr(lab[2]), _ptr(lab[3]), int(carry is not None), _ptr(idx), _ptr(val), _ptr(cnt),
                                  _lib.stream_ptr()), "mpreid_rank_topk")
    return idx, val, cnt


def search_topk(qf, gf, k: int, mode: int = GEMM_F32_EXACT, chunk: Optional[int] = None, q_pids=None, g_pids=None,
                q_camids=None, g_camids=None):
    """Ranked lists of euclidean_distance(qf, gf) WITHOUT the nq x ng matrix: the gallery goes through euclidean_distance
    in blocks of `chunk` rows of gf into one reused [nq, chunk] buffer, and every block is merged into the lists with
    rank_topk's carry.  chunk: any value >= 1 (smaller than k, not a divisor of ng: fine); default the largest that keeps
    the buffer at or below 256 MB.  The lists are those of a stable argsort of the concatenated blocks; with
    GEMM_F32_EXACT an entry does not depend on the blocking, so they are those of the unblocked matrix.  With all four
    label arrays the Market-1501 filter applies.  Returns device tensors (idx int32 [nq, k], val fp32 [nq, k], cnt int32 [nq])."""
    k = _check_topk_k(k)
    shp_q, shp_g = tuple(qf.shape), tuple(gf.shape)
    if len(shp_q) != 2 or len(shp_g) != 2 or shp_q[1] != shp_g[1]:
        raise ValueError(f"qf {shp_q} and gf {shp_g}: two matrices with the same number of columns are expected")
    nq, ng = int(shp_q[0]), int(shp_g[0])
    if ng >= 2 ** 31:
        raise ValueError("gallery indices must stay below 2^31")
    if chunk is None:
        chunk = max(_SEARCH_BUFFER_BYTES // (4 * max(nq, 1)), 1)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk}: at least one gallery row per block")
    labels = _check_labels((q_pids, g_pids, q_camids, g_camids), nq, ng)
    dev = _lib.require_gpu()
    qf, gf = _dev_f32(qf, dev), _dev_f32(gf, dev)
    if labels is not None:
        labels = [_dev_i64(a, dev) for a in labels]
    chunk = max(min(chunk, ng), 1)
    buf = torch.empty((nq, chunk), dtype=torch.float32, device=dev)
    out = None
    for c0 in range(0, max(ng, 1), chunk):
        c1 = min(c0 + chunk, ng)
        if c1 > c0:
            euclidean_distance(qf, gf[c0:c1], mode=mode, out=buf, col_offset=0)
        lab = None if labels is None else (labels[0], labels[1][c0:c1], labels[2], labels[3][c0:c1])
        out = rank_topk(buf[:, :c1 - c0], k, col0=c0, labels=lab, carry=out)
    return out


def _check_qe_alpha(alpha) -> float:
    alpha = float(alpha)
    if not np.isfinite(alpha) or alpha < 0:
        raise ValueError(f"alpha = {alpha}: the weight exponent of query expansion is a finite number >= 0")
    return alpha


def _check_qe_times(times) -> int:
    if int(times) != times or int(times) < 0:
        raise ValueError(f"times = {times}: the number of expansion rounds is an integer >= 0")
    return int(times)


def qe_aggregate(src: torch.Tensor, idx: torch.Tensor, dist: torch.Tensor, cnt: torch.Tensor, alpha: float,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The aggregation of query expansion (mpreid_qe_aggregate_f32, include/mpreid.h): src fp32 [n_src, d] on the device,
    unit column stride, any row stride; (idx int32 [rows, k], dist fp32 [rows, k], cnt int32 [rows]) as rank_topk /
    search_topk return them.  Row i of the result is the mean of w_j * src[idx[i, j]] over the first cnt[i] entries in list
    order, w_j = max(1 - dist[i, j] / 2, 0) ** alpha.  The CONTENTS of idx are not checked (they must index src).
    out: an fp32 device tensor [rows, d] that does not overlap src (default: a new one).  Returns it."""
    alpha = _check_qe_alpha(alpha)
    for name, t, dt in (("src", src, torch.float32), ("idx", idx, torch.int32), ("dist", dist, torch.float32),
                        ("cnt", cnt, torch.int32)):
        if not torch.is_tensor(t) or t.dtype != dt:
            raise ValueError(f"{name}: a {dt} tensor is expected")
    if src.dim() != 2 or idx.dim() != 2 or tuple(dist.shape) != tuple(idx.shape) or tuple(cnt.shape) != (idx.shape[0],):
        raise ValueError(f"src {tuple(src.shape)}, idx {tuple(idx.shape)}, dist {tuple(dist.shape)}, cnt {tuple(cnt.shape)}: "
                         "[n_src, d], [rows, k], [rows, k] and [rows] are expected")
    rows, k = int(idx.shape[0]), _check_topk_k(idx.shape[1])
    n_src, d = int(src.shape[0]), int(src.shape[1])
    if d < 1:
        raise ValueError("src has no columns")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (rows, d)):
        raise ValueError(f"out: an fp32 tensor of shape {(rows, d)} is expected")
    dev = _lib.require_gpu()
    src = src.detach()
    if out is None:
        out = torch.empty((rows, d), dtype=torch.float32, device=dev)
    assert all(t.is_cuda for t in (src, idx, dist, cnt, out)), "device tensors are expected"
    assert idx.is_contiguous() and dist.is_contiguous() and cnt.is_contiguous()
    assert (src.stride(1) == 1 or d == 1 or n_src == 0) and (out.stride(1) == 1 or d == 1 or rows == 0), "unit column stride"
    if rows:
        _lib.check(_lib.load().mpreid_qe_aggregate_f32(_ptr(src), n_src, d, max(int(src.stride(0)), d), _ptr(idx), _ptr(dist),
                                                       _ptr(cnt), rows, k, alpha, _ptr(out), max(int(out.stride(0)), d),
                                                       _lib.stream_ptr()), "mpreid_qe_aggregate_f32")
    return out


def _expand_rows(feats: torch.Tensor, k: int, alpha: float, times: int, mode: int, chunk: Optional[int]) -> torch.Tensor:
    """`times` rounds of query expansion over the device stack feats [N, D] (arguments already validated): per round
    l2_normalize -> search_topk of the normalised rows against themselves -> qe_aggregate over the RAW rows, ping-pong
    between two buffers (`feats` is only read).  Returns a tensor that is never `feats` itself."""
    if times == 0 or feats.shape[0] == 0:
        return feats.clone()
    cur, bufs = feats, [None, None]
    for r in range(times):
        unit = l2_normalize(cur)
        idx, val, cnt = search_topk(unit, unit, k, mode=mode, chunk=chunk)
        del unit
        if bufs[r % 2] is None:
            bufs[r % 2] = torch.empty_like(feats)
        cur = qe_aggregate(cur, idx, val, cnt, alpha, out=bufs[r % 2])
    return cur


def expand_features(qf, gf, k: int, alpha: float = 3.0, times: int = 1, mode: int = GEMM_F32_EXACT,
                    chunk: Optional[int] = None):
    """Query expansion in feature space over the stack F = qf || gf (AQE on the query rows, DBA on the gallery rows): every
    row becomes the similarity-weighted mean of its first k neighbours -- utils/metrics.py:expand_features is the host
    definition of one round.  Per round: F^ = l2_normalize(F); the first min(k, N) neighbours of every row by exact
    (distance, index) order from search_topk(F^, F^) -- no N x N matrix, for any N search_topk takes; `mode` / `chunk` are
    search_topk's --; weights max(1 - d / 2, 0) ** alpha; the RAW rows are averaged (qe_aggregate).  `times` rounds repeat
    that with F <- F' (0: copies).  Returns (qf', gf') as device tensors, not normalised."""
    k = _check_topk_k(k)
    alpha = _check_qe_alpha(alpha)
    times = _check_qe_times(times)
    shp_q, shp_g = tuple(qf.shape), tuple(gf.shape)
    if len(shp_q) != 2 or len(shp_g) != 2 or shp_q[1] != shp_g[1] or shp_q[1] < 1:
        raise ValueError(f"qf {shp_q} and gf {shp_g}: two matrices with the same number (>= 1) of columns are expected")
    if shp_q[0] + shp_g[0] >= 2 ** 31:
        raise ValueError("row indices must stay below 2^31")
    dev = _lib.require_gpu()
    feats = torch.cat([_dev_f32(qf, dev), _dev_f32(gf, dev)], dim=0)
    out = _expand_rows(feats, k, alpha, times, mode, chunk)
    return out[:shp_q[0]], out[shp_q[0]:]


PAIR_BOUNDS_MAX = _lib.PAIR_BOUNDS_MAX
PAIR_SELECT_MAX = 16   # budgets per pair_select call


def dist_keys(d) -> np.ndarray:
    """The 32-bit ranking key of float32 distances (include/mpreid.h, verification statistics): ascending as unsigned
    integers = ascending distance, -0 equal to +0.  numpy in, uint32 out, same shape."""
    d = np.asarray(d, dtype=np.float32)
    u = np.ascontiguousarray(np.atleast_1d(d) + np.float32(0)).view(np.uint32)      # -0 + 0 = +0
    top = np.uint32(0x80000000)
    return np.where(u & top, ~u, u | top).astype(np.uint32).reshape(d.shape)


def keys_to_dist(k) -> np.ndarray:
    """the inverse of dist_keys (a zero comes back as +0)"""
    k = np.asarray(k, dtype=np.uint32)
    top = np.uint32(0x80000000)
    kk = np.atleast_1d(k)
    u = np.ascontiguousarray(np.where(kk & top, kk ^ top, ~kk).astype(np.uint32))
    return u.view(np.float32).reshape(k.shape)


def _check_bound_keys(bound_keys) -> np.ndarray:
    b = np.asarray(bound_keys)
    if b.ndim != 1 or b.dtype.kind not in "iu":
        raise ValueError("bound_keys: a 1-D array of uint32 keys (dist_keys of the thresholds) is expected")
    if b.size < 1 or b.size > PAIR_BOUNDS_MAX:
        raise ValueError(f"bound_keys: {b.size} bounds; 1 ... {PAIR_BOUNDS_MAX} are supported (MPREID_PAIR_BOUNDS_MAX)")
    if int(b.min()) < 0 or int(b.max()) > 0xFFFFFFFF:
        raise ValueError("bound_keys: keys are 32-bit unsigned integers")
    b = b.astype(np.uint32)
    if b.size > 1 and not bool(np.all(b[1:] > b[:-1])):
        raise ValueError("bound_keys must be strictly ascending")
    return np.ascontiguousarray(b)


def _pair_labels(nq, ng, q_pids, g_pids, q_camids, g_camids, dev):
    """device int64 labels of the pair statistics: (qp, gp, qc, gc), the camera ids both given or both None"""
    if (q_camids is None) != (g_camids is None):
        raise ValueError("q_camids and g_camids go together (both, or neither)")
    out = []
    for name, a, n in (("q_pids", q_pids, nq), ("g_pids", g_pids, ng), ("q_camids", q_camids, nq), ("g_camids", g_camids, ng)):
        if a is None:
            out.append(None)
            continue
        if tuple(a.shape if torch.is_tensor(a) else np.shape(a)) != (n,):
            raise ValueError(f"{name}: expected shape ({n},)")
        out.append(_dev_i64(a, dev))
    return out


def pair_bucket_counts(dist: torch.Tensor, q_pids, g_pids, q_camids=None, g_camids=None, bound_keys=None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How many positive / negative pairs of a resident matrix fall between consecutive bounds (mpreid_pair_bucket_counts,
    include/mpreid.h): dist fp32 [nq, ng] on the device, unit column stride, any row stride and alignment; bound_keys =
    dist_keys(thresholds), strictly ascending, at most 4096.  Returns an int64 device tensor [2, B + 1] (positive row,
    negative row): bucket b counts the kept pairs with bound[b-1] < key <= bound[b].  With both camera id arrays the
    same-identity same-camera pairs are dropped.  out: a tensor of an earlier call with the same bounds -- the counts are
    ADDED to it (column blocks of a matrix that is never held whole).  No host synchronisation."""
    if bound_keys is None:
        raise ValueError("bound_keys is required")
    bk = _check_bound_keys(bound_keys)
    if not torch.is_tensor(dist) or dist.dim() != 2:
        raise ValueError("dist: a 2-D fp32 device tensor is expected")
    nq, ng = int(dist.shape[0]), int(dist.shape[1])
    dev = _lib.require_gpu()
    dist = dist.detach()
    assert dist.is_cuda and dist.dtype == torch.float32 and (dist.stride(1) == 1 or ng <= 1 or nq == 0), \
        "dist: fp32 on the device with unit column stride"
    lab = _pair_labels(nq, ng, q_pids, g_pids, q_camids, g_camids, dev)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != (2, bk.size + 1) or \
                not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out: a contiguous int64 device tensor of shape {(2, bk.size + 1)} is expected")
    counts = out if out is not None else torch.empty((2, bk.size + 1), dtype=torch.int64, device=dev)
    bounds = torch.from_numpy(bk.view(np.int32)).to(dev)
    _lib.check(_lib.load().mpreid_pair_bucket_counts(_ptr(dist), max(int(dist.stride(0)), ng), nq, ng, _ptr(lab[0]),
                                                     _ptr(lab[1]), _ptr(lab[2]), _ptr(lab[3]), _ptr(bounds), int(bk.size),
                                                     int(out is not None), _ptr(counts), _lib.stream_ptr()),
               "mpreid_pair_bucket_counts")
    return counts


def _check_budgets(budgets) -> np.ndarray:
    b = np.asarray(budgets)
    if b.ndim != 1 or b.size < 1 or b.size > PAIR_SELECT_MAX or b.dtype.kind not in "iu":
        raise ValueError(f"budgets: 1 ... {PAIR_SELECT_MAX} integers are expected")
    if int(b.min()) < 0:
        raise ValueError("budgets: a false-positive budget is >= 0")
    return b.astype(np.int64)


def pair_select(dist: torch.Tensor, q_pids, g_pids, q_camids=None, g_camids=None, budgets=None, fprs=None):
    """The exact operating points "at most m false positives" of a resident matrix (definition: include/mpreid.h and
    utils/metrics.py:tpr_at_fpr): for every integer budget m, tau = the (m + 1)-th smallest negative distance, tp / fp =
    the positive / negative pairs with d < tau; m >= Nn accepts everything (tau = +inf).
    Radix refinement over the 32-bit key, digits of 12 | 12 | 8 bits, through pair_bucket_counts: one pass counts the
    first digit of every pair; per DISTINCT selected first digit one pass counts the second digit inside it, per distinct
    (first, second) prefix one pass counts the third -- 1 + n1 + n2 <= 1 + 2 * len(budgets) passes over the matrix, 3 when
    all budgets share their prefixes.  The small count arrays come back to the host between the rounds (this loop is
    Python; the ABI entry stays free of synchronisation); the positive counts below the selected bucket are summed on the
    way, so tp needs no pass of its own.
    budgets: up to 16 integers m >= 0; or fprs: up to 16 rates f in [0, 1], m = int(np.floor(np.float64(f) * Nn)) once the
    first pass has counted Nn.
    Returns a dict of numpy arrays / ints: budgets int64 [n], tau float32 [n], tp int64 [n], fp int64 [n], P, Nn."""
    if (budgets is None) == (fprs is None):
        raise ValueError("give budgets or fprs (one of them)")
    if budgets is not None:
        budgets = _check_budgets(budgets)
    else:
        fprs = np.atleast_1d(np.asarray(fprs, dtype=np.float64))
        if fprs.ndim != 1 or fprs.size < 1 or fprs.size > PAIR_SELECT_MAX or not bool(np.all((fprs >= 0) & (fprs <= 1))):
            raise ValueError(f"fprs: 1 ... {PAIR_SELECT_MAX} rates in [0, 1] are expected")
    args = (dist, q_pids, g_pids, q_camids, g_camids)
    full = np.uint64(0xFFFFFFFF)

    def digit_counts(prefix, shift, bits, known):
        """counts [2][2^bits] of the digit `bits` wide at `shift` among the pairs whose key has `prefix` above it; `known`
        [2] = the pairs under the prefix (None for the first digit): the last digit's count is what is left of it"""
        n = 1 << bits
        top = (np.arange(n - 1, dtype=np.uint64) << np.uint64(shift)) | ((np.uint64(1) << np.uint64(shift)) - np.uint64(1))
        keys = (np.uint64(prefix) | top) & full
        lead = prefix > 0
        if lead:                                    # bucket 0: everything below the prefix
            keys = np.concatenate([[np.uint64(prefix - 1)], keys])
        c = pair_bucket_counts(*args, bound_keys=keys.astype(np.uint32)).cpu().numpy()
        c = c[:, 1:] if lead else c                 # [2][n]: digits 0 ... n-2, then digit n-1 together with what lies above
        if known is not None:
            c = c.copy()
            c[:, n - 1] = known - c[:, :n - 1].sum(axis=1)
        return c

    c1 = digit_counts(0, 20, 12, None)
    P, Nn = int(c1[0].sum()), int(c1[1].sum())
    if budgets is None:
        budgets = np.array([int(np.floor(np.float64(f) * Nn)) for f in fprs], np.int64)
    n = budgets.size
    tau = np.full(n, np.inf, np.float32)
    tp = np.full(n, P, np.int64)
    fp = np.full(n, Nn, np.int64)
    cache = {}
    for i, m in enumerate(budgets.tolist()):
        if m >= Nn:
            continue
        prefix, rem, tpa, fpa, c, known = 0, m, 0, 0, c1, None
        for shift, bits in ((20, 12), (8, 12), (0, 8)):
            if c is None:
                if (prefix, shift) not in cache:
                    cache[(prefix, shift)] = digit_counts(prefix, shift, bits, known)
                c = cache[(prefix, shift)]
            cum = np.cumsum(c[1])
            d = int(np.searchsorted(cum, rem, side="right"))      # first digit with more than rem negatives up to it
            below = int(cum[d - 1]) if d else 0
            tpa += int(c[0][:d].sum())
            fpa += below
            rem -= below
            known = c[:, d].copy()
            prefix |= d << shift
            c = None
        tau[i] = keys_to_dist(np.uint32(prefix))
        tp[i], fp[i] = tpa, fpa
    return {"budgets": budgets, "tau": tau, "tp": tp, "fp": fp, "P": P, "Nn": Nn}


def re_ranking(q, g, k1: int, k2: int, lambda_value: float, local_distmat=None, only_local: bool = False,
               timing: bool = False, debug: bool = False, algo: int = _lib.RERANK_AUTO, ws_tag: str = "rerank"):
    """utils/reranking.py:29-100 on the GPU.  Returns (device tensor [nq, ng] fp32, stats dict)
    and, with debug=True, additionally (initial_rank[:, :k1+1], nnz(V) per row, nnz(V_qe) per row).
    algo: RERANK_AUTO (the candidate pipeline without the N x N matrix when it applies, else the dense one; a sparse
    call that hits a data-dependent capacity is repeated densely), RERANK_DENSE, RERANK_SPARSE -- same bits;
    RERANK_SPARSE_SPLIT3: the sparse algorithm with the blend term's distance rows from the fp16 matrix cores (3-term
    split): neighbour table / V / V_qe / Jaccard term bit-identical, |final - exact| <= lambda * 1e-6 / max.
    RERANK_WIDE: the dense arithmetic for any k1 / k2 (AUTO / DENSE / SPARSE refuse max(k1 + 1, k2) > 256 and expansion
    lists beyond a workgroup's LDS, include/mpreid.h "Limits"; ``rerank_fits`` tells beforehand) -- same bits, slower; never
    chosen by AUTO here (utils.reranking, the reference-signature layer, switches to it by itself).
    ws_tag: name of the cached workspace; calls that run CONCURRENTLY on different streams need different tags (the C
    entry point is re-entrant per stream with caller-owned workspaces)."""
    dev = _lib.require_gpu()
    L = _lib.load()
    q, g = _dev_f32(q, dev), _dev_f32(g, dev)
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    N = nq + ng
    loc = None
    if local_distmat is not None:
        loc = _dev_f32(local_distmat, dev)
        assert tuple(loc.shape) == (N, N)
    out = torch.empty((nq, ng), dtype=torch.float32, device=dev)
    st = _lib.RerankStats()
    for attempt in (algo, _lib.RERANK_DENSE):
        wsb = L.mpreid_rerank_workspace_bytes_ex(nq, ng, d, int(k1), int(k2), int(loc is not None), int(attempt))
        ws = _workspace(ws_tag, wsb, dev)
        rc = L.mpreid_rerank_f32_ex(_ptr(q), _ptr(g), nq, ng, d, int(k1), int(k2), float(lambda_value), _ptr(loc),
                                    int(bool(only_local)), _ptr(out), ng, _ptr(ws), ws.numel(), _lib.stream_ptr(),
                                    C.byref(st), int(bool(timing)), int(attempt))
        if rc == _lib.ERR_RETRY_DENSE and attempt != _lib.RERANK_DENSE and algo == _lib.RERANK_AUTO:
            continue
        _lib.check(rc, "mpreid_rerank_f32_ex")
        break
    stats = st.as_dict()
    if not debug:
        return out, stats
    rank = np.empty((N, k1 + 1), np.int32)
    vc = np.empty(N, np.int32)
    vq = np.empty(N, np.int32)
    _lib.check(L.mpreid_rerank_debug_copy_ex(_ptr(ws), nq, ng, d, int(k1), int(k2), int(loc is not None),
                                             C.c_void_p(rank.ctypes.data), C.c_void_p(vc.ctypes.data),
                                             C.c_void_p(vq.ctypes.data), _lib.stream_ptr(), int(stats["algo"])),
               "mpreid_rerank_debug_copy_ex")
    return out, stats, rank, vc, vq


def rerank_fits(nq: int, ng: int, d: int, k1: int, k2: int, has_local: bool = False, algo: int = _lib.RERANK_AUTO) -> bool:
    """True when ``algo`` accepts the problem, False when re_ranking would refuse it for one of the documented limits
    (mpreid_rerank_fits: no GPU needed, no side effects)."""
    return bool(_lib.load().mpreid_rerank_fits(int(nq), int(ng), int(d), int(k1), int(k2), int(bool(has_local)), int(algo)))


def gemm_f16_nt(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """C[M,N] fp32 = A[M,K] fp16 x B[N,K]^T fp16 (M, N multiples of 128, K of 64)."""
    dev = _lib.require_gpu()
    assert a.dtype == torch.float16 and b.dtype == torch.float16 and a.is_contiguous() and b.is_contiguous()
    m, k = a.shape
    n = b.shape[0]
    c = torch.empty((m, n), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mpreid_gemm_f16_nt(_ptr(a), _ptr(b), _ptr(c), m, n, k, _lib.stream_ptr()),
               "mpreid_gemm_f16_nt")
    return c


VIEW_ORIGINAL, VIEW_FLIP, VIEW_PSEUDO_IR, VIEW_PSEUDO_RGB = 0, 1, 2, 3


def tta_mean(feats: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """feats [n_views, rows, dim] fp32 -> [rows, dim]: torch.stack(feat_list).mean(0) (+ F.normalize)."""
    dev = _lib.require_gpu()
    f = _dev_f32(feats, dev)
    assert f.dim() == 3
    out = torch.empty(f.shape[1:], dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mpreid_tta_mean_f32(_ptr(f), f.shape[0], f.shape[1], f.shape[2], int(bool(normalize)), _ptr(out),
                                               _lib.stream_ptr()), "mpreid_tta_mean_f32")
    return out


class _HostStager:
    """Two pinned host buffers used alternately for H2D uploads: packing batch i+1 on the host overlaps the copy of
    batch i, and a buffer is reused only after the copy that read it has finished (event)."""

    def __init__(self, n: int = 2):
        self.bufs, self.events, self.i = [None] * n, [None] * n, 0

    def stage(self, nbytes: int):
        self.i = (self.i + 1) % len(self.bufs)
        i = self.i
        if self.events[i] is not None:
            self.events[i].synchronize()
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(max(int(nbytes * 1.5), 1 << 20), dtype=torch.uint8).pin_memory()
        return self.bufs[i][:nbytes], i

    def copied(self, i: int):
        self.events[i] = torch.cuda.Event()
        self.events[i].record(torch.cuda.current_stream())


_stager = _HostStager()


def raw_image_layout(images):
    """(contiguous uint8 [h, w, 3] arrays, hw int32 [B, 2], byte offsets int64 [B], total bytes) of a sequence of decoded
    RGB images laid back to back"""
    arrs = [np.ascontiguousarray(im.cpu().numpy() if isinstance(im, torch.Tensor) else im, dtype=np.uint8) for im in images]
    assert len(arrs) > 0 and all(a.ndim == 3 and a.shape[2] == 3 for a in arrs)
    hw = np.array([a.shape[:2] for a in arrs], dtype=np.int32)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offsets = np.zeros(len(arrs), np.int64)
    offsets[1:] = np.cumsum(sizes)[:-1]
    return arrs, hw, offsets, int(sizes.sum())


class PackedRawImages:
    """A batch of decoded uint8 RGB images of ragged sizes ALREADY on the device, packed back to back: data uint8 [bytes],
    offsets int64 [B], hw int32 [B, 2] (device tensors), max_h = tallest image.  What mpreid.pipeline uploads for a
    RawImageBatch loader; ``resize_packed_u8`` turns it into the uint8 [B, H, W, 3] input of forward_u8."""

    def __init__(self, data, offsets, hw, count, max_h):
        self.data, self.offsets, self.hw, self.count, self.max_h = data, offsets, hw, int(count), int(max_h)

    def __len__(self):
        return self.count


RESIZE_FILTERS = {"bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC}


def resize_packed_u8(packed: PackedRawImages, out_hw, filter: Optional[str] = None) -> torch.Tensor:
    """the two resize kernels on images that are already packed in device memory (no host work, no copy); filter None is the
    bilinear entry point mpreid_resize_bilinear_u8, a name of RESIZE_FILTERS goes through mpreid_resize_u8"""
    dev = _lib.require_gpu()
    L = _lib.load()
    B, oh, ow = packed.count, int(out_hw[0]), int(out_hw[1])
    dst = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
    ws = _workspace("resize", L.mpreid_resize_workspace_bytes(B, packed.max_h, ow), dev)
    if filter is None:
        _lib.check(L.mpreid_resize_bilinear_u8(_ptr(packed.data), _ptr(packed.offsets), _ptr(packed.hw), B, packed.max_h, oh, ow,
                                               _ptr(dst), _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_resize_bilinear_u8")
    else:
        if filter not in RESIZE_FILTERS:
            raise ValueError(f"resize_u8: filter {filter!r} is none of {sorted(RESIZE_FILTERS)}")
        _lib.check(L.mpreid_resize_u8(_ptr(packed.data), _ptr(packed.offsets), _ptr(packed.hw), B, packed.max_h, oh, ow,
                                      RESIZE_FILTERS[filter], _ptr(dst), _ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "mpreid_resize_u8")
    return dst


def upload_raw_images(images) -> PackedRawImages:
    """decoded uint8 [h, w, 3] images of any sizes -> PackedRawImages: ONE H2D copy of the packed bytes through the pinned
    staging buffers"""
    dev = _lib.require_gpu()
    arrs, hw, offsets, total = raw_image_layout(images)
    packed, slot = _stager.stage(total)
    np.concatenate([a.reshape(-1) for a in arrs], out=packed.numpy())
    src = packed.to(dev, non_blocking=True)
    _stager.copied(slot)
    return PackedRawImages(src, torch.from_numpy(offsets).to(dev), torch.from_numpy(hw).to(dev), len(arrs), int(hw[:, 0].max()))


def resize_bilinear_u8(images, out_hw) -> torch.Tensor:
    """T.Resize(cfg.INPUT.SIZE_TEST) of val_transforms (datasets/make_dataloader.py:57-58) on the GPU, bit-exact with
    PIL.Image.resize(BILINEAR): images = sequence of uint8 [h, w, 3] arrays / tensors of any sizes (decoded RGB), or a
    PackedRawImages; returns uint8 [B, out_h, out_w, 3] on the device -- the input of VitEncoder.forward_u8.  One H2D
    copy of the packed bytes (pinned staging), two kernels."""
    if isinstance(images, PackedRawImages):
        return resize_packed_u8(images, out_hw)
    return resize_packed_u8(upload_raw_images(images), out_hw)


def resize_u8(images, out_hw, filter: str = "bilinear") -> torch.Tensor:
    """resize_bilinear_u8 with a filter: "bilinear" gives its bytes, "bicubic" is T.Resize(cfg.INPUT.SIZE_TRAIN, interpolation=3)
    of train_transforms (datasets/make_dataloader_uniprompt.py:54), bit-exact with PIL.Image.resize(BICUBIC)."""
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"resize_u8: filter {filter!r} is none of {sorted(RESIZE_FILTERS)}")
    if not isinstance(images, PackedRawImages):
        images = upload_raw_images(images)
    return resize_packed_u8(images, out_hw, filter)


def train_augment(img_u8: torch.Tensor, pad: int, params, sample_ids, seed: int, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5),
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mpreid_train_augment_f32 on a resized uint8 [B, H, W, 3] device batch: flip, pad + crop, ToTensor, Normalize and the erase
    box of each image as its row of params (int32 [B, 8]: flip, crop_top, crop_left, erase_top, erase_left, erase_h, erase_w, 0)
    says -> fp32 [B, 3, H, W].  The noise in a box depends on (seed, sample_ids[b], box) only."""
    dev = _lib.require_gpu()
    img = img_u8.detach().to(device=dev, dtype=torch.uint8).contiguous()
    assert img.dim() == 4 and img.shape[3] == 3, img.shape
    B, H, W = (int(v) for v in img.shape[:3])
    table = np.ascontiguousarray(params, dtype=np.int32)
    ids = np.ascontiguousarray(sample_ids, dtype=np.int64)
    if table.shape != (B, 8) or ids.shape != (B,):
        raise ValueError(f"train_augment: params is int32 [{B}, 8] and sample_ids int64 [{B}], got {table.shape} and {ids.shape}")
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, H, W) and out.is_cuda
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().mpreid_train_augment_f32(_ptr(img), B, H, W, int(pad), table.ctypes.data, ids.ctypes.data,
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, m, s, _ptr(out), _lib.stream_ptr()),
               "mpreid_train_augment_f32")
    return out


class TrainAugment:
    """The reference's train_transforms (datasets/make_dataloader_uniprompt.py:53-62) for decoded uint8 images, on the device:
    Resize(size_hw, bicubic) -> RandomHorizontalFlip(flip_p) -> Pad(pad) -> RandomCrop(size_hw) -> ToTensor -> Normalize(mean,
    std) -> timm RandomErasing(erase_p, mode='pixel', max_count=1).  The random decisions are drawn on the host by ``draw`` from
    the global torch / random generators in the order a num_workers=0 loader draws them, image after image: torch.rand(1) for the
    flip; two torch.randint(0, 2 pad + 1) for the crop (none when pad == 0); random.random() for the erase decision and, per
    attempt, random.uniform (area), random.uniform (log aspect) and, on the first box that fits, two random.randint.  The kernels
    take the decisions as a table: ``apply`` is one packed upload, the bicubic resize and mpreid_train_augment_f32.  The noise in
    an erase box is Philox4x32-10 keyed by ``seed`` and the image's sample id (include/mpreid.h): N(0, 1), not timm's bits."""

    MIN_AREA, MAX_AREA, MIN_ASPECT, MAX_ASPECT, ATTEMPTS = 0.02, 1.0 / 3.0, 0.3, 1.0 / 0.3, 10

    def __init__(self, size_hw, flip_p: float = 0.5, pad: int = 10, erase_p: float = 0.5, mean=(0.5, 0.5, 0.5),
                 std=(0.5, 0.5, 0.5), seed: int = 0):
        self.size_hw = (int(size_hw[0]), int(size_hw[1]))
        self.flip_p, self.pad, self.erase_p = float(flip_p), int(pad), float(erase_p)
        self.mean, self.std, self.seed = tuple(float(v) for v in mean), tuple(float(v) for v in std), int(seed)
        if self.pad < 0 or min(self.size_hw) < 1:
            raise ValueError("TrainAugment: pad >= 0 and a positive size")

    def _draw_erase(self):
        import math
        import random
        H, W = self.size_hw
        if random.random() > self.erase_p:
            return 0, 0, 0, 0
        lo, hi = math.log(self.MIN_ASPECT), math.log(self.MAX_ASPECT)
        for _ in range(self.ATTEMPTS):
            target = random.uniform(self.MIN_AREA, self.MAX_AREA) * (H * W)
            ar = math.exp(random.uniform(lo, hi))
            h, w = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if w < W and h < H:
                top, left = random.randint(0, H - h), random.randint(0, W - w)
                return (top, left, h, w) if h > 0 and w > 0 else (0, 0, 0, 0)   # an empty box erases nothing
        return 0, 0, 0, 0

    def draw(self, n: int) -> np.ndarray:
        """the int32 [n, 8] table of n images, drawn in the reference's order"""
        table = np.zeros((int(n), 8), dtype=np.int32)
        for r in table:
            r[0] = int(bool(torch.rand(1) < self.flip_p))
            if self.pad > 0:
                r[1] = int(torch.randint(0, 2 * self.pad + 1, size=(1,)).item())
                r[2] = int(torch.randint(0, 2 * self.pad + 1, size=(1,)).item())
            r[3:7] = self._draw_erase()
        return table

    def apply(self, raw_images, sample_ids, params=None) -> torch.Tensor:
        """decoded uint8 images (a sequence, or a PackedRawImages) + their sample ids -> fp32 [B, 3, H, W] on the device;
        params: the table to use instead of draw(B)"""
        n = len(raw_images)
        table = self.draw(n) if params is None else params
        resized = resize_u8(raw_images, self.size_hw, "bicubic")
        return train_augment(resized, self.pad, table, sample_ids, self.seed, self.mean, self.std)


# ----------------------------------------------------------------------------------------------
# The image batch of every encoder forward (include/mpreid.h: mpreid_image_in)
# ----------------------------------------------------------------------------------------------
#: (encoder, precision) -> (forward, workspace query, weights attribute, workspace-tag suffix, images per call).  The towers with
#: fp32 activations (and, RN50 fp32, an im2col matrix) take 4x-36x the bytes per image and run in chunks; None = the whole batch
_TOWERS = {
    ("vit", "fp16"): ("mpreid_vit_forward", "mpreid_vit_workspace_bytes", "c_w", "", None),
    ("vit", "split"): ("mpreid_vit_forward", "mpreid_vit_workspace_bytes", "c_w", "", None),
    ("vit", "fp32"): ("mpreid_vit_forward_f32", "mpreid_vit_workspace_bytes_f32", "c_w", "_f32", 64),
    ("rn50", "fp16"): ("mpreid_rn50_forward", "mpreid_rn50_workspace_bytes", "c_w", "", None),
    ("rn50", "split"): ("mpreid_rn50_forward_split", "mpreid_rn50_workspace_bytes_split", "c_ws", "_split", 256),
    ("rn50", "fp32"): ("mpreid_rn50_forward_f32", "mpreid_rn50_workspace_bytes_f32", "c_w", "_f32", 64),
}


@torch.no_grad()
def _stage_images(enc, img, u8: bool, view: int, cv_emb, pixel_mean, pixel_std):
    """An image batch as every tower entry point takes it -> (img on enc's device, cv_emb on it or None, the ImageIn
    descriptor pointing at the whole batch): fp32 [B,3,H,W], or, u8, uint8 [B,H,W,3]; cv_emb None or [B, width]"""
    if u8:
        img = img.detach().to(device=enc.device, dtype=torch.uint8).contiguous()
        assert tuple(img.shape[1:]) == enc.img_hw + (3,), img.shape
    else:
        img = _dev_f32(img, enc.device)
        assert tuple(img.shape[1:]) == (3,) + enc.img_hw, img.shape
    cv = None
    if cv_emb is not None:
        cv = _dev_f32(cv_emb, enc.device)
        assert tuple(cv.shape) == (img.shape[0], enc.cfg["width"]), cv.shape
    desc = _lib.ImageIn(mean=(C.c_float * 3)(*[float(x) for x in pixel_mean]),
                        std=(C.c_float * 3)(*[float(x) for x in pixel_std]), view=int(view))
    desc.f32_dev, desc.u8_hwc_dev = (None, img.data_ptr()) if u8 else (img.data_ptr(), None)
    return img, cv, desc


def _forward_images(enc, img, u8: bool, view: int = 0, cv_emb=None, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5),
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one path from an image batch to a tower: img is fp32 [B,3,H,W] (val_transforms applied) or, u8, uint8 [B,H,W,3]
    (after Resize; ToTensor + Normalize with pixel_mean / pixel_std and the view run inside the tower's first kernel).
    cv_emb: None or [B, width] (ViT only).  Validates, stages on enc's device, runs the tower chunk by chunk into out."""
    L = _lib.load()
    fwd, ws_query, weights, tag, step = _TOWERS[enc.tower, enc.precision]
    img, cv, desc = _stage_images(enc, img, u8, view, cv_emb, pixel_mean, pixel_std)
    B = img.shape[0]
    if out is None:
        out = torch.empty((B, enc.feat_dim), dtype=torch.float32, device=enc.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, enc.feat_dim)
    moe_arg = []
    if getattr(enc, "c_moe", None) is not None:   # the MoE image tower: its own entry points, the MoE description behind the weights
        fwd, ws_query, tag, moe_arg = "mpreid_vit_forward_moe", "mpreid_vit_workspace_bytes_moe", "_moe", [C.byref(enc.c_moe)]
    for s in range(0, B, step) if step else (0,):
        n = min(B, s + step) - s if step else B
        ws = _workspace(enc.ws_tag + tag, getattr(L, ws_query)(C.byref(enc.c_cfg), *moe_arg, n), enc.device)
        desc.f32_dev, desc.u8_hwc_dev = (None, img[s:].data_ptr()) if u8 else (img[s:].data_ptr(), None)
        cv_arg = [_ptr(None if cv is None else cv[s:s + n])] if enc.tower == "vit" else []
        _lib.check(getattr(L, fwd)(C.byref(enc.c_cfg), C.byref(getattr(enc, weights)), *moe_arg, C.byref(desc), n, *cv_arg,
                                   _ptr(out[s:]), _ptr(ws), ws.numel(), _lib.stream_ptr()), fwd)
    return out


# ----------------------------------------------------------------------------------------------
# ViT image encoder
# ----------------------------------------------------------------------------------------------
def resolve_moe(cfg: dict):
    """(num_experts, top_k, MoE blocks) of a tower cfg, as model/clip/model.py:294, 391 resolve them: the tower uses MoE when
    num_experts > 0 and top_k > 0; moe_layers == -1 means every block, a value above layers is clipped.  (0, 0, 0) for the
    dense tower, which includes moe_layers == 0."""
    n_exp, top_k, n_moe = (int(cfg.get(k, 0) or 0) for k in ("num_experts", "top_k", "moe_layers"))
    if not (n_exp > 0 and top_k > 0):
        return 0, 0, 0
    if top_k > n_exp:
        raise ValueError(f"MoE: top_k {top_k} > num_experts {n_exp} (torch.topk raises in the reference)")
    if n_moe < -1:
        raise ValueError(f"MoE: moe_layers {n_moe} (use -1 for every block)")
    n_moe = cfg["layers"] if n_moe == -1 else min(n_moe, cfg["layers"])
    if n_moe == 0:
        return 0, 0, 0
    if n_exp > _lib.MOE_MAX_EXPERTS or top_k > _lib.MOE_MAX_TOPK:
        raise NotImplementedError(f"MoE: num_experts {n_exp} / top_k {top_k} above the kernels' limits "
                                  f"({_lib.MOE_MAX_EXPERTS} / {_lib.MOE_MAX_TOPK})")
    return n_exp, top_k, n_moe


def _moe_gate_key(i: int) -> str:
    return f"transformer.resblocks.{i}.gate.weight"


def _moe_expert_keys(i: int, e: int):
    return [f"transformer.resblocks.{i}.experts.{e}.{lin}.{p}" for lin in ("c_fc", "c_proj") for p in ("weight", "bias")]


def check_moe_request(cfg: dict, state_dict: dict, precision: str):
    """Host-side validation of an MoE tower request; returns resolve_moe(cfg).  ValueError: top_k > num_experts, missing
    expert / gate keys; NotImplementedError: a precision other than 'split'.  Gates of blocks 1.. are accepted and unused."""
    n_exp, top_k, n_moe = resolve_moe(cfg)
    if not n_moe:
        return 0, 0, 0
    if precision != "split":
        raise NotImplementedError(f"the MoE image encoder runs in precision 'split' only (asked for {precision!r}): the router is "
                                  "fp32 end to end and the expert GEMMs keep the split mode's parity bound")
    have = lambda k: k in state_dict or "image_encoder." + k in state_dict   # noqa: E731
    for i in range(n_moe):
        missing = [k for e in range(n_exp) for k in _moe_expert_keys(i, e) if not have(k)]
        if i == 0 and not have(_moe_gate_key(0)):
            missing.append(_moe_gate_key(0))
        if missing:
            raise ValueError(f"MoE block {i}: the state dict lacks {len(missing)} expert / gate keys, first {missing[0]!r} "
                             f"(num_experts {n_exp}, moe_layers {n_moe})")
    return n_exp, top_k, n_moe


def _state_getter(state_dict, prefix: str):
    """get(name) -> the torch tensor of a state dict (numpy or torch) whose keys may carry `prefix`; a missing key is a
    KeyError, or None with required=False"""
    def get(name, required=True):
        for k in (name, prefix + name):
            if k in state_dict:
                v = state_dict[k]
                return torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
        if required:
            raise KeyError(name)
        return None
    return get


def _split_pack(t: torch.Tensor, out: Optional[torch.Tensor] = None):
    """A GEMM weight of the split precision: fp32 device matrix [n, k] -> (pair, 2^-e, src).  pair: fp16 [n][hi(k) | lo(k)] of
    W * 2^e with the largest finite |entry| in [2^9, 2^10) -- hi + lo carries 22 significant bits of every entry that matters,
    and 2^-e is undone in the GEMM epilogue (exact); written into `out` when given.  src: what the pack kernel reads on the
    current stream, so the caller keeps it alive until it has synchronised."""
    src = t.contiguous()
    n, k = src.shape
    amax = float(torch.nan_to_num(src, nan=0.0, posinf=0.0, neginf=0.0).abs().max())
    e = 9 - int(np.floor(np.log2(amax))) if amax > 0 else 0
    if out is None:
        out = torch.empty((n, 2 * k), dtype=torch.float16, device=src.device)
    _lib.check(_lib.load().mpreid_split_pack_f32(_ptr(src), n, k, float(2.0 ** e), _ptr(out), _lib.stream_ptr()),
               "mpreid_split_pack_f32")
    return out, float(2.0 ** -e), src


def _gemm_weight(t: torch.Tensor, precision: str):
    """fp32 device matrix -> (the GEMM operand of `precision`, its scale, the pack source): _split_pack, or the fp16 / fp32
    matrix itself with no scale and nothing to keep"""
    if precision == "split":
        return _split_pack(t)
    return (t.contiguous() if precision == "fp32" else t.to(torch.float16).contiguous()), None, None


def _fill_block(layer, load, i: int, w: int, dense_mlp: bool, precision: str = "split"):
    """Fills `layer` (a _lib.VitLayer, the *_s scales included) from CLIP's transformer.resblocks.{i}.* of width w; mlp.* only
    with dense_mlp.  load(name, shape) -> the fp32 device tensor of a key.  Returns (the tensors the struct points to, the
    pack sources of _split_pack)."""
    b = f"transformer.resblocks.{i}."
    lin = [("in_proj", "attn.in_proj_", 3 * w, w), ("out_proj", "attn.out_proj.", w, w)]
    if dense_mlp:
        lin += [("fc", "mlp.c_fc.", 4 * w, w), ("proj", "mlp.c_proj.", w, 4 * w)]
    t, src = {}, []
    for part, key, n, k in lin:
        t[part + "_w"], scale, s = _gemm_weight(load(b + key + "weight", (n, k)), precision)
        t[part + "_b"] = load(b + key + "bias", (n,))
        if scale is not None:
            setattr(layer, part + "_s", scale)
            src.append(s)
    for part, key in (("ln1", "ln_1."), ("ln2", "ln_2.")):
        t[part + "_g"], t[part + "_b"] = load(b + key + "weight", (w,)), load(b + key + "bias", (w,))
    for k, v in t.items():
        setattr(layer, k, v.data_ptr())
    return list(t.values()), src


class VitEncoder:
    """Device-resident CLIP ViT image encoder + feature head.

    cfg keys: h_res, w_res, patch, stride, width, layers, heads, out_dim (mpreid.synth.VIT_B16 layout); optional
    num_experts, top_k, moe_layers (default 0: the dense tower): the MoE tower of model/clip/model.py:283-330, whose first
    moe_layers blocks (-1: all) carry experts.{e}.c_fc / c_proj and gate.weight in place of mlp.* (split precision only;
    include/mpreid.h "MoE image encoder").
    state_dict: CLIP VisionTransformer key names (optionally prefixed 'image_encoder.'), numpy or torch.
    bn: optional dict(bottleneck=(weight, bias, running_mean, running_var), bottleneck_proj=(...)).
    """

    def __init__(self, cfg: dict, state_dict: dict, img_hw, neck_after: bool = False, bn: Optional[dict] = None,
                 device=None, cls_only_last: bool = True, ws_tag: str = "vit", precision: str = "split",
                 ln_fold: bool = False):
        """precision: 'split' (default: the parity-grade mode, as in config/node.py and bench.py) = every GEMM operand an fp16 pair hi + lo, products hi.hi' + lo.hi' + hi.lo' on the fp16
        matrix cores with fp32 accumulation -- fp32-grade features (~1e-6) at 3x the matrix work: the mode that meets
        the 1e-4 mAP bound AND is the measured one; 'fp16' = fp16 operands, fp32 accumulate / residual stream (fastest,
        relative feature error ~4e-4: misses the bound on hard data); 'fp32' = every weight and activation fp32, exact
        fp32 matrix instruction (~1e-6, ~1/8 of the fp16 throughput; mpreid_vit_forward_f32)."""
        assert precision in ("fp16", "fp32", "split"), precision
        self.tower = "vit"
        if ln_fold:
            raise ValueError("ln_fold: the folded-LayerNorm form of the split mode was removed in round 4 (0.5 % slower than the plain "
                             "split mode and not reproducible run to run at small batches: include/mpreid.h)")
        self.precision = precision
        # MoE tower (num_experts, top_k, moe_layers in cfg; all 0 = the dense tower): the first n_moe blocks carry experts.
        # Checked on the host, before a device is asked for.
        n_exp, top_k, n_moe = check_moe_request(cfg, state_dict, precision)
        self.device = device or _lib.require_gpu()
        self.ws_tag = ws_tag   # encoders that run concurrently on different streams need distinct workspaces
        self.cfg = dict(cfg)
        self.img_hw = tuple(img_hw)
        dev = self.device

        get = self._get = _state_getter(state_dict, "image_encoder.")
        self.masters = None   # enable_training()

        def f32(name, shape=None):   # (shapes are not checked here: the library's own checks and the asserts below)
            return get(name).to(device=dev, dtype=torch.float32).contiguous()

        w = cfg["width"]
        self._keep = []  # owns every device tensor referenced by the C structs
        keep = self._keep.append
        pack_src = []   # the pack kernels' fp32 sources: alive until the synchronize at the end
        self.c_cfg = _lib.VitCfg(self.img_hw[0], self.img_hw[1], cfg["patch"], cfg["stride"], cfg["h_res"],
                                 cfg["w_res"], w, cfg["layers"], cfg["heads"], cfg["out_dim"], int(bool(neck_after)),
                                 int(bool(cls_only_last)),
                                 _lib.VIT_SPLIT if precision == "split" else _lib.VIT_F16)
        layers = (_lib.VitLayer * max(cfg["layers"], 1))()
        for i in range(cfg["layers"]):
            kept, src = _fill_block(layers[i], f32, i, w, i >= n_moe, precision)
            self._keep += kept
            pack_src += src
        self._layers = layers
        self.c_moe = None
        if n_moe:
            # per MoE block the experts' matrices stacked [E][out][2 * in] as fp16 pairs, one power-of-two scale per expert
            # matrix by the rule of the dense layers (device arrays: the grouped GEMM looks its expert up on the device);
            # block 0's gate as fp32.  The gates of later blocks are never read (model/clip/model.py:314-322).
            moe_layers = (_lib.MoeLayer * n_moe)()
            for i in range(n_moe):
                b = f"transformer.resblocks.{i}"
                t = {}
                for part, key in (("fc", "c_fc"), ("proj", "c_proj")):
                    t[part + "_w"], t[part + "_s"] = _pack_experts(
                        (get(f"{b}.experts.{e}.{key}.weight") for e in range(n_exp)), n_exp, dev)
                    t[part + "_b"] = torch.stack([f32(f"{b}.experts.{e}.{key}.bias") for e in range(n_exp)]).contiguous()
                if i == 0:
                    t["gate_w"] = f32(_moe_gate_key(0))
                    assert tuple(t["gate_w"].shape) == (n_exp, w), t["gate_w"].shape
                for k, v in t.items():
                    keep(v)
                    setattr(moe_layers[i], k, v.data_ptr())
            self._moe_layers = moe_layers
            self.c_moe = _lib.VitMoe(n_exp, top_k, n_moe, C.cast(moe_layers, C.POINTER(_lib.MoeLayer)))
        conv_w, conv_s, src = _gemm_weight(f32("conv1.weight").reshape(w, -1), precision)   # fp32 in the all-fp32 mode
        pack_src.append(src)
        top = dict(conv_w=conv_w, class_emb=f32("class_embedding"),
                   pos_emb=f32("positional_embedding"), ln_pre_g=f32("ln_pre.weight"), ln_pre_b=f32("ln_pre.bias"),
                   ln_post_g=f32("ln_post.weight"), ln_post_b=f32("ln_post.bias"), proj=f32("proj"))
        L = cfg["h_res"] * cfg["w_res"] + 1
        assert tuple(top["pos_emb"].shape) == (L, w), (top["pos_emb"].shape, L, w)
        self.c_w = _lib.VitWeights()
        for k, v in top.items():
            keep(v)
            setattr(self.c_w, k, v.data_ptr())
        if precision == "split":
            self.c_w.conv_s = conv_s
        if bn is not None:
            for name, (sk, bk) in (("bottleneck", ("bn_scale", "bn_shift")),
                                   ("bottleneck_proj", ("bn_proj_scale", "bn_proj_shift"))):
                wt, bs, mu, var = (torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(
                    device=dev, dtype=torch.float32) for a in bn[name])
                scale = (wt / torch.sqrt(var + 1e-5)).contiguous()
                shift = (bs - mu * scale).contiguous()
                keep(scale), keep(shift)
                setattr(self.c_w, sk, scale.data_ptr())
                setattr(self.c_w, bk, shift.data_ptr())
        self.c_w.layers = C.cast(layers, C.POINTER(_lib.VitLayer))
        self.feat_dim = w + cfg["out_dim"]
        torch.cuda.current_stream().synchronize()   # the pack kernels are done with their fp32 sources

    def forward(self, img: torch.Tensor, cv_emb: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return _forward_images(self, img, False, cv_emb=cv_emb, out=out)

    __call__ = forward

    def forward_u8(self, img_hwc: torch.Tensor, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5),
                   cv_emb: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 images [B, H, W, 3] (after Resize); ToTensor + Normalize run inside the patch-gather kernel."""
        return _forward_images(self, img_hwc, True, VIEW_ORIGINAL, cv_emb, pixel_mean, pixel_std, out)

    def forward_view(self, img: torch.Tensor, view: int, cv_emb: Optional[torch.Tensor] = None,
                     pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5),
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One test-time-augmentation view (VIEW_ORIGINAL / VIEW_FLIP / VIEW_PSEUDO_IR / VIEW_PSEUDO_RGB) of a batch:
        img is either fp32 [B,3,H,W] (already normalised) or uint8 [B,H,W,3].  The view transform of
        processor/processor_uniprompt_stage2.py:605-633 happens inside the patch gather (all three precisions)."""
        return _forward_images(self, img, img.dtype == torch.uint8, view, cv_emb, pixel_mean, pixel_std, out)

    @torch.no_grad()
    def forward_tta(self, img: torch.Tensor, cv_emb: Optional[torch.Tensor] = None, views=(0, 1, 2, 3),
                    normalize: bool = True, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5)) -> torch.Tensor:
        """processor/processor_uniprompt_stage2.py:598-640: features of the views, averaged, then L2-normalised when
        TEST.FEAT_NORM is set."""
        B = img.shape[0]
        feats = torch.empty((len(views), B, self.feat_dim), dtype=torch.float32, device=self.device)
        for i, v in enumerate(views):
            self.forward_view(img, v, cv_emb, pixel_mean, pixel_std, out=feats[i])
        return tta_mean(feats, normalize)

    @torch.no_grad()
    def forward_train(self, img: torch.Tensor, cv_emb: Optional[torch.Tensor] = None, view: int = VIEW_ORIGINAL,
                      pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5), want_router: bool = False):
        """The three features stage 2 differentiates (mpreid_vit_forward_train) -> (f_last [B, width], f [B, width],
        f_proj [B, out_dim]): the CLS row of the last block's input, ln_post of the CLS row, and that @ proj; no BatchNorm neck
        (Stage2Head owns BNNeck).  f | f_proj carries the bits of forward() of an encoder without a neck.  img as forward_view
        takes it: fp32 [B,3,H,W] or uint8 [B,H,W,3], any view -- pixels are data, there is no pixel gradient.  The split
        precision only.
        An MoE tower (mpreid_vit_forward_train_moe): f_last is the CLS row of the last block's OUTPUT (model/clip/model.py:
        448-454), and want_router=True appends (router_logits [B * L, E] in rows b * L + l, l_aux [1] = the load-balancing loss
        of those logits)."""
        if self.precision != "split":
            raise NotImplementedError("forward_train: the ViT tower in the split precision only (no fp16 or fp32 tower)")
        L = _lib.load()
        img, cv, desc = _stage_images(self, img, img.dtype == torch.uint8, view, cv_emb, pixel_mean, pixel_std)
        B, w = img.shape[0], self.cfg["width"]
        f_last, f = (torch.empty((B, w), dtype=torch.float32, device=self.device) for _ in range(2))
        f_proj = torch.empty((B, self.cfg["out_dim"]), dtype=torch.float32, device=self.device)
        if self.c_moe is not None:
            n_tok = self.cfg["h_res"] * self.cfg["w_res"] + 1
            logits = torch.empty((B * n_tok, self.c_moe.num_experts), dtype=torch.float32, device=self.device) if want_router else None
            l_aux = torch.empty((1,), dtype=torch.float32, device=self.device) if want_router else None
            ws = _workspace(self.ws_tag + "_train_moe",
                            L.mpreid_vit_forward_train_moe_workspace_bytes(C.byref(self.c_cfg), C.byref(self.c_moe), B), self.device)
            _lib.check(L.mpreid_vit_forward_train_moe(C.byref(self.c_cfg), C.byref(self.c_w), C.byref(self.c_moe), C.byref(desc), B,
                                                      _ptr(cv), _ptr(f_last), _ptr(f), _ptr(f_proj), _ptr(logits), _ptr(l_aux),
                                                      _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_vit_forward_train_moe")
            return (f_last, f, f_proj, logits, l_aux) if want_router else (f_last, f, f_proj)
        if want_router:
            raise ValueError("forward_train: want_router needs an MoE tower")
        ws = _workspace(self.ws_tag, L.mpreid_vit_workspace_bytes(C.byref(self.c_cfg), B), self.device)
        _lib.check(L.mpreid_vit_forward_train(C.byref(self.c_cfg), C.byref(self.c_w), C.byref(desc), B, _ptr(cv), _ptr(f_last),
                                              _ptr(f), _ptr(f_proj), _ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "mpreid_vit_forward_train")
        return f_last, f, f_proj

    # ---- training (include/mpreid.h "The image tower's gradient") ----
    _LAYER_KEYS = dict(in_proj_w="attn.in_proj_weight", in_proj_b="attn.in_proj_bias", out_proj_w="attn.out_proj.weight",
                       out_proj_b="attn.out_proj.bias", fc_w="mlp.c_fc.weight", fc_b="mlp.c_fc.bias", proj_w="mlp.c_proj.weight",
                       proj_b="mlp.c_proj.bias", ln1_g="ln_1.weight", ln1_b="ln_1.bias", ln2_g="ln_2.weight", ln2_b="ln_2.bias")
    _TOWER_KEYS = dict(conv_w="conv1.weight", class_emb="class_embedding", pos_emb="positional_embedding",
                       ln_pre_g="ln_pre.weight", ln_pre_b="ln_pre.bias", ln_post_g="ln_post.weight", ln_post_b="ln_post.bias",
                       proj="proj")

    _MLP_FIELDS = ("fc_w", "fc_b", "proj_w", "proj_b")
    GATE_KEY = "transformer.resblocks.0.gate.weight"

    def _param_fields(self):
        """(reference key name, layer index or None, struct field) of every trained parameter, in a fixed order.  An MoE tower:
        the dense parameters of every block (an MoE block has no mlp.*) and block 0's gate.weight (field "gate_w").  Later gates
        are never read and the experts are frozen in stage 2: neither is a master, their .grad stays None."""
        n_moe = self.c_moe.moe_layers if self.c_moe is not None else 0
        out = [(key, None, field) for field, key in self._TOWER_KEYS.items()]
        for i in range(self.cfg["layers"]):
            out += [(f"transformer.resblocks.{i}.{key}", i, field) for field, key in self._LAYER_KEYS.items()
                    if i >= n_moe or field not in self._MLP_FIELDS]
        if n_moe:
            out.append((self.GATE_KEY, 0, "gate_w"))
        return out

    def _check_trainable(self, what: str):
        if self.precision != "split":
            raise NotImplementedError(f"{what}: the ViT tower in the split precision only (no fp16 or fp32 tower)")
        if self.cfg["layers"] < 1:
            raise NotImplementedError(f"{what}: a tower of at least one layer")

    def enable_training(self, masters: Optional[dict] = None):
        """fp32 master copies of every parameter as device tensors (leaves that require grad) in self.masters, under the
        reference's checkpoint key names and in its shapes; the split pairs the forward reads and the transposed fp32 copies
        [in][out] the gradient GEMMs read are rebuilt from them by sync_weights().  Returns self.masters.
        masters: {key: tensor} (keys optionally prefixed 'image_encoder.') to ADOPT as the masters instead of cloning -- fp32,
        contiguous, on the encoder's device, in the checkpoint's shapes; a model's own parameters become the masters that way,
        and whoever updates them calls sync_weights() / sync_weights_batched() afterwards."""
        self._check_trainable("enable_training")
        if masters is not None and self.c_moe is not None:
            for key, m in masters.items():
                if ".experts." in key and torch.is_tensor(m) and m.requires_grad:
                    raise NotImplementedError(f"enable_training: {key!r} requires grad, and the expert matrices' own gradients are "
                                              "not implemented (stage 2 freezes every parameter whose name contains 'expert'); "
                                              "missing: the grouped weight-gradient GEMMs per expert")
        if masters is not None:
            adopted = {}
            for key, _, _ in self._param_fields():
                m = masters[key] if key in masters else masters.get("image_encoder." + key)
                if m is None:
                    raise KeyError(f"enable_training: no master given for {key!r}")
                if not (torch.is_tensor(m) and m.dtype == torch.float32 and m.is_contiguous() and m.device == self.device
                        and tuple(m.shape) == tuple(self._get(key).shape)):
                    raise ValueError(f"enable_training: the master of {key!r} must be a contiguous fp32 tensor "
                                     f"{tuple(self._get(key).shape)} on {self.device}")
                adopted[key] = m
            self.masters = None
        if self.masters is None:
            self.masters = adopted if masters is not None else {
                key: self._get(key).to(device=self.device, dtype=torch.float32).contiguous().clone().requires_grad_(True)
                for key, _, _ in self._param_fields()}
            self._pairs, self._wt = {}, {}
            self._layers_t = (_lib.TextLayerT * self.cfg["layers"])()
            self.c_wt = _lib.VitWeightsT(C.cast(self._layers_t, C.POINTER(_lib.TextLayerT)))
            if self.c_moe is not None and getattr(self, "c_moe_t", None) is None:
                # the frozen experts' fp32 transposed copies, built once: what the gradient GEMMs through the experts multiply by
                n_moe, n_exp = self.c_moe.moe_layers, self.c_moe.num_experts
                self._moe_layers_t = (_lib.MoeLayerT * n_moe)()
                for i in range(n_moe):
                    for part, name in (("fc", "c_fc"), ("proj", "c_proj")):
                        t = torch.stack([self._get(f"transformer.resblocks.{i}.experts.{e}.{name}.weight").to(
                            device=self.device, dtype=torch.float32).t().contiguous() for e in range(n_exp)])
                        self._keep.append(t)
                        setattr(self._moe_layers_t[i], part + "_t", t.data_ptr())
                self.c_moe_t = _lib.VitMoeT(C.cast(self._moe_layers_t, C.POINTER(_lib.MoeLayerT)))
            self.sync_weights()
        return self.masters

    @torch.no_grad()
    def sync_weights(self):
        """Re-packs the forward's fp16 pairs and the transposed copies from the masters (after an optimizer step on them) and
        points the library's structs at the masters' vectors.  Reading each matrix's largest entry back for the pair's
        power-of-two scale synchronises with the device once per matrix."""
        L = _lib.load()
        for key, i, field in self._param_fields():
            m = self.masters[key]
            assert m.is_contiguous() and m.dtype == torch.float32 and m.device == self.device, key
            target = self.c_w if i is None else self._layers[i]
            if field == "gate_w":      # block 0's gate: the router reads the master itself (fp32, no pair)
                self._moe_layers[0].gate_w = m.data_ptr()
            elif field.endswith("_w"):   # a GEMM weight: conv_w and the four matrices of a block
                m2 = m.detach().reshape(m.shape[0], -1)
                pair, scale, _ = _split_pack(m2, out=self._pairs.get(key))
                self._pairs[key] = pair
                setattr(target, field, pair.data_ptr())
                setattr(target, field[:-2] + "_s" if i is not None else "conv_s", scale)
                if i is not None:
                    n, k = m2.shape
                    if key not in self._wt:
                        self._wt[key] = torch.empty((k, n), dtype=torch.float32, device=self.device)
                    _lib.check(L.mpreid_transpose_pad_f32(_ptr(m2), n, k, _ptr(self._wt[key]), n, _lib.stream_ptr()),
                               "mpreid_transpose_pad_f32")
                    setattr(self._layers_t[i], field[:-2] + "_t", self._wt[key].data_ptr())
            else:
                setattr(target, field, m.data_ptr())
        torch.cuda.current_stream().synchronize()

    @torch.no_grad()
    def sync_weights_batched(self):
        """sync_weights() with ONE wait for the device: the largest finite entry of all GEMM weights by one absmax_multi call
        (mpreid_absmax_multi_f32), one copy of those floats into pinned host memory, one synchronisation; the scales are then
        computed on the host as _split_pack computes them and the same pack and transpose launches follow, enqueued and not
        waited for (their sources are the masters, their targets the buffers this encoder keeps).  Leaves the pairs, the
        transposed copies, every scale and every struct pointer as sync_weights() leaves them, bit for bit."""
        if self.masters is None:
            raise RuntimeError("sync_weights_batched: call enable_training() first")
        L = _lib.load()
        fields = self._param_fields()
        mats = []
        for key, i, field in fields:
            m = self.masters[key]
            assert m.is_contiguous() and m.dtype == torch.float32 and m.device == self.device, key
            if field.endswith("_w") and field != "gate_w":
                mats.append((key, i, field, m.detach().reshape(m.shape[0], -1)))
        sb = getattr(self, "_sync_bufs", None)
        if sb is None or sb[0].numel() != len(mats):
            sb = self._sync_bufs = (torch.empty(len(mats), dtype=torch.float32, device=self.device),
                                    torch.empty(len(mats), dtype=torch.float32).pin_memory())
        absmax_multi([m2 for _, _, _, m2 in mats], out=sb[0])
        sb[1].copy_(sb[0], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        amax = sb[1].tolist()
        for (key, i, field, m2), a in zip(mats, amax):
            target = self.c_w if i is None else self._layers[i]
            e = 9 - int(np.floor(np.log2(a))) if a > 0 else 0
            n, k = m2.shape
            pair = self._pairs.get(key)
            if pair is None:
                pair = self._pairs[key] = torch.empty((n, 2 * k), dtype=torch.float16, device=self.device)
            _lib.check(L.mpreid_split_pack_f32(_ptr(m2), n, k, float(2.0 ** e), _ptr(pair), _lib.stream_ptr()), "mpreid_split_pack_f32")
            setattr(target, field, pair.data_ptr())
            setattr(target, field[:-2] + "_s" if i is not None else "conv_s", float(2.0 ** -e))
            if i is not None:
                if key not in self._wt:
                    self._wt[key] = torch.empty((k, n), dtype=torch.float32, device=self.device)
                _lib.check(L.mpreid_transpose_pad_f32(_ptr(m2), n, k, _ptr(self._wt[key]), n, _lib.stream_ptr()),
                           "mpreid_transpose_pad_f32")
                setattr(self._layers_t[i], field[:-2] + "_t", self._wt[key].data_ptr())
        for key, i, field in fields:
            if field == "gate_w":
                self._moe_layers[0].gate_w = self.masters[key].data_ptr()
            elif not field.endswith("_w"):
                setattr(self.c_w if i is None else self._layers[i], field, self.masters[key].data_ptr())

    @torch.no_grad()
    def backward(self, img: torch.Tensor, cv_emb: Optional[torch.Tensor], d_f_last: Optional[torch.Tensor],
                 d_f: Optional[torch.Tensor], d_f_proj: Optional[torch.Tensor], want=None, view: int = VIEW_ORIGINAL,
                 pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5), out: Optional[dict] = None, aux_coef: float = 0.0):
        """The gradients of sum(f_last o d_f_last) + sum(f o d_f) + sum(f_proj o d_f_proj) over forward_train's features
        (mpreid_vit_backward; a None seed is zero) -> {reference key name: fp32 gradient in the checkpoint's shape}.  want: the
        names to compute (default: every parameter, and "cv_emb" when cv_emb is given); "cv_emb" [B, width] is the gradient of
        the cv_emb rows as given, "tokens" [B, L, width] that of the embedded sequence.  Names left out cost nothing.
        out: optional {name: a contiguous fp32 device tensor of the gradient's shape} to write into (it may be a view into a
        larger buffer).  The call re-runs the forward itself; img as forward_train takes it (pixels are data: there is no
        pixel gradient).
        An MoE tower (mpreid_vit_backward_moe): + aux_coef * l_aux in the function differentiated, and
        "transformer.resblocks.0.gate.weight" among the names; aux_coef is ignored by a dense tower."""
        self._check_trainable("backward")
        if self.masters is None:
            raise RuntimeError("backward: call enable_training() first")
        L = _lib.load()
        img, cv, desc = _stage_images(self, img, img.dtype == torch.uint8, view, cv_emb, pixel_mean, pixel_std)
        B, w, od = img.shape[0], self.cfg["width"], self.cfg["out_dim"]
        fields = self._param_fields()
        if want is None:
            want = [key for key, _, _ in fields] + (["cv_emb"] if cv is not None else [])
        want = list(want)
        known = {key for key, _, _ in fields} | {"cv_emb", "tokens"}
        for name in want:
            if name not in known:
                raise KeyError(f"backward: no gradient named {name!r}")
        if "cv_emb" in want and cv is None:
            raise ValueError("backward: the gradient of cv_emb was asked for and no cv_emb given")
        seeds = []
        for t, dim, what in ((d_f_last, w, "d_f_last"), (d_f, w, "d_f"), (d_f_proj, od, "d_f_proj")):
            if t is not None:
                t = _dev_f32(t, self.device)
                if tuple(t.shape) != (B, dim):
                    raise ValueError(f"{what}: expected [{B}, {dim}], got {tuple(t.shape)}")
            seeds.append(t)
        given, out = out or {}, {}
        n_tok = self.cfg["h_res"] * self.cfg["w_res"] + 1
        shapes = {key: tuple(self.masters[key].shape) for key, _, _ in fields}
        shapes.update(cv_emb=(B, w), tokens=(B, n_tok, w))
        for name in want:
            out[name] = _f32_buffer(given.get(name), shapes[name], self.device, name)
        lg = (_lib.VitLayerGrads * self.cfg["layers"])()
        g = _lib.VitGrads()
        g.layers = C.cast(lg, C.POINTER(_lib.VitLayerGrads))
        for key, i, field in fields:
            if key in want and field != "gate_w":
                setattr(g if i is None else lg[i], field, out[key].data_ptr())
        if "cv_emb" in want:
            g.cv_emb = out["cv_emb"].data_ptr()
        if self.c_moe is not None:
            ws = _workspace(self.ws_tag + "_grad_moe",
                            L.mpreid_vit_backward_moe_workspace_bytes(C.byref(self.c_cfg), C.byref(self.c_moe), B), self.device)
            _lib.check(L.mpreid_vit_backward_moe(C.byref(self.c_cfg), C.byref(self.c_w), C.byref(self.c_wt), C.byref(self.c_moe),
                                                 C.byref(self.c_moe_t), C.byref(desc), B, _ptr(cv), _ptr(seeds[0]), _ptr(seeds[1]),
                                                 _ptr(seeds[2]), float(aux_coef), C.byref(g), _ptr(out.get(self.GATE_KEY)),
                                                 _ptr(out.get("tokens")), None, _ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "mpreid_vit_backward_moe")
            return out
        ws = _workspace(self.ws_tag + "_grad", L.mpreid_vit_backward_workspace_bytes(C.byref(self.c_cfg), B), self.device)
        _lib.check(L.mpreid_vit_backward(C.byref(self.c_cfg), C.byref(self.c_w), C.byref(self.c_wt), C.byref(desc), B, _ptr(cv),
                                         _ptr(seeds[0]), _ptr(seeds[1]), _ptr(seeds[2]), C.byref(g), _ptr(out.get("tokens")),
                                         _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_vit_backward")
        return out

    def forward_grad(self, img: torch.Tensor, cv_emb: Optional[torch.Tensor] = None, view: int = VIEW_ORIGINAL,
                     pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5)):
        """forward_train as a node of torch's autograd graph -> (f_last, f, f_proj), differentiable in self.masters and in
        cv_emb (not in the pixels): its backward is backward() with the incoming gradients, so torch.optim.* can drive the
        masters; call sync_weights() after each optimizer step.
        An MoE tower -> (f_last, f, f_proj, router_logits, l_aux): the logits are data (non-differentiable); l_aux [1] is
        differentiable, and the gradient that reaches it is backward()'s aux_coef (read back once per backward)."""
        self._check_trainable("forward_grad")
        if self.masters is None:
            raise RuntimeError("forward_grad: call enable_training() first")
        keys = [key for key, _, _ in self._param_fields()]
        return _VitForwardGrad.apply(self, img, (view, pixel_mean, pixel_std), keys, cv_emb, *[self.masters[k] for k in keys])

    def clone_for_stream(self, ws_tag: str) -> "VitEncoder":
        """a second handle on the same device weights with its own workspace (for a second HIP stream)"""
        import copy
        other = copy.copy(self)
        other.ws_tag = ws_tag
        return other


class _VitForwardGrad(torch.autograd.Function):
    """VitEncoder.forward_grad"""

    @staticmethod
    def forward(ctx, enc, img, how, keys, cv_emb, *masters):
        ctx.enc, ctx.img, ctx.how, ctx.keys = enc, img, how, keys
        ctx.cv = None if cv_emb is None else cv_emb.detach()
        if enc.c_moe is None:
            return enc.forward_train(img, ctx.cv, *how)
        # an MoE tower: (f_last, f, f_proj, router_logits, l_aux).  The logits are data; l_aux is differentiable, and the
        # gradient that reaches it IS the coefficient of the load-balancing term in the caller's loss.
        out = enc.forward_train(img, ctx.cv, *how, want_router=True)
        ctx.mark_non_differentiable(out[3])
        return out

    @staticmethod
    def backward(ctx, d_f_last, d_f, d_f_proj, *router):
        need = ctx.needs_input_grad   # (enc, img, how, keys, cv_emb, *masters)
        want = [k for k, n in zip(ctx.keys, need[5:]) if n] + (["cv_emb"] if need[4] else [])
        aux = float(router[1]) if len(router) == 2 and router[1] is not None else 0.0   # (one read-back: the autograd path)
        g = ctx.enc.backward(ctx.img, ctx.cv, d_f_last, d_f, d_f_proj, want, *ctx.how, aux_coef=aux)
        return (None, None, None, None, g.get("cv_emb")) + tuple(g.get(k) for k in ctx.keys)


# ----------------------------------------------------------------------------------------------
# RN50 image encoder (CLIP ModifiedResNet, model/clip/model.py:10-148)
# ----------------------------------------------------------------------------------------------
def _pad_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _np64(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)


def fold_conv_bn(weight, bn=None, cin_pad: Optional[int] = None, eps: float = 1e-5):
    """Conv2d weight [cout, cin, k, k] (+ eval-mode BatchNorm2d (gamma, beta, running_mean, running_var)) ->
    (fp16 [cout_pad128, k*k*cin_pad] with k order (kh, kw, c), fp32 bias [cout_pad128]); model/clip/model.py:17-24:
    y = gamma * (conv(x) - mean) / sqrt(var + eps) + beta = conv'(x) + b'.  Folded in fp64, rounded once."""
    w = np.asarray(weight, dtype=np.float64)
    cout, cin, kh, kw = w.shape
    if bn is not None:
        gamma, beta, mean, var = (np.asarray(a, dtype=np.float64) for a in bn)
        scale = gamma / np.sqrt(var + eps)
        w = w * scale[:, None, None, None]
        b = beta - mean * scale
    else:
        b = np.zeros(cout)
    cpad = cin if cin_pad is None else cin_pad
    npad = _pad_to(cout, 128)
    wk = np.zeros((npad, kh, kw, cpad), dtype=np.float32)
    wk[:cout, :, :, :cin] = w.transpose(0, 2, 3, 1)
    bk = np.zeros(npad, dtype=np.float32)
    bk[:cout] = b
    return (torch.from_numpy(wk.reshape(npad, kh * kw * cpad)).to(torch.float16), torch.from_numpy(bk))


_zero_pages = {}


def _zero_page(dev):
    if dev not in _zero_pages:
        _zero_pages[dev] = torch.zeros(256, dtype=torch.uint8, device=dev)
    return _zero_pages[dev]


def conv_f16_nhwc(act: torch.Tensor, wgt: torch.Tensor, bias: torch.Tensor, cout: int, taps: int,
                  identity: Optional[torch.Tensor] = None, relu: bool = True) -> torch.Tensor:
    """one folded conv layer on NHWC fp16 [B,H,W,Cin] -> [B,H,W,cout] (stride 1; taps 1 or 9 with pad 1)"""
    dev = _lib.require_gpu()
    assert act.dtype == torch.float16 and act.is_contiguous() and act.is_cuda and wgt.dtype == torch.float16
    B, H, W, C = act.shape
    assert wgt.shape[1] == taps * C and wgt.shape[0] % 128 == 0 and bias.numel() == wgt.shape[0]
    out = torch.empty((B, H, W, cout), dtype=torch.float16, device=dev)
    if identity is not None:
        assert identity.dtype == torch.float16 and identity.is_contiguous() and tuple(identity.shape) == tuple(out.shape)
    _lib.check(_lib.load().mpreid_conv_f16_nhwc(_ptr(act), B, H, W, C, _ptr(wgt), _ptr(bias), cout, wgt.shape[0], taps,
                                                _ptr(identity), int(relu), _ptr(out), _ptr(_zero_page(dev)),
                                                _lib.stream_ptr()), "mpreid_conv_f16_nhwc")
    return out


def pairs_of(w2d, bias, cin: int, taps: int, dev):
    """folded fp32 matrix [cout][taps * cin] + bias -> (Rn50ConvSplit, [pair matrix, bias]): the zero-padded fp16 pair
    matrix [npad][hi(kseg) | lo(kseg)] of W * 2^e (include/mpreid.h, mpreid_rn50_conv_split); the two device tensors
    must outlive the struct, which holds their addresses"""
    cout, k = w2d.shape
    kseg, npad = _pad_to(k, 64), _pad_to(cout, 128)
    wp = np.zeros((npad, kseg), np.float32)
    wp[:cout, :k] = w2d.astype(np.float32)
    bp = np.zeros(npad, np.float32)
    bp[:cout] = bias
    amax = float(np.abs(wp).max())
    e = 9 - int(np.floor(np.log2(amax))) if amax > 0 and np.isfinite(amax) else 0
    wt = torch.from_numpy(wp).to(dev)
    pair = torch.empty((npad, 2 * kseg), dtype=torch.float16, device=dev)
    _lib.check(_lib.load().mpreid_split_pack_f32(_ptr(wt), npad, kseg, float(2.0 ** e), _ptr(pair), _lib.stream_ptr()),
               "mpreid_split_pack_f32")
    torch.cuda.current_stream().synchronize()   # wt is a temporary of this call
    bt = torch.from_numpy(bp).to(dev)
    return _lib.Rn50ConvSplit(_ptr(pair), _ptr(bt), cin, cout, taps, kseg, npad, float(2.0 ** -e)), [pair, bt]


def pairs_of_3x3(w, bias, dev):
    """folded [cout][cin][3][3] + bias -> (Rn50ConvSplit, [slabs, bias]) for the implicit GEMM (csrc/conv_f16.hip, pair
    form): fp16 slabs [cout_pad128][tap][cin_pad64 / 64][hi(64) | lo(64)] of W * 2^e; kseg = cin_pad64"""
    cout, cin = w.shape[:2]
    cp, npad = _pad_to(cin, 64), _pad_to(cout, 128)
    wp = np.zeros((npad, 9, cp), np.float32)
    wp[:cout, :, :cin] = w.transpose(0, 2, 3, 1).reshape(cout, 9, cin).astype(np.float32)
    bp = np.zeros(npad, np.float32)
    bp[:cout] = bias
    amax = float(np.abs(wp).max())
    e = 9 - int(np.floor(np.log2(amax))) if amax > 0 and np.isfinite(amax) else 0
    wt = torch.from_numpy(wp).to(dev) * float(2.0 ** e)          # exact: a power of two
    hi = wt.half()
    lo = (wt - hi.float()).half()
    hi, lo = hi.view(npad, 9, cp // 64, 1, 64), lo.view(npad, 9, cp // 64, 1, 64)
    slab = torch.cat([hi, lo], dim=3).reshape(npad, 9 * (cp // 64) * 2 * 64).contiguous()
    bt = torch.from_numpy(bp).to(dev)
    return _lib.Rn50ConvSplit(_ptr(slab), _ptr(bt), cin, cout, 9, cp, npad, float(2.0 ** -e)), [slab, bt]


def conv_split_layer(conv, B: int, H: int, W: int, x: Optional[torch.Tensor] = None, relu_in: bool = False,
                     in_pairs: Optional[torch.Tensor] = None, res: int = 0, out: Optional[torch.Tensor] = None,
                     pair_c: int = 0, pair_out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """one convolution of the split RN50 tower (mpreid_rn50_conv_split_layer, include/mpreid.h) -> (out, pair_out).
    conv: an Rn50ConvSplit (pairs_of / pairs_of_3x3).  x: fp32 [B*H*W, ld_in] NHWC rows (ReLU on read with relu_in), or
    in_pairs: fp16 [Mp, 2 * kseg], Mp = B*H*W rounded up to 256.  out: fp32 [Mp, npad] (res 1: += ; res 2: max(out, 0) +);
    pair_c > 0: the ReLU-ed result as fp16 pairs [Mp, 2 * pair_c] -- instead of `out` when res == 0, beside it otherwise.
    Buffers that are not passed are allocated (uninitialised: see the header for the rows that are written)."""
    dev = _lib.require_gpu()
    M = B * H * W
    Mp = _pad_to(M, 256)
    if x is not None:
        assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[0] == M
        if scratch is None:
            scratch = torch.empty((Mp, 2 * conv.kseg), dtype=torch.float16, device=dev)
        assert scratch.dtype == torch.float16 and scratch.is_contiguous() and scratch.numel() >= Mp * 2 * conv.kseg
    if in_pairs is not None:
        assert in_pairs.dtype == torch.float16 and in_pairs.is_contiguous() and tuple(in_pairs.shape) == (Mp, 2 * conv.kseg)
    if pair_c and pair_out is None:
        pair_out = torch.empty((Mp, 2 * pair_c), dtype=torch.float16, device=dev)
    if pair_out is not None:
        assert pair_out.dtype == torch.float16 and pair_out.is_contiguous() and tuple(pair_out.shape) == (Mp, 2 * pair_c)
    if out is None and (res or pair_out is None):
        assert not res, "a residual form adds onto `out`"
        out = torch.empty((Mp, conv.npad), dtype=torch.float32, device=dev)
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (Mp, conv.npad)
    _lib.check(_lib.load().mpreid_rn50_conv_split_layer(
        C.byref(conv), _ptr(x), 0 if x is None else x.shape[1], int(relu_in), _ptr(in_pairs), B, H, W, int(res), _ptr(out),
        _ptr(pair_out), int(pair_c), _ptr(scratch), _ptr(_zero_page(dev)), _lib.stream_ptr()), "mpreid_rn50_conv_split_layer")
    return out, pair_out


def vit_attention(qkv: torch.Tensor, batch: int, tokens: int, heads: int, q_tiles: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the encoder's attention step alone (mpreid_vit_attention, include/mpreid.h).  qkv: [batch * tokens, 3 * 64 * heads],
    fp32 (split precision) or fp16.  out: fp16 [batch * tokens, 2 * width] = [hi | lo] for fp32 input, [batch * tokens, width]
    for fp16 input; allocated (uninitialised) when not passed.  q_tiles > 0 writes only the first 16 * q_tiles rows of every
    image.  `out` may be a view into a larger buffer (the tests put guard rows around it)."""
    _lib.require_gpu()
    width = 64 * heads
    assert qkv.is_cuda and qkv.is_contiguous() and tuple(qkv.shape) == (batch * tokens, 3 * width)
    assert qkv.dtype in (torch.float32, torch.float16)
    split = qkv.dtype == torch.float32
    cols = 2 * width if split else width
    if out is None:
        out = torch.empty((batch * tokens, cols), dtype=torch.float16, device=qkv.device)
    assert out.dtype == torch.float16 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (batch * tokens, cols)
    _lib.check(_lib.load().mpreid_vit_attention(_ptr(qkv), _lib.VIT_SPLIT if split else _lib.VIT_F16, int(batch), int(tokens),
                                                width, int(heads), int(q_tiles), _ptr(out), _lib.stream_ptr()),
               "mpreid_vit_attention")
    return out


def vit_attention_f32(qkv: torch.Tensor, batch: int, tokens: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the attention step of the all-fp32 encoder mode alone (mpreid_vit_attention_f32): the resident / chunked rule of
    mpreid_vit_forward_f32.  qkv: fp32 [batch * tokens, 3 * 64 * heads] in the column layout of vit_attention; out: fp32
    [batch * tokens, width], allocated (uninitialised) when not passed; may be a view into a larger buffer."""
    _lib.require_gpu()
    width = 64 * heads
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.dtype == torch.float32 and tuple(qkv.shape) == (batch * tokens, 3 * width)
    if out is None:
        out = torch.empty((batch * tokens, width), dtype=torch.float32, device=qkv.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (batch * tokens, width)
    _lib.check(_lib.load().mpreid_vit_attention_f32(_ptr(qkv), int(batch), int(tokens), width, int(heads), _ptr(out),
                                                    _lib.stream_ptr()), "mpreid_vit_attention_f32")
    return out


def vit_attention_backward(qkv: torch.Tensor, d_o: torch.Tensor, batch: int, tokens: int, heads: int,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the image tower's unmasked attention gradient alone (mpreid_vit_attention_backward).  qkv: fp32 [batch * tokens, 3 * width]
    in the column layout of vit_attention, d_o: fp32 [batch * tokens, width] -> dq | dk | dv, fp32 [batch * tokens, 3 * width];
    `out` may be a view into a larger buffer (the tests put guard rows around it).  2 <= tokens <= MPREID_VIT_MAX_TOKENS."""
    dev = _lib.require_gpu()
    width = 64 * heads
    assert qkv.is_cuda and qkv.is_contiguous() and tuple(qkv.shape) == (batch * tokens, 3 * width)
    assert d_o.is_cuda and d_o.is_contiguous() and tuple(d_o.shape) == (batch * tokens, width)
    if qkv.dtype != torch.float32 or d_o.dtype != torch.float32:
        raise RuntimeError(f"mpreid_vit_attention_backward failed (code {_lib.ERR_UNSUPPORTED}): gradients are fp32 only")
    if out is None:
        out = torch.empty((batch * tokens, 3 * width), dtype=torch.float32, device=qkv.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (batch * tokens, 3 * width)
    L = _lib.load()
    ws = _workspace("vit_attention_backward", L.mpreid_vit_attention_backward_workspace_bytes(int(batch), int(tokens), int(heads)), dev)
    _lib.check(L.mpreid_vit_attention_backward(_ptr(qkv), _ptr(d_o), int(batch), int(tokens), width, int(heads), _ptr(out),
                                               _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_vit_attention_backward")
    return out


# ----------------------------------------------------------------------------------------------
# MoE unit seams (include/mpreid.h: mpreid_moe_route, mpreid_moe_mlp_split)
# ----------------------------------------------------------------------------------------------
def moe_route(x: torch.Tensor, gate: torch.Tensor, top_k: int, ln=None, want_logits: bool = False):
    """The router alone.  x fp32 [rows, width]: the residual stream with ln = (gamma, beta) of the LayerNorm in front of the
    gate, or h itself with ln = None; gate fp32 [E, width].  Returns (sel int32 [rows, K], w fp32 [rows, K], logits fp32
    [rows, E] or None)."""
    dev = _lib.require_gpu()
    x, gate = _dev_f32(x, dev), _dev_f32(gate, dev)
    rows, width = x.shape
    E, K = gate.shape[0], int(top_k)
    assert gate.shape[1] == width, (gate.shape, width)
    g = b = None
    if ln is not None:
        g, b = _dev_f32(ln[0], dev), _dev_f32(ln[1], dev)
        assert g.numel() == width and b.numel() == width
    sel = torch.empty((rows, max(K, 1)), dtype=torch.int32, device=dev)
    w = torch.empty((rows, max(K, 1)), dtype=torch.float32, device=dev)
    logits = torch.empty((rows, E), dtype=torch.float32, device=dev) if want_logits else None
    _lib.check(_lib.load().mpreid_moe_route(_ptr(x), rows, width, _ptr(g), _ptr(b), _ptr(gate), E, K, _ptr(sel), _ptr(w),
                                            _ptr(logits), _lib.stream_ptr()), "mpreid_moe_route")
    return sel, w, logits


def _pack_experts(mats, n_exp: int, dev):
    """n_exp fp32 matrices [out, in] (an iterable: one is on the device at a time) -> (fp16 pairs [E][out][2 * in], fp32 [E] of
    2^-e): every expert is packed straight into its slice of the one stacked buffer, by the dense layers' packer (_split_pack)"""
    pair, sc = None, []
    for e, m in enumerate(mats):
        t = _dev_f32(m, dev)
        n, k = t.shape
        if pair is None:
            pair = torch.empty((n_exp, n, 2 * k), dtype=torch.float16, device=dev)
        assert tuple(pair.shape[1:]) == (n, 2 * k), (e, tuple(t.shape))
        _, scale, src = _split_pack(t, out=pair[e])
        sc.append(scale)
        torch.cuda.current_stream().synchronize()   # t (= src) is a temporary: one expert's fp32 matrix on the device at a time
        del t, src
    assert len(sc) == n_exp
    return pair, torch.tensor(sc, dtype=torch.float32, device=dev)


def pack_moe_layer(fc_w, fc_b, proj_w, proj_b, dev=None):
    """fp32 expert weights [E, 4w, w], [E, 4w], [E, w, 4w], [E, w] -> (mpreid_moe_layer, the tensors it points to): the stacked
    fp16 pair layout and one power-of-two scale per expert matrix, as VitEncoder builds them (no gate)."""
    dev = dev or _lib.require_gpu()
    keep = []
    layer = _lib.MoeLayer()
    for part, wt, bs in (("fc", fc_w, fc_b), ("proj", proj_w, proj_b)):
        bs = _dev_f32(bs, dev)
        pair, s = _pack_experts(wt, len(wt), dev)
        keep += [bs, pair, s]
        setattr(layer, part + "_w", pair.data_ptr())
        setattr(layer, part + "_b", bs.data_ptr())
        setattr(layer, part + "_s", s.data_ptr())
    torch.cuda.current_stream().synchronize()
    return layer, keep


def moe_mlp(a_pairs: torch.Tensor, sel: torch.Tensor, w: torch.Tensor, layer, x: torch.Tensor, num_experts: int,
            ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The routed MLP alone, in place: x[row] += sum over the row's experts (ascending) of w * expert(a[row]).  a_pairs fp16
    [rows, 2 * width] ([hi | lo], split_pairs(h)); sel int32 / w fp32 [rows, K]; layer from pack_moe_layer; x fp32, at least
    rows rows of width.  ws: a uint8 workspace of the caller's (the tests put guard bytes behind it)."""
    dev = _lib.require_gpu()
    L = _lib.load()
    rows, K = sel.shape
    width = a_pairs.shape[1] // 2
    assert a_pairs.dtype == torch.float16 and a_pairs.is_cuda and a_pairs.is_contiguous() and a_pairs.shape[0] >= rows
    assert sel.dtype == torch.int32 and w.dtype == torch.float32 and sel.is_contiguous() and w.is_contiguous() and w.shape == sel.shape
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.shape[0] >= rows and x.shape[1] == width
    if ws is None:
        ws = _workspace("moe_mlp", L.mpreid_moe_workspace_bytes(rows, width, int(num_experts), K), dev)
    _lib.check(L.mpreid_moe_mlp_split(_ptr(a_pairs), rows, width, _ptr(sel), _ptr(w), int(num_experts), K, C.byref(layer), _ptr(x),
                                      _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_moe_mlp_split")
    return x


def pack_moe_layer_t(fc_w, proj_w, dev=None):
    """fp32 expert weights [E, 4w, w] and [E, w, 4w] (the checkpoint's [out][in]) -> (mpreid_moe_layer_t, the tensors it points
    to): per expert the fp32 transpose, fc_t [E, w, 4w] and proj_t [E, 4w, w], what the gradient GEMMs multiply by"""
    dev = dev or _lib.require_gpu()
    keep = []
    lt = _lib.MoeLayerT()
    for part, wt in (("fc", fc_w), ("proj", proj_w)):
        t = torch.stack([_dev_f32(m, dev).t().contiguous() for m in wt])
        keep.append(t)
        setattr(lt, part + "_t", t.data_ptr())
    return lt, keep


def _refuse_expert_grads(d_experts):
    if d_experts is not None and any(v is not None for v in (d_experts.values() if isinstance(d_experts, dict) else d_experts)):
        raise NotImplementedError("MoE backward: the expert matrices' own gradients are not implemented (stage 2 freezes every "
                                  "parameter whose name contains 'expert'); missing: the grouped weight-gradient GEMMs per expert")


def moe_mlp_backward(a_pairs: torch.Tensor, sel: torch.Tensor, w: torch.Tensor, layer, layer_t, dy: torch.Tensor, num_experts: int,
                     d_a: Optional[torch.Tensor] = None, d_w: Optional[torch.Tensor] = None, accumulate_d_w: bool = False,
                     want_d_a: bool = True, want_d_w: bool = True, d_experts=None, ws: Optional[torch.Tensor] = None):
    """The gradient through one routed MLP (include/mpreid.h: mpreid_moe_mlp_backward).  a_pairs / sel / w / layer as for
    moe_mlp, layer_t from pack_moe_layer_t, dy fp32 [rows, width].  Returns (d_a fp32 [rows, width] or None, d_w fp32 [rows, K]
    or None); d_w is added to the caller's tensor with accumulate_d_w.  d_experts: must be None (not implemented)."""
    _refuse_expert_grads(d_experts)
    dev = _lib.require_gpu()
    L = _lib.load()
    rows, K = sel.shape
    width = a_pairs.shape[1] // 2
    assert a_pairs.dtype == torch.float16 and a_pairs.is_cuda and a_pairs.is_contiguous() and a_pairs.shape[0] >= rows
    assert sel.dtype == torch.int32 and w.dtype == torch.float32 and sel.is_contiguous() and w.is_contiguous() and w.shape == sel.shape
    assert dy.dtype == torch.float32 and dy.is_cuda and dy.is_contiguous() and dy.shape[0] >= rows and dy.shape[1] == width
    assert want_d_a or want_d_w
    if want_d_a and d_a is None:
        d_a = torch.empty((rows, width), dtype=torch.float32, device=dev)
    if want_d_w and d_w is None:
        assert not accumulate_d_w, "accumulate_d_w needs the caller's d_w"
        d_w = torch.empty((rows, K), dtype=torch.float32, device=dev)
    for t, cols in ((d_a if want_d_a else None, width), (d_w if want_d_w else None, K)):
        assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.shape[0] >= rows and t.shape[1] == cols)
    if ws is None:
        ws = _workspace("moe_grad", L.mpreid_moe_grad_workspace_bytes(rows, width, int(num_experts), K), dev)
    _lib.check(L.mpreid_moe_mlp_backward(_ptr(a_pairs), rows, width, _ptr(sel), _ptr(w), int(num_experts), K, C.byref(layer),
                                         C.byref(layer_t), _ptr(dy), _ptr(d_a if want_d_a else None),
                                         _ptr(d_w if want_d_w else None), int(bool(accumulate_d_w)), None, _ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "mpreid_moe_mlp_backward")
    return (d_a if want_d_a else None), (d_w if want_d_w else None)


def moe_route_backward(logits: torch.Tensor, sel: torch.Tensor, w: torch.Tensor, d_w: Optional[torch.Tensor], aux_coef: float = 0.0,
                       want_d_logits: bool = True, want_l_aux: bool = True, ws: Optional[torch.Tensor] = None):
    """The router's gradient and the load-balancing loss (include/mpreid.h: mpreid_moe_route_backward).  logits fp32 [rows, E],
    sel int32 / w fp32 [rows, K] of moe_route, d_w fp32 [rows, K] or None (zeros).  Returns (d_logits fp32 [rows, E] or None,
    l_aux fp32 [1] or None); l_aux is the reference's load_balancing_loss_func of these logits, NOT multiplied by aux_coef."""
    dev = _lib.require_gpu()
    L = _lib.load()
    rows, E = logits.shape
    K = sel.shape[1]
    assert logits.dtype == torch.float32 and logits.is_cuda and logits.is_contiguous()
    assert sel.dtype == torch.int32 and w.dtype == torch.float32 and sel.is_cuda and w.is_cuda and sel.is_contiguous() and \
        w.is_contiguous() and tuple(sel.shape) == (rows, K) and w.shape == sel.shape
    assert d_w is None or (d_w.dtype == torch.float32 and d_w.is_cuda and d_w.is_contiguous() and d_w.shape == sel.shape)
    assert want_d_logits or want_l_aux
    d_logits = torch.empty((rows, E), dtype=torch.float32, device=dev) if want_d_logits else None
    l_aux = torch.empty((1,), dtype=torch.float32, device=dev) if want_l_aux else None
    if ws is None:
        ws = _workspace("moe_route_grad", L.mpreid_moe_route_backward_workspace_bytes(rows, E), dev)
    _lib.check(L.mpreid_moe_route_backward(_ptr(logits), rows, E, K, _ptr(sel), _ptr(w), _ptr(d_w), float(aux_coef), _ptr(d_logits),
                                           _ptr(l_aux), _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_moe_route_backward")
    return d_logits, l_aux


def split_pairs_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, k] -> fp16 pairs [rows, 2k] = [hi | lo] (mpreid_split_pack_f32 with scale 1): the operand layout of the
    split mode, as layernorm writes it"""
    dev = _lib.require_gpu()
    x = _dev_f32(x, dev)
    out = torch.empty((x.shape[0], 2 * x.shape[1]), dtype=torch.float16, device=dev)
    _lib.check(_lib.load().mpreid_split_pack_f32(_ptr(x), x.shape[0], x.shape[1], 1.0, _ptr(out), _lib.stream_ptr()),
               "mpreid_split_pack_f32")
    return out


# ----------------------------------------------------------------------------------------------
# CLIP text tower (include/mpreid.h: mpreid_text_forward)
# ----------------------------------------------------------------------------------------------
def _text_unsupported(what: str):
    """the text tower is built in the split precision only (include/mpreid.h): any other request is MPREID_ERR_UNSUPPORTED"""
    raise RuntimeError(f"{what} failed (code {_lib.ERR_UNSUPPORTED}): the text tower runs in the split precision only; there is "
                       "no fp16 and no all-fp32 text mode")


def text_attention(qkv: torch.Tensor, batch: int, tokens: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the text tower's causal attention step alone (mpreid_text_attention).  qkv: fp32 [batch * tokens, 3 * 64 * heads] in
    the column layout of vit_attention; out: fp16 [batch * tokens, 2 * width] = [hi | lo], allocated (uninitialised) when
    not passed; it may be a view into a larger buffer (the tests put guard rows around it)."""
    _lib.require_gpu()
    width = 64 * heads
    assert qkv.is_cuda and qkv.is_contiguous() and tuple(qkv.shape) == (batch * tokens, 3 * width)
    if qkv.dtype != torch.float32:
        _text_unsupported("mpreid_text_attention")
    if out is None:
        out = torch.empty((batch * tokens, 2 * width), dtype=torch.float16, device=qkv.device)
    assert out.dtype == torch.float16 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (batch * tokens, 2 * width)
    _lib.check(_lib.load().mpreid_text_attention(_ptr(qkv), int(batch), int(tokens), width, int(heads), _ptr(out),
                                                 _lib.stream_ptr()), "mpreid_text_attention")
    return out


def text_attention_backward(qkv: torch.Tensor, d_o: torch.Tensor, batch: int, tokens: int, heads: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the causal attention backward kernel alone (mpreid_text_attention_backward).  qkv: fp32 [batch * tokens, 3 * width] as
    for text_attention, d_o: fp32 [batch * tokens, width] -> dq | dk | dv, fp32 [batch * tokens, 3 * width]; `out` may be a
    view into a larger buffer (the tests put guard rows around it)."""
    _lib.require_gpu()
    width = 64 * heads
    assert qkv.is_cuda and qkv.is_contiguous() and tuple(qkv.shape) == (batch * tokens, 3 * width)
    assert d_o.is_cuda and d_o.is_contiguous() and tuple(d_o.shape) == (batch * tokens, width)
    if qkv.dtype != torch.float32 or d_o.dtype != torch.float32:
        _text_unsupported("mpreid_text_attention_backward")
    if out is None:
        out = torch.empty((batch * tokens, 3 * width), dtype=torch.float32, device=qkv.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (batch * tokens, 3 * width)
    _lib.check(_lib.load().mpreid_text_attention_backward(_ptr(qkv), _ptr(d_o), int(batch), int(tokens), width, int(heads),
                                                          _ptr(out), _lib.stream_ptr()), "mpreid_text_attention_backward")
    return out


def layernorm_backward(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm's input gradient (mpreid_layernorm_backward_f32: biased variance, eps 1e-5, statistics recomputed from x).
    x, dy: fp32 [rows, width], gamma [width] -> dx [rows, width]; with `out` given the gradient is ADDED to it (the form of the
    residual joins) and `out` is returned."""
    dev = _lib.require_gpu()
    x, dy, gamma = _dev_f32(x, dev), _dev_f32(dy, dev), _dev_f32(gamma, dev)
    assert x.dim() == 2 and dy.shape == x.shape and tuple(gamma.shape) == (x.shape[1],)
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.shape == x.shape
    _lib.check(_lib.load().mpreid_layernorm_backward_f32(_ptr(x), _ptr(dy), _ptr(gamma), x.shape[0], x.shape[1], int(acc),
                                                         _ptr(out), _lib.stream_ptr()), "mpreid_layernorm_backward_f32")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, form: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the towers' forward LayerNorm alone (mpreid_layernorm_f32).  x: fp32 [rows, width] on the device, used as it is (it may
    be a view into a larger buffer).  form 0 -> fp32 [rows, width], and `out` may be x itself (ln_pre's in-place call); form 1
    -> fp16 [rows, width]; form 2 -> the fp16 pair [rows, 2 * width] = [hi | lo].  `out` is allocated when not passed."""
    dev = _lib.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    gamma, beta = _dev_f32(gamma, dev), _dev_f32(beta, dev)
    rows, width = x.shape
    assert tuple(gamma.shape) == (width,) and tuple(beta.shape) == (width,)
    shape, dtype = ((rows, width), torch.float32) if form == 0 else ((rows, width * (2 if form == 2 else 1)), torch.float16)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == shape
    _lib.check(_lib.load().mpreid_layernorm_f32(_ptr(x), rows, width, _ptr(gamma), _ptr(beta), int(form), _ptr(out),
                                                _lib.stream_ptr()), "mpreid_layernorm_f32")
    return out


def tower_head(x: torch.Tensor, item_stride: int, row_of: Optional[torch.Tensor], tokens: int, batch: int, ln_g: torch.Tensor,
               ln_b: torch.Tensor, proj: torch.Tensor, bn=None, bnp=None, ln_to_out: bool = True,
               out: Optional[torch.Tensor] = None, out_col: Optional[int] = None):
    """the head of every tower alone (mpreid_tower_head_f32) -> (y [batch, width], out).  x: fp32 on the device, item b at
    b * item_stride floats; its row is row 0, or row row_of[b] (int32, clamped into the item's `tokens` rows by the kernel).
    proj: [width, out_dim]; bn / bnp: optional (scale, shift) of the eval-BatchNorm necks on the two halves.  ln_to_out: out is
    [batch, width + out_dim] = [ln | ln @ proj] (the image towers), else [batch, out_dim] (the text tower); a passed `out` may
    be a view whose rows are out.stride(0) apart, with the projection at column out_col."""
    dev = _lib.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    ln_g, ln_b, proj = _dev_f32(ln_g, dev), _dev_f32(ln_b, dev), _dev_f32(proj, dev)
    width, out_dim = proj.shape
    assert tuple(ln_g.shape) == (width,) and tuple(ln_b.shape) == (width,)
    reach = (tokens if row_of is not None else 1) * width
    assert batch == 0 or (batch - 1) * int(item_stride) + reach <= x.numel(), "x is too short for the rows the head may read"
    if row_of is not None:
        row_of = row_of.to(device=dev, dtype=torch.int32).contiguous()
        assert tuple(row_of.shape) == (batch,)
    necks = []
    for neck, n in ((bn, width), (bnp, out_dim)):
        pair = [None, None] if neck is None else [_dev_f32(t, dev) for t in neck]
        assert all(t is None or tuple(t.shape) == (n,) for t in pair)
        necks += pair
    if out_col is None:
        out_col = width if ln_to_out else 0
    if out is None:
        out = torch.empty((batch, out_col + out_dim), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == batch
    assert out.shape[1] >= out_col + out_dim and (batch == 0 or out.stride(1) == 1)
    y = torch.empty((batch, width), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mpreid_tower_head_f32(_ptr(x), int(item_stride), _ptr(row_of), int(tokens), int(batch), width, out_dim,
                                                 _ptr(ln_g), _ptr(ln_b), _ptr(proj), *[_ptr(t) for t in necks], _ptr(y), _ptr(out),
                                                 int(out.stride(0)) if batch else out_col + out_dim, int(out_col), int(ln_to_out),
                                                 _lib.stream_ptr()), "mpreid_tower_head_f32")
    return y, out


def quickgelu_backward(u: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """QuickGELU's backward in place (mpreid_quickgelu_backward_f32): d *= s + 1.702 u s (1 - s), s = sigmoid(1.702 u); u, d fp32
    on the device with the same number of elements, a multiple of 4; d is returned."""
    _lib.require_gpu()
    for t in (u, d):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert u.numel() == d.numel()
    _lib.check(_lib.load().mpreid_quickgelu_backward_f32(_ptr(u), _ptr(d), u.numel(), _lib.stream_ptr()),
               "mpreid_quickgelu_backward_f32")
    return d


def check_eot(eot, batch: int, tokens: int) -> np.ndarray:
    """the read-out rows of a prompt batch as int32 [batch], validated on the host (the library does not look at them):
    integers with 0 <= eot < tokens, else ValueError"""
    e = eot.detach().cpu().numpy() if torch.is_tensor(eot) else np.asarray(eot)
    if e.shape != (batch,):
        raise ValueError(f"eot: expected shape ({batch},), got {e.shape}")
    if e.dtype == np.bool_ or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"eot: expected an integer type, got {e.dtype}")
    if batch and (int(e.min()) < 0 or int(e.max()) >= tokens):
        raise ValueError(f"eot: rows must lie in 0 .. {tokens - 1}, got {int(e.min())} .. {int(e.max())}")
    return np.ascontiguousarray(e, dtype=np.int32)


class TextEncoder:
    """Device-resident CLIP text transformer: prompts + positional embedding, causal residual blocks, ln_final on the
    end-of-text row, text_projection (model/make_model_uniprompt.py:49-68).  Split precision.

    cfg keys: tokens, width, layers, heads, out_dim (mpreid.synth.CLIP_TEXT layout); an optional 'precision' other than
    'split' is refused.  state_dict: CLIP's own key names, optionally prefixed 'text_encoder.', numpy or torch:
    transformer.resblocks.{l}.*, positional_embedding, ln_final.*, text_projection and, optionally, token_embedding.weight."""

    CHUNK = 512   # prompts per library call: one workspace of ~0.6 GB at CLIP's size serves any batch

    def __init__(self, cfg: dict, state_dict: dict, ws_tag: str = "text", device=None):
        if cfg.get("precision", "split") != "split":
            _text_unsupported("TextEncoder")
        self.device = dev = device or _lib.require_gpu()
        self.ws_tag = ws_tag
        self.cfg = {k: int(cfg[k]) for k in ("tokens", "width", "layers", "heads", "out_dim")}
        get = _state_getter(state_dict, "text_encoder.")
        self._get = get      # backward() builds its transposed fp32 weights from the same tensors, at its first call
        self.c_wt = None

        def f32(name, shape):
            t = get(name).to(device=dev, dtype=torch.float32).contiguous()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return t

        w, nl = self.cfg["width"], self.cfg["layers"]
        self._keep = []   # owns every device tensor referenced by the C structs
        self.c_cfg = _lib.TextCfg(self.cfg["tokens"], w, nl, self.cfg["heads"], self.cfg["out_dim"])
        layers = (_lib.VitLayer * max(nl, 1))()
        pack_src = []   # the pack kernels' fp32 sources: alive until the synchronize at the end
        for i in range(nl):
            kept, src = _fill_block(layers[i], f32, i, w, True)
            self._keep += kept
            pack_src += src
        self._layers = layers
        top = dict(pos_emb=f32("positional_embedding", (self.cfg["tokens"], w)), ln_final_g=f32("ln_final.weight", (w,)),
                   ln_final_b=f32("ln_final.bias", (w,)), proj=f32("text_projection", (w, self.cfg["out_dim"])))
        self.c_w = _lib.TextWeights()
        for k, v in top.items():
            self._keep.append(v)
            setattr(self.c_w, k, v.data_ptr())
        self.c_w.layers = C.cast(layers, C.POINTER(_lib.VitLayer))
        emb = get("token_embedding.weight", required=False)
        self.token_embedding = None if emb is None else emb.to(device=dev, dtype=torch.float32).contiguous()
        torch.cuda.current_stream().synchronize()   # the pack kernels are done with their fp32 sources

    @torch.no_grad()
    def forward(self, prompts: torch.Tensor, eot, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """prompts [B, tokens, width] (the embedded prompts, positional embedding NOT added), eot [B] integer rows ->
        fp32 [B, out_dim] on the device; at most CHUNK prompts per library call, through one workspace"""
        _lib.load()
        n_tok, w, od = self.cfg["tokens"], self.cfg["width"], self.cfg["out_dim"]
        if prompts.dim() != 3 or tuple(prompts.shape[1:]) != (n_tok, w):
            raise ValueError(f"prompts: expected [B, {n_tok}, {w}], got {tuple(prompts.shape)}")
        B = prompts.shape[0]
        e = torch.from_numpy(check_eot(eot, B, n_tok)).to(self.device)
        x = _dev_f32(prompts, self.device)
        if out is None:
            out = torch.empty((B, od), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, od)
        return self._forward_into(x, e, out)

    __call__ = forward

    def _forward_into(self, x: torch.Tensor, e: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """forward's library calls on checked device tensors (x fp32 [B, tokens, width], e int32 [B], out fp32 [B, out_dim], all
        contiguous): nothing is allocated beyond the cached workspace and nothing is copied from the host"""
        L = _lib.load()
        B = x.shape[0]
        for s in range(0, B, self.CHUNK):
            n = min(B, s + self.CHUNK) - s
            ws = _workspace(self.ws_tag, L.mpreid_text_workspace_bytes(C.byref(self.c_cfg), n), self.device)
            _lib.check(L.mpreid_text_forward(C.byref(self.c_cfg), C.byref(self.c_w), _ptr(x[s:]), _ptr(e[s:]), n, _ptr(out[s:]),
                                             _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_text_forward")
        return out

    def _transposed_weights(self):
        """mpreid_text_weights_t: fp32 [in][out] copies of the frozen matrices (~150 MB at CLIP's size), made once"""
        if self.c_wt is None:
            def tr(name):
                return self._get(name).to(device=self.device, dtype=torch.float32).t().contiguous()
            nl = self.cfg["layers"]
            layers = (_lib.TextLayerT * max(nl, 1))()
            keep = []
            for i in range(nl):
                b = f"transformer.resblocks.{i}."
                for field, key in (("in_proj_t", "attn.in_proj_weight"), ("out_proj_t", "attn.out_proj.weight"),
                                   ("fc_t", "mlp.c_fc.weight"), ("proj_t", "mlp.c_proj.weight")):
                    keep.append(tr(b + key))
                    setattr(layers[i], field, keep[-1].data_ptr())
            keep.append(tr("text_projection"))
            wt = _lib.TextWeightsT()
            wt.proj_t = keep[-1].data_ptr()
            wt.layers = C.cast(layers, C.POINTER(_lib.TextLayerT))
            self._keep_t = (keep, layers)
            self.c_wt = wt
        return self.c_wt

    @torch.no_grad()
    def backward(self, prompts: torch.Tensor, eot, grad_out: torch.Tensor) -> torch.Tensor:
        """d loss / d prompts, fp32 [B, tokens, width], given grad_out = d loss / d forward(prompts, eot) [B, out_dim]; the
        tower's weights are frozen (mpreid_text_backward: it re-runs the forward itself, so no earlier forward call is needed).
        At most CHUNK prompts per library call, through one workspace (tag ws_tag + "_grad")."""
        _lib.load()
        n_tok, w, od = self.cfg["tokens"], self.cfg["width"], self.cfg["out_dim"]
        if prompts.dim() != 3 or tuple(prompts.shape[1:]) != (n_tok, w):
            raise ValueError(f"prompts: expected [B, {n_tok}, {w}], got {tuple(prompts.shape)}")
        B = prompts.shape[0]
        if tuple(grad_out.shape) != (B, od):
            raise ValueError(f"grad_out: expected [{B}, {od}], got {tuple(grad_out.shape)}")
        e = torch.from_numpy(check_eot(eot, B, n_tok)).to(self.device)
        x, g = _dev_f32(prompts, self.device), _dev_f32(grad_out, self.device)
        return self._backward_into(x, e, g, torch.empty((B, n_tok, w), dtype=torch.float32, device=self.device))

    def _backward_into(self, x: torch.Tensor, e: torch.Tensor, g: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """backward's library calls on checked device tensors (as _forward_into; g fp32 [B, out_dim], out fp32 [B, tokens, width])"""
        L = _lib.load()
        B = x.shape[0]
        wt = self._transposed_weights()
        for s in range(0, B, self.CHUNK):
            n = min(B, s + self.CHUNK) - s
            ws = _workspace(self.ws_tag + "_grad", L.mpreid_text_backward_workspace_bytes(C.byref(self.c_cfg), n), self.device)
            _lib.check(L.mpreid_text_backward(C.byref(self.c_cfg), C.byref(self.c_w), C.byref(wt), _ptr(x[s:]), _ptr(e[s:]),
                                              _ptr(g[s:]), n, _ptr(out[s:]), _ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "mpreid_text_backward")
        return out

    def forward_grad(self, prompts: torch.Tensor, eot) -> torch.Tensor:
        """forward(prompts, eot) as a node of torch's autograd graph, differentiable with respect to `prompts` only: its
        backward is backward(prompts, eot, the incoming gradient)"""
        return _TextForwardGrad.apply(prompts, self, check_eot(eot, prompts.shape[0], self.cfg["tokens"]))

    def encode_tokens(self, token_ids: torch.Tensor) -> torch.Tensor:
        """model/clip/model.py:609-619: forward(token_embedding[token_ids], token_ids.argmax(-1)); the embedding gather is
        torch indexing on the device"""
        if self.token_embedding is None:
            raise ValueError("encode_tokens: the state dict had no token_embedding.weight")
        ids = torch.as_tensor(token_ids).to(self.device).long()
        if ids.dim() != 2 or ids.shape[1] != self.cfg["tokens"]:
            raise ValueError(f"token_ids: expected [B, {self.cfg['tokens']}], got {tuple(ids.shape)}")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.token_embedding.shape[0]):
            raise ValueError(f"token_ids outside the embedding table of {self.token_embedding.shape[0]} rows")
        return self.forward(self.token_embedding[ids], ids.argmax(dim=-1))


class _TextForwardGrad(torch.autograd.Function):
    """TextEncoder.forward_grad"""

    @staticmethod
    def forward(ctx, prompts, enc, eot):
        ctx.enc, ctx.eot = enc, eot
        ctx.save_for_backward(prompts)
        return enc.forward(prompts, eot)

    @staticmethod
    def backward(ctx, grad_out):
        (prompts,) = ctx.saved_tensors
        grad = ctx.enc.backward(prompts, ctx.eot, grad_out)
        return grad.to(device=prompts.device, dtype=prompts.dtype), None, None


# ----------------------------------------------------------------------------------------------
# Stage-1 prompt learning (include/mpreid.h: mpreid_supcon_pair_f32, mpreid_rows_segment_sum_f32, mpreid_adam_step_f32)
# ----------------------------------------------------------------------------------------------
def _f32_buffer(t: Optional[torch.Tensor], shape, device, what: str) -> torch.Tensor:
    """an output buffer: allocated (uninitialised) when not passed, else checked; it may be a view into a larger buffer"""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), what
    return t


def supcon_pair(img: torch.Tensor, txt: torch.Tensor, labels: torch.Tensor, need_d_img: bool = False, directions: int = 3,
                loss: Optional[torch.Tensor] = None, d_txt: Optional[torch.Tensor] = None, d_img: Optional[torch.Tensor] = None):
    """The symmetric supervised contrastive loss of stage 1 and its gradients (mpreid_supcon_pair_f32): img, txt fp32
    [B, dim], labels int64 [B] -> (loss [2] = loss_i2t, loss_t2i; d_txt [B, dim][; d_img [B, dim] with need_d_img]), the gradients
    of loss_i2t + loss_t2i, all on the device, nothing synchronised.  directions = 1 / 2: the gradients of loss_i2t / loss_t2i
    alone (mpreid_supcon_f32).  1 <= B <= SUPCON_MAX_BATCH.  The output buffers may be passed (the trainer's persistent ones)."""
    dev = _lib.require_gpu()
    L = _lib.load()
    img, txt = _dev_f32(img, dev), _dev_f32(txt, dev)
    if img.dim() != 2 or txt.shape != img.shape:
        raise ValueError(f"supcon_pair: img and txt must be [B, dim] of one shape, got {tuple(img.shape)} and {tuple(txt.shape)}")
    B, D = img.shape
    labels = _dev_i64(labels, dev)
    if tuple(labels.shape) != (B,):
        raise ValueError(f"supcon_pair: labels must be [{B}], got {tuple(labels.shape)}")
    if B < 1 or D < 1:
        raise ValueError("supcon_pair: an empty batch has no loss")
    loss = _f32_buffer(loss, (2,), dev, "loss")
    d_txt = _f32_buffer(d_txt, (B, D), dev, "d_txt")
    d_img = _f32_buffer(d_img, (B, D), dev, "d_img") if need_d_img else None
    ws = _workspace("supcon", L.mpreid_supcon_workspace_bytes(B, D), dev)
    _lib.check(L.mpreid_supcon_f32(_ptr(img), _ptr(txt), _ptr(labels), B, D, int(directions), _ptr(loss), _ptr(d_txt), _ptr(d_img),
                                   _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_supcon_pair_f32")
    return (loss, d_txt, d_img) if need_d_img else (loss, d_txt)


def check_segment_index(idx, batch: int, n_seg: int) -> None:
    """host-side validation of a segment index (the library does not look at its contents): integers in 0 .. n_seg - 1"""
    i = idx.detach().cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
    if i.shape != (batch,) or i.dtype == np.bool_ or not np.issubdtype(i.dtype, np.integer):
        raise ValueError(f"idx: expected {batch} integers, got shape {i.shape} of {i.dtype}")
    if batch and (int(i.min()) < 0 or int(i.max()) >= n_seg):
        raise ValueError(f"idx: values must lie in 0 .. {n_seg - 1}, got {int(i.min())} .. {int(i.max())}")


def rows_segment_sum(src: torch.Tensor, idx: torch.Tensor, tok0: int, n_tok: int, n_seg: int,
                     out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """out[s, t, e] = sum over b ascending with idx[b] == s of src[b, tok0 + t, e] (mpreid_rows_segment_sum_f32): the gradient of
    a context tensor ctx[idx] that fills the rows tok0 .. tok0 + n_tok - 1 of the prompts, from the prompt gradient src fp32
    [B, tokens, width]; a sequential fp32 sum in batch order, bit-reproducible.  idx int64 [B] -> fp32 [n_seg, n_tok, width].
    validate=False skips the host-side range check of idx (it reads the indices back from the device)."""
    dev = _lib.require_gpu()
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3
    B, tokens, width = src.shape
    if validate:
        check_segment_index(idx, B, n_seg)
    idx = _dev_i64(idx, dev)
    if not (0 <= tok0 and 1 <= n_tok and tok0 + n_tok <= tokens):
        raise ValueError(f"rows_segment_sum: the window {tok0} .. {tok0 + n_tok - 1} does not lie in 0 .. {tokens - 1}")
    out = _f32_buffer(out, (n_seg, n_tok, width), dev, "out")
    _lib.check(_lib.load().mpreid_rows_segment_sum_f32(_ptr(src), _ptr(idx), B, tokens, width, int(tok0), int(n_tok), int(n_seg),
                                                       _ptr(out), _lib.stream_ptr()), "mpreid_rows_segment_sum_f32")
    return out


def adam_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int, lr: float,
              betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False) -> None:
    """one step of torch.optim.Adam (decoupled False: weight decay added to the gradient) or AdamW (True) on fp32 device
    tensors of one size, in place (mpreid_adam_step_f32: the arithmetic order is in include/mpreid.h); step >= 1"""
    _lib.require_gpu()
    n = param.numel()
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    _lib.check(_lib.load().mpreid_adam_step_f32(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, int(step), float(lr),
                                                float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)),
                                                _lib.stream_ptr()), "mpreid_adam_step_f32")


class PromptAdam:
    """torch.optim.Adam / AdamW over fp32 device tensors whose step is adam_step: zero_grad, step, param_groups and state_dict as
    torch's optimizers have them (one group per entry of `params`: a tensor, or a dict with "params" and its own lr /
    weight_decay, the form solver/make_optimizer_prompt.py builds).  step() updates every parameter that has a .grad (the
    autograd path); update(p, grad) is the same step on a gradient held elsewhere (PromptTrainer's buffers).  No amsgrad."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False):
        self.decoupled = bool(decoupled)
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.param_groups = []
        for g in params:
            g = dict(g) if isinstance(g, dict) else {"params": [g]}
            g["params"] = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            self.param_groups.append(g)
        for p in self._params():
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("PromptAdam: parameters are contiguous fp32 tensors on the device")
        self.state = {}

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _group_of(self, p):
        for g in self.param_groups:
            if any(q is p for q in g["params"]):
                return g
        raise KeyError("PromptAdam: not a parameter of this optimizer")

    def zero_grad(self, set_to_none: bool = True):
        for p in self._params():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    @torch.no_grad()
    def update(self, p: torch.Tensor, grad: torch.Tensor, lr: Optional[float] = None):
        g = self._group_of(p)
        st = self.state.get(id(p))
        if st is None:
            st = self.state[id(p)] = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        st["step"] += 1
        adam_step(p.detach(), grad, st["exp_avg"], st["exp_avg_sq"], st["step"], g["lr"] if lr is None else lr, g["betas"], g["eps"],
                  g["weight_decay"], self.decoupled)

    def step(self):
        for p in self._params():
            if p.grad is not None:
                self.update(p, _dev_f32(p.grad, p.device))

    def state_dict(self):
        order = {id(p): i for i, p in enumerate(self._params())}
        groups = [dict({k: v for k, v in g.items() if k != "params"}, params=[order[id(p)] for p in g["params"]])
                  for g in self.param_groups]
        return {"state": {order[k]: {"step": v["step"], "exp_avg": v["exp_avg"].clone(), "exp_avg_sq": v["exp_avg_sq"].clone()}
                          for k, v in self.state.items()}, "param_groups": groups, "decoupled": self.decoupled}


class PromptTrainer:
    """One fused stage-1 step on the device (reference processor/processor_uniprompt_stage1.py:74-98 without autograd): assemble
    the prompts (PromptLearner.forward), TextEncoder forward, supcon_pair against the fixed image features, TextEncoder backward,
    rows_segment_sum into a persistent gradient buffer per trained context tensor, adam_step on those tensors in place -- the
    next get_text call of the model sees the new values.  stage '1a' trains ctx_generic, '1b' ctx_modality and ctx_platform (it
    needs the views: the index of each prompt's context rows).  `optimizer`: a PromptAdam over the trained tensors (made from
    the keyword settings when not given); its param_groups carry the learning rate a scheduler sets.  `eot`: the read-out row of
    the prompts, an integer or a function batch -> rows.  Not reproduced from the reference: autocast and GradScaler -- the
    text features and their gradient are fp32-grade and the backward never passes through fp16, so there is nothing to scale.
    After the first step of a batch size nothing is allocated but what torch's prompt assembly takes from its cached blocks."""

    WINDOWS = {"ctx_generic": (1, 8), "ctx_modality": (9, 4), "ctx_platform": (13, 4)}   # first prompt row, rows

    def __init__(self, text_encoder: "TextEncoder", prompt_learner, stage: str, optimizer: Optional[PromptAdam] = None, eot=19,
                 lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 5e-4, decoupled: bool = False):
        if stage not in ("1a", "1b"):
            raise ValueError(f"PromptTrainer: stage must be '1a' or '1b', got {stage!r}")
        self.enc, self.pl, self.stage, self.eot = text_encoder, prompt_learner, stage, eot
        self.names = ("ctx_generic",) if stage == "1a" else ("ctx_modality", "ctx_platform")
        n_tok, w = self.enc.cfg["tokens"], self.enc.cfg["width"]
        for name in ("ctx_generic", "ctx_modality", "ctx_platform"):
            t, (tok0, rows) = getattr(prompt_learner, name), self.WINDOWS[name]
            if t.dim() != 3 or tuple(t.shape[1:]) != (rows, w) or tok0 + rows > n_tok:
                raise ValueError(f"PromptTrainer: {name} {tuple(t.shape)} does not fill rows {tok0} .. {tok0 + rows - 1} of "
                                 f"[{n_tok}, {w}] prompts")
        trained = [getattr(prompt_learner, k) for k in self.names]
        self.optimizer = optimizer or PromptAdam(trained, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled)
        for t in trained:
            self.optimizer._group_of(t)
        self.grads = {k: torch.zeros_like(getattr(prompt_learner, k).detach()) for k in self.names}
        self._bufs = {}

    def _buffers(self, B: int):
        b = self._bufs.get(B)
        if b is None:
            dev, c = self.enc.device, self.enc.cfg
            rows = self.eot(B) if callable(self.eot) else np.full(B, int(self.eot), dtype=np.int64)
            b = self._bufs[B] = dict(
                eot=torch.from_numpy(check_eot(rows, B, c["tokens"])).to(dev),
                feats=torch.empty((B, c["out_dim"]), dtype=torch.float32, device=dev),
                d_txt=torch.empty((B, c["out_dim"]), dtype=torch.float32, device=dev),
                d_prompts=torch.empty((B, c["tokens"], c["width"]), dtype=torch.float32, device=dev),
                loss=torch.empty(2, dtype=torch.float32, device=dev))
        return b

    @torch.no_grad()
    def step(self, img_feat: torch.Tensor, labels: torch.Tensor, views: Optional[torch.Tensor] = None, lr: Optional[float] = None,
             validate: bool = False) -> torch.Tensor:
        """img_feat fp32 [B, out_dim], labels int64 [B] (and views [B] in stage 1b), all on the device -> the two losses of the
        batch BEFORE the update, a device tensor [2] that the next step of this batch size overwrites.  Nothing is synchronised.
        The labels index ctx_generic on the device: validate=True checks them (and the views) on the host first, which waits
        for the device; do_train_stage1 checks its whole label set once instead."""
        dev = self.enc.device
        if not (torch.is_tensor(img_feat) and img_feat.is_cuda and torch.is_tensor(labels) and labels.is_cuda):
            raise ValueError("PromptTrainer.step: img_feat and labels are device tensors")
        B = labels.shape[0]
        if self.pl.training_stage != self.stage:
            raise ValueError(f"PromptTrainer.step: the prompt learner assembles stage {self.pl.training_stage!r} prompts, the "
                             f"trainer was built for stage {self.stage!r}")
        if self.stage == "1b" and views is None:
            raise ValueError("PromptTrainer.step: stage 1b needs the views (the rows of ctx_modality / ctx_platform per prompt)")
        if tuple(img_feat.shape) != (B, self.enc.cfg["out_dim"]):
            raise ValueError(f"img_feat: expected [{B}, {self.enc.cfg['out_dim']}], got {tuple(img_feat.shape)}")
        labels = _dev_i64(labels, dev)
        prompts = self.pl.forward(labels, view=views if self.stage == "1b" else None, validate=validate)
        prompts = prompts.detach().to(dtype=torch.float32).contiguous()
        b = self._buffers(B)
        self.enc._forward_into(prompts, b["eot"], b["feats"])
        supcon_pair(img_feat, b["feats"], labels, loss=b["loss"], d_txt=b["d_txt"])
        self.enc._backward_into(prompts, b["eot"], b["d_txt"], b["d_prompts"])
        if self.stage == "1a":
            index = {"ctx_generic": labels}
        else:
            v = _dev_i64(views, dev)
            index = {"ctx_modality": self.pl.modality_index(v), "ctx_platform": self.pl.platform_index(v)}
        for name in self.names:
            p = getattr(self.pl, name)
            tok0, rows = self.WINDOWS[name]
            rows_segment_sum(b["d_prompts"], index[name], tok0, rows, p.shape[0], out=self.grads[name], validate=False)
            self.optimizer.update(p, self.grads[name], lr=lr)
        return b["loss"]


# ----------------------------------------------------------------------------------------------
# Stage-2 head (include/mpreid.h: mpreid_xent_rows_f32, mpreid_triplet_hard_f32, mpreid_bn1d_train_*_f32, mpreid_matmul_f32)
# ----------------------------------------------------------------------------------------------
def _i32_buffer(t: Optional[torch.Tensor], shape, device, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), what
    return t


def check_class_labels(labels, rows: int, classes: int) -> None:
    """host-side validation of class labels (the library does not look at their contents): integers in 0 .. classes - 1"""
    i = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if i.shape != (rows,) or i.dtype == np.bool_ or not np.issubdtype(i.dtype, np.integer):
        raise ValueError(f"labels: expected {rows} integers, got shape {i.shape} of {i.dtype}")
    if rows and (int(i.min()) < 0 or int(i.max()) >= classes):
        raise ValueError(f"labels: values must lie in 0 .. {classes - 1}, got {int(i.min())} .. {int(i.max())}")


def _rows_f32(t, device, what: str) -> torch.Tensor:
    """a 2-D fp32 device tensor with unit column stride (a column slice of a wider matrix is fine), copied only when it is not"""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a matrix, got {tuple(t.shape)}")
    t = t.detach().to(device=device, dtype=torch.float32)
    if t.shape[1] > 1 and t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def xent_rows(logits: torch.Tensor, labels: torch.Tensor, epsilon: float = 0.0, scale: float = 1.0, need_grad: bool = True,
              need_argmax: bool = False, validate: bool = True, loss: Optional[torch.Tensor] = None,
              row_loss: Optional[torch.Tensor] = None, d_logits: Optional[torch.Tensor] = None,
              argmax: Optional[torch.Tensor] = None):
    """Row cross-entropy with label smoothing and its gradient (mpreid_xent_rows_f32): logits fp32 [rows, classes], labels int64
    [rows] -> (loss [1] = -(scale / rows) sum_a sum_c t_ac log_softmax(logits)_ac with t_ac = (1 - epsilon) [c == y_a] +
    epsilon / classes; d_logits [rows, classes] or None; argmax int32 [rows] (lowest index of the row maximum) or None), all on the
    device, nothing synchronised.  validate=False skips the host-side range check of the labels (it reads them back)."""
    dev = _lib.require_gpu()
    logits = _rows_f32(logits, dev, "xent_rows: logits")
    rows, classes = logits.shape
    if rows < 1 or classes < 1:
        raise ValueError("xent_rows: an empty matrix has no loss")
    if validate:
        check_class_labels(labels, rows, classes)
    labels = _dev_i64(labels, dev)
    if tuple(labels.shape) != (rows,):
        raise ValueError(f"xent_rows: labels must be [{rows}], got {tuple(labels.shape)}")
    loss = _f32_buffer(loss, (1,), dev, "loss")
    row_loss = _f32_buffer(row_loss, (rows,), dev, "row_loss")
    d_logits = _f32_buffer(d_logits, (rows, classes), dev, "d_logits") if need_grad else None
    argmax = _i32_buffer(argmax, (rows,), dev, "argmax") if need_argmax else None
    _lib.check(_lib.load().mpreid_xent_rows_f32(_ptr(logits), logits.stride(0) if rows > 1 else classes, _ptr(labels), rows, classes,
                                                float(epsilon), float(scale), _ptr(loss), _ptr(row_loss), _ptr(d_logits), _ptr(argmax),
                                                _lib.stream_ptr()), "mpreid_xent_rows_f32")
    return loss, d_logits, argmax


def triplet_hard(feat: torch.Tensor, labels: torch.Tensor, margin: Optional[float] = None, hard_factor: float = 0.0,
                 scale: float = 1.0, need_grad: bool = True, loss: Optional[torch.Tensor] = None,
                 d_feat: Optional[torch.Tensor] = None):
    """The batch-hard triplet loss and its gradient (mpreid_triplet_hard_f32): feat fp32 [B, dim], labels int64 [B] (only compared
    with each other); margin None is the soft-margin form.  -> (loss [1], dist_ap [B], dist_an [B], p_idx int32 [B], n_idx int32
    [B], d_feat [B, dim] or None), on the device, nothing synchronised.  1 <= B <= TRIPLET_MAX_BATCH."""
    dev = _lib.require_gpu()
    L = _lib.load()
    feat = _dev_f32(feat, dev)
    if feat.dim() != 2 or feat.shape[0] < 1 or feat.shape[1] < 1:
        raise ValueError(f"triplet_hard: feat must be [B, dim], got {tuple(feat.shape)}")
    B, D = feat.shape
    if B > _lib.TRIPLET_MAX_BATCH:
        raise ValueError(f"triplet_hard: batch {B} above TRIPLET_MAX_BATCH = {_lib.TRIPLET_MAX_BATCH}")
    labels = _dev_i64(labels, dev)
    if tuple(labels.shape) != (B,):
        raise ValueError(f"triplet_hard: labels must be [{B}], got {tuple(labels.shape)}")
    loss = _f32_buffer(loss, (1,), dev, "loss")
    d_feat = _f32_buffer(d_feat, (B, D), dev, "d_feat") if need_grad else None
    stats = torch.empty((2, B), dtype=torch.float32, device=dev)
    idx = torch.empty((2, B), dtype=torch.int32, device=dev)
    ws = _workspace("triplet", L.mpreid_triplet_workspace_bytes(B, D), dev)
    _lib.check(L.mpreid_triplet_hard_f32(_ptr(feat), _ptr(labels), B, D, float(margin or 0.0), int(margin is None), float(hard_factor),
                                         float(scale), _ptr(loss), _ptr(stats[0]), _ptr(stats[1]), _ptr(idx[0]), _ptr(idx[1]),
                                         _ptr(d_feat), _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_triplet_hard_f32")
    return loss, stats[0], stats[1], idx[0], idx[1], d_feat


def _vec_f32(t, n: int, what: str) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n,)):
        raise ValueError(f"{what}: expected a contiguous fp32 device tensor [{n}]")
    return t.detach()


def bn1d_train(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor] = None,
               running_var: Optional[torch.Tensor] = None, momentum: float = 0.1, eps: float = 1e-5,
               y: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None, invstd: Optional[torch.Tensor] = None):
    """nn.BatchNorm1d in training mode (mpreid_bn1d_train_forward_f32): x fp32 [B, dim], B >= 2 -> (y [B, dim], the batch mean
    [dim], 1 / sqrt(biased variance + eps) [dim]); running_mean / running_var (both or neither, device tensors) are updated IN
    PLACE with the momentum and the unbiased variance"""
    dev = _lib.require_gpu()
    x = _dev_f32(x, dev)
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"bn1d_train: x must be [B, dim], got {tuple(x.shape)}")
    B, D = x.shape
    if B < 2:
        raise ValueError(f"bn1d_train: expected more than 1 value per channel when training, got a batch of {B}")
    if (running_mean is None) != (running_var is None):
        raise ValueError("bn1d_train: running_mean and running_var come together")
    w, b = _vec_f32(weight, D, "weight"), _vec_f32(bias, D, "bias")
    rm = None if running_mean is None else _vec_f32(running_mean, D, "running_mean")
    rv = None if running_var is None else _vec_f32(running_var, D, "running_var")
    y, mean, invstd = _f32_buffer(y, (B, D), dev, "y"), _f32_buffer(mean, (D,), dev, "mean"), _f32_buffer(invstd, (D,), dev, "invstd")
    _lib.check(_lib.load().mpreid_bn1d_train_forward_f32(_ptr(x), _ptr(w), _ptr(b), B, D, float(eps), float(momentum), _ptr(y), _ptr(mean),
                                                         _ptr(invstd), _ptr(rm), _ptr(rv), _lib.stream_ptr()),
               "mpreid_bn1d_train_forward_f32")
    return y, mean, invstd


def bn1d_train_backward(x: torch.Tensor, dy: torch.Tensor, weight: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                        dx_add: Optional[torch.Tensor] = None, need_dbeta: bool = True, dx: Optional[torch.Tensor] = None,
                        dweight: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None):
    """its backward pass (mpreid_bn1d_train_backward_f32) from the saved statistics -> (dx [B, dim] (+ dx_add: another gradient
    of x), dweight [dim], dbias [dim] or None)"""
    dev = _lib.require_gpu()
    x, dy = _dev_f32(x, dev), _dev_f32(dy, dev)
    if x.dim() != 2 or x.shape != dy.shape or x.shape[0] < 2:
        raise ValueError(f"bn1d_train_backward: x and dy must be [B >= 2, dim] of one shape, got {tuple(x.shape)} and {tuple(dy.shape)}")
    B, D = x.shape
    w, mean, invstd = _vec_f32(weight, D, "weight"), _vec_f32(mean, D, "mean"), _vec_f32(invstd, D, "invstd")
    if dx_add is not None:
        dx_add = _dev_f32(dx_add, dev)
        assert dx_add.shape == x.shape, "dx_add"
    dx, dweight = _f32_buffer(dx, (B, D), dev, "dx"), _f32_buffer(dweight, (D,), dev, "dweight")
    dbias = _f32_buffer(dbias, (D,), dev, "dbias") if need_dbeta else None
    _lib.check(_lib.load().mpreid_bn1d_train_backward_f32(_ptr(x), _ptr(dy), _ptr(w), _ptr(mean), _ptr(invstd), _ptr(dx_add), B, D,
                                                          _ptr(dx), _ptr(dweight), _ptr(dbias), _lib.stream_ptr()),
               "mpreid_bn1d_train_backward_f32")
    return dx, dweight, dbias


def _matmul(a, a_rs, a_cs, b, b_rs, b_cs, m, n, k, out, add=None):
    _lib.check(_lib.load().mpreid_matmul_f32(_ptr(a), a_rs, a_cs, _ptr(b), b_rs, b_cs, m, n, k, _ptr(add), _ptr(out), n,
                                             _lib.stream_ptr()), "mpreid_matmul_f32")
    return out


def _linear_operands(x, w, what: str):
    dev = _lib.require_gpu()
    x, w = _dev_f32(x, dev), _dev_f32(w, dev)
    if x.dim() != 2 or w.dim() != 2 or min(x.shape) < 1 or min(w.shape) < 1:
        raise ValueError(f"{what}: expected two non-empty matrices, got {tuple(x.shape)} and {tuple(w.shape)}")
    return dev, x, w


def linear_forward(f: torch.Tensor, weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """S = f . weight^T of a bias-free nn.Linear (mpreid_matmul_f32): f [B, D], weight [C, D] -> [B, C]; each element one fmaf
    chain over D, ascending"""
    dev, f, weight = _linear_operands(f, weight, "linear_forward")
    if f.shape[1] != weight.shape[1]:
        raise ValueError(f"linear_forward: f {tuple(f.shape)} and weight {tuple(weight.shape)} differ in width")
    (B, D), Cn = f.shape, weight.shape[0]
    return _matmul(f, D, 1, weight, D, 1, B, Cn, D, _f32_buffer(out, (B, Cn), dev, "out"))


def linear_grad_input(d_scores: torch.Tensor, weight: torch.Tensor, add: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_f = d_scores . weight (+ add): d_scores [B, C], weight [C, D] -> [B, D]; each element one fmaf chain over C, ascending"""
    dev, d_scores, weight = _linear_operands(d_scores, weight, "linear_grad_input")
    if d_scores.shape[1] != weight.shape[0]:
        raise ValueError(f"linear_grad_input: d_scores {tuple(d_scores.shape)} and weight {tuple(weight.shape)} do not match")
    (B, Cn), D = d_scores.shape, weight.shape[1]
    if add is not None:
        add = _dev_f32(add, dev)
        assert tuple(add.shape) == (B, D), "add"
    return _matmul(d_scores, Cn, 1, weight, 1, D, B, D, Cn, _f32_buffer(out, (B, D), dev, "out"), add)


def linear_grad_weight(d_scores: torch.Tensor, f: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_weight = d_scores^T . f: d_scores [B, C], f [B, D] -> [C, D]; each element one fmaf chain over B, ascending"""
    dev, d_scores, f = _linear_operands(d_scores, f, "linear_grad_weight")
    if d_scores.shape[0] != f.shape[0]:
        raise ValueError(f"linear_grad_weight: d_scores {tuple(d_scores.shape)} and f {tuple(f.shape)} differ in batch")
    (B, Cn), D = d_scores.shape, f.shape[1]
    return _matmul(d_scores, 1, Cn, f, 1, D, Cn, D, B, _f32_buffer(out, (Cn, D), dev, "out"))


class Stage2Step:
    """what Stage2Head.step returns: device tensors that the next step of the same batch size and form overwrites.  loss [1];
    id_loss, triplet_loss, i2t_loss: views of the three parts AS THEY ENTER the loss (weights applied); scores (classifier,
    classifier_proj or None) and i2t_logits (or None); d_f_last, d_f, d_f_proj; grads: parameter name -> gradient;
    acc: (i2t_logits.max(1)[1] == target).float().mean() as a device scalar, or None without text features."""

    def __init__(self, parts, scores, i2t_logits, argmax, target, d_f_last, d_f, d_f_proj, grads):
        self.loss, self.id_loss, self.triplet_loss, self.i2t_loss = parts[0:1], parts[1], parts[2], parts[3]
        self.scores, self.i2t_logits, self.i2t_argmax, self._target = scores, i2t_logits, argmax, target
        self.d_f_last, self.d_f, self.d_f_proj, self.grads = d_f_last, d_f, d_f_proj, grads
        self.aux_loss = None   # an MoE tower's load-balancing loss [1] (Stage2Trainer.step sets it)

    @property
    def acc(self):
        return None if self.i2t_argmax is None else (self.i2t_argmax == self._target).float().mean()


class Stage2Head:
    """The stage-2 head as one fused step on the device, without autograd (reference model/make_model.py:98-112 in training
    mode, loss/make_loss.py, processor/processor_uniprompt_stage2.py:114-119): BNNeck in training mode, the two bias-free
    classifiers, the label-smoothed identity loss, the batch-hard triplet loss, the image-to-text loss, and the gradients with
    respect to the three features and the head's parameters.  The launch counts are in csrc/stage2_head.hip.

    classifier / classifier_proj: the weights [classes, width] / [classes, width_proj]; bottleneck / bottleneck_proj: dicts (or
    modules) with weight, bias, running_mean, running_var and num_batches_tracked; all fp32 on the device, used IN PLACE.
    epsilon None: plain cross-entropy (MODEL.IF_LABELSMOOTH off); margin None: the soft-margin triplet loss (MODEL.NO_MARGIN).
    on_update: called after a step has changed the running statistics (the model invalidates its folded encoder)."""

    FORMS = ("uniprompt", "list")
    PARAMS = ("classifier.weight", "classifier_proj.weight", "bottleneck.weight", "bottleneck.bias", "bottleneck_proj.weight",
              "bottleneck_proj.bias")

    def __init__(self, classifier: torch.Tensor, classifier_proj: torch.Tensor, bottleneck, bottleneck_proj,
                 id_weight: float = 1.0, triplet_weight: float = 1.0, i2t_weight: float = 1.0, epsilon: Optional[float] = 0.1,
                 margin: Optional[float] = 0.3, momentum: float = 0.1, bn_eps: float = 1e-5, on_update=None):
        self.device = _lib.require_gpu()

        def get(src, k):
            return src[k] if isinstance(src, dict) else getattr(src, k)
        self.C, self.D = classifier.shape
        self.Dp = classifier_proj.shape[1]
        if classifier_proj.shape[0] != self.C:
            raise ValueError("Stage2Head: the two classifiers differ in their number of classes")
        self.params = {"classifier.weight": classifier, "classifier_proj.weight": classifier_proj}
        self.bn = {}
        for name, src, n in (("bottleneck", bottleneck, self.D), ("bottleneck_proj", bottleneck_proj, self.Dp)):
            self.params[name + ".weight"], self.params[name + ".bias"] = get(src, "weight"), get(src, "bias")
            self.bn[name] = (get(src, "running_mean"), get(src, "running_var"), get(src, "num_batches_tracked"))
            for t in (self.params[name + ".weight"], self.params[name + ".bias"]) + self.bn[name][:2]:
                _vec_f32(t, n, "Stage2Head: " + name)
        for k in ("classifier.weight", "classifier_proj.weight"):
            t = self.params[k]
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"Stage2Head: {k} is a contiguous fp32 tensor on the device")
        self.id_weight, self.triplet_weight, self.i2t_weight = float(id_weight), float(triplet_weight), float(i2t_weight)
        self.epsilon = 0.0 if epsilon is None else float(epsilon)
        self.margin, self.momentum, self.bn_eps, self.on_update = margin, float(momentum), float(bn_eps), on_update
        self._bufs = {}

    def _buffers(self, B: int, T: int, form: str):
        key = (B, T, form)
        b = self._bufs.get(key)
        if b is None:
            dev = self.device

            def e(*shape):
                return torch.empty(shape, dtype=torch.float32, device=dev)
            b = self._bufs[key] = dict(terms=e(8), parts=e(4), row_loss=e(B), tri_stats=e(2, B),
                                       tri_idx=torch.empty((2, B), dtype=torch.int32, device=dev))
            branches = (("", self.D),) if form == "uniprompt" else (("", self.D), ("_proj", self.Dp))
            for s, n in branches:
                b.update({"y" + s: e(B, n), "mean" + s: e(n), "invstd" + s: e(n), "S" + s: e(B, self.C), "dS" + s: e(B, self.C),
                          "dy" + s: e(B, n), "d_tri" + s: e(B, n)})
            # gradients: in the Uni-Prompt form nothing ever writes those of the unused branch -- they stay the exact zeros of here
            z = torch.zeros
            b["grads"] = {"classifier.weight": e(self.C, self.D), "bottleneck.weight": e(self.D), "bottleneck.bias": e(self.D)}
            if form == "uniprompt":
                b["grads"].update({"classifier_proj.weight": z((self.C, self.Dp), device=dev), "bottleneck_proj.weight": z(self.Dp, device=dev),
                                   "bottleneck_proj.bias": z(self.Dp, device=dev)})
                b["d_f_last"] = z((B, self.D), device=dev)
            else:
                b["grads"].update({"classifier_proj.weight": e(self.C, self.Dp), "bottleneck_proj.weight": e(self.Dp),
                                   "bottleneck_proj.bias": e(self.Dp)})
                b["d_f_last"], b["d_add_proj"] = e(B, self.D), e(B, self.Dp)
            b["d_f"], b["d_f_proj"] = e(B, self.D), (e(B, self.Dp) if (T or form == "list") else z((B, self.Dp), device=dev))
            if T:
                b.update(i2t=e(B, T), d_i2t=e(B, T), argmax=torch.empty(B, dtype=torch.int32, device=dev))
        return b

    def _triplet(self, b, feat, target, term, d_feat):
        L = _lib.load()
        B, D = feat.shape
        ws = _workspace("triplet", L.mpreid_triplet_workspace_bytes(B, D), self.device)
        st, ix = b["tri_stats"], b["tri_idx"]
        _lib.check(L.mpreid_triplet_hard_f32(_ptr(feat), _ptr(target), B, D, float(self.margin or 0.0), int(self.margin is None), 0.0,
                                             self.triplet_weight, _ptr(term), _ptr(st[0]), _ptr(st[1]), _ptr(ix[0]), _ptr(ix[1]),
                                             _ptr(d_feat), _ptr(ws), ws.numel(), _lib.stream_ptr()), "mpreid_triplet_hard_f32")

    def _identity(self, b, s, name, f, target, term, dx_add, d_f):
        """one identity branch: BNNeck, classifier, loss, and back; the feature gradient takes dx_add along"""
        w, beta = self.params[name + ".weight"].detach(), self.params[name + ".bias"].detach()
        W = self.params["classifier" + s + ".weight"].detach()
        rm, rv, nbt = self.bn[name]
        g = b["grads"]
        bn1d_train(f, w, beta, rm, rv, self.momentum, self.bn_eps, y=b["y" + s], mean=b["mean" + s], invstd=b["invstd" + s])
        nbt.add_(1)
        linear_forward(b["y" + s], W, out=b["S" + s])
        xent_rows(b["S" + s], target, self.epsilon, self.id_weight, validate=False, loss=term, row_loss=b["row_loss"],
                  d_logits=b["dS" + s])
        linear_grad_input(b["dS" + s], W, out=b["dy" + s])
        linear_grad_weight(b["dS" + s], b["y" + s], out=g["classifier" + s + ".weight"])
        bn1d_train_backward(f, b["dy" + s], w, b["mean" + s], b["invstd" + s], dx_add=dx_add, dx=d_f, dweight=g[name + ".weight"],
                            dbias=g[name + ".bias"])

    @torch.no_grad()
    def step(self, f_last: torch.Tensor, f: torch.Tensor, f_proj: torch.Tensor, target: torch.Tensor,
             text_features: Optional[torch.Tensor] = None, form: str = "uniprompt", write_grad: bool = False,
             validate: bool = False) -> Stage2Step:
        """f_last, f fp32 [B, width], f_proj fp32 [B, width_proj] (the tower's three features: model/make_model.py:98-100),
        target int64 [B], text_features fp32 [T, width_proj] (held constant), all on the device.
        form 'uniprompt': identity loss on classifier(bottleneck(f)), triplet loss on f, image-to-text loss on f_proj .
        text_features^T (it needs them); classifier_proj, bottleneck_proj and f_last receive exact zeros.
        form 'list': make_loss over [score, score_proj] and [f_last, f, f_proj], plus the image-to-text loss when text_features
        are given.  write_grad: the parameter gradients also become the parameters' .grad (clones).
        The labels select a class on the device: validate=True checks them on the host first, which waits for the device."""
        if form not in self.FORMS:
            raise ValueError(f"Stage2Head.step: form must be one of {self.FORMS}, got {form!r}")
        for t, n, what in ((f_last, self.D, "f_last"), (f, self.D, "f"), (f_proj, self.Dp, "f_proj")):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == n
                    and t.shape[0] == f.shape[0]):
                raise ValueError(f"Stage2Head.step: {what} is an fp32 device tensor [B, {n}]")
        B = f.shape[0]
        if B < 2 or B > _lib.TRIPLET_MAX_BATCH:
            raise ValueError(f"Stage2Head.step: 2 <= batch <= {_lib.TRIPLET_MAX_BATCH}, got {B}")
        if form == "uniprompt" and text_features is None:
            raise ValueError("Stage2Head.step: the Uni-Prompt form needs the text features")
        T = 0
        if text_features is not None:
            text_features = _dev_f32(text_features, self.device)
            if text_features.dim() != 2 or text_features.shape[1] != self.Dp or text_features.shape[0] < 1:
                raise ValueError(f"Stage2Head.step: text_features must be [T, {self.Dp}], got {tuple(text_features.shape)}")
            T = text_features.shape[0]
        if validate:
            check_class_labels(target, B, min(self.C, T) if T else self.C)
        target = _dev_i64(target, self.device)
        if tuple(target.shape) != (B,):
            raise ValueError(f"Stage2Head.step: target must be [{B}], got {tuple(target.shape)}")
        f_last, f, f_proj = (t.detach().contiguous() for t in (f_last, f, f_proj))
        b = self._buffers(B, T, form)
        terms = b["terms"]
        if form == "uniprompt":
            n_id, n_tri = 1, 1
            self._triplet(b, f, target, terms[1:2], b["d_tri"])
            self._identity(b, "", "bottleneck", f, target, terms[0:1], b["d_tri"], b["d_f"])
            add_proj, scores = None, (b["S"], None)
        else:
            n_id, n_tri = 2, 3
            self._triplet(b, f_last, target, terms[2:3], b["d_f_last"])
            self._triplet(b, f, target, terms[3:4], b["d_tri"])
            self._triplet(b, f_proj, target, terms[4:5], b["d_tri_proj"])
            self._identity(b, "", "bottleneck", f, target, terms[0:1], b["d_tri"], b["d_f"])
            add_proj, scores = b["d_tri_proj"], (b["S"], b["S_proj"])
        if T:
            term = terms[n_id + n_tri:n_id + n_tri + 1]
            linear_forward(f_proj, text_features, out=b["i2t"])
            xent_rows(b["i2t"], target, self.epsilon, self.i2t_weight, need_argmax=True, validate=False, loss=term,
                      row_loss=b["row_loss"], d_logits=b["d_i2t"], argmax=b["argmax"])
            # d_f_proj in the Uni-Prompt form; in the list form what the BatchNorm backward of the projected branch takes along
            linear_grad_input(b["d_i2t"], text_features, add=add_proj, out=b["d_f_proj"] if form == "uniprompt" else b["d_add_proj"])
            add_proj = b.get("d_add_proj")
        if form == "list":
            self._identity(b, "_proj", "bottleneck_proj", f_proj, target, terms[1:2], add_proj, b["d_f_proj"])
        _lib.check(_lib.load().mpreid_stage2_total_f32(_ptr(terms), n_id, n_tri, 1 if T else 0, _ptr(b["parts"]), _lib.stream_ptr()),
                   "mpreid_stage2_total_f32")
        if write_grad:
            for k, g in b["grads"].items():
                self.params[k].grad = g.clone()
        if self.on_update is not None:
            self.on_update()
        return Stage2Step(b["parts"], scores, b.get("i2t"), b.get("argmax"), target, b["d_f_last"], b["d_f"], b["d_f_proj"], b["grads"])


# ----------------------------------------------------------------------------------------------
# Stage-2 training (include/mpreid.h: mpreid_optim_step_multi_f32, mpreid_absmax_multi_f32)
# ----------------------------------------------------------------------------------------------
OPTIM_ALGOS = {"SGD": _lib.OPTIM_SGD, "Adam": _lib.OPTIM_ADAM, "AdamW": _lib.OPTIM_ADAMW}


class OptimTable:
    """The HOST table of mpreid_optim_step_multi_f32 over fp32 device tensors: entries = [(param, grad, state1, state2 or None,
    class index)], each tensor contiguous and of the parameter's size.  The table keeps the tensors alive; set_classes rewrites
    the class indices in place."""

    def __init__(self, entries):
        entries = list(entries)
        if not entries:
            raise ValueError("OptimTable: an empty table")
        self.c = (_lib.OptimEntry * len(entries))()
        self.keep = entries
        for e, (p, g, s1, s2, cls) in zip(self.c, entries):
            n = p.numel()
            for t in (p, g, s1) + (() if s2 is None else (s2,)):
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                    raise ValueError("OptimTable: every buffer of an entry is a contiguous fp32 device tensor of the parameter's size")
            e.param, e.grad, e.state1, e.state2 = p.data_ptr(), g.data_ptr(), s1.data_ptr(), None if s2 is None else s2.data_ptr()
            e.n, e.hyper = n, int(cls)

    def __len__(self):
        return len(self.c)

    def set_classes(self, classes):
        for e, c in zip(self.c, classes):
            e.hyper = int(c)


def optim_step_launches(n_tensors: int) -> int:
    """the number of kernel launches of one optim_step_multi call over n_tensors tensors (needs no device)"""
    return int(_lib.load().mpreid_optim_step_launches(int(n_tensors)))


def optim_step_multi(table: OptimTable, classes, algo: str, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
                     momentum: float = 0.0) -> None:
    """One optimizer step over every tensor of `table`, in place (mpreid_optim_step_multi_f32): algo 'SGD' (momentum, torch's
    form), 'Adam' (weight decay added to the gradient) or 'AdamW'; classes = [(lr, weight_decay)], at most OPTIM_MAX_CLASSES,
    indexed by the entries; step >= 1.  Adam / AdamW leave every tensor bit-identical to adam_step on it.  A few launches for
    the whole table (optim_step_launches), nothing synchronised."""
    _lib.require_gpu()
    if algo not in OPTIM_ALGOS:
        raise ValueError(f"optim_step_multi: algo must be one of {sorted(OPTIM_ALGOS)}, got {algo!r}")
    cls = (_lib.OptimClass * len(classes))(*[_lib.OptimClass(float(lr), float(wd)) for lr, wd in classes])
    _lib.check(_lib.load().mpreid_optim_step_multi_f32(table.c, len(table), cls, len(classes), OPTIM_ALGOS[algo], int(step),
                                                       float(betas[0]), float(betas[1]), float(eps), float(momentum),
                                                       _lib.stream_ptr()), "mpreid_optim_step_multi_f32")


def absmax_multi(tensors, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = the largest finite |entry| of tensors[i] (NaN and +-Inf count as 0: torch.nan_to_num(t, 0, 0, 0).abs().max()) for
    a list of contiguous fp32 device tensors, by one mpreid_absmax_multi_f32 call -> fp32 [len(tensors)] on the device; nothing
    is synchronised"""
    dev = _lib.require_gpu()
    tensors = list(tensors)
    if not tensors:
        raise ValueError("absmax_multi: an empty list")
    tab = (_lib.AbsmaxEntry * len(tensors))()
    for e, t in zip(tab, tensors):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= 1):
            raise ValueError("absmax_multi: contiguous non-empty fp32 device tensors")
        e.src, e.n = t.data_ptr(), t.numel()
    L = _lib.load()
    out = _f32_buffer(out, (len(tensors),), dev, "out")
    ws = _workspace("absmax", L.mpreid_absmax_multi_workspace_bytes(tab, len(tensors)), dev)
    _lib.check(L.mpreid_absmax_multi_f32(tab, len(tensors), _ptr(out), _ptr(ws), ws.numel(), _lib.stream_ptr()),
               "mpreid_absmax_multi_f32")
    return out


class TensorOptimizer:
    """torch.optim.SGD (momentum, no dampening, no Nesterov) / Adam / AdamW over fp32 device tensors whose step is ONE
    optim_step_multi call over all of them: param_groups (one group per entry of `params`: a tensor, or a dict with "params" and
    its own lr / weight_decay, the form solver/make_optimizer_prompt.py builds), zero_grad, step, state_dict and load_state_dict
    in the shape of torch's optimizers.  bind(param, grad_buffer) fixes the buffer a parameter's step reads its gradient from
    (a trainer's persistent buffers: the table is then built once); a parameter bound to no buffer is stepped from its .grad,
    and skipped -- no state, no weight decay -- when it has none, as in torch.  betas, eps and momentum are the optimizer's;
    lr and weight_decay are per group (at most OPTIM_MAX_CLASSES distinct pairs go into one call, more are split over calls).
    No amsgrad, dampening or Nesterov momentum."""

    def __init__(self, params, algo: str = "Adam", lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.0,
                 weight_decay: float = 0.0):
        if algo not in OPTIM_ALGOS:
            raise ValueError(f"TensorOptimizer: algo must be one of {sorted(OPTIM_ALGOS)}, got {algo!r}")
        self.algo = algo
        self.defaults = dict(lr=lr, weight_decay=weight_decay)
        self.defaults.update(dict(momentum=momentum) if algo == "SGD" else dict(betas=tuple(betas), eps=eps))
        self.param_groups = []
        for g in params:
            g = dict(g) if isinstance(g, dict) else {"params": [g]}
            g["params"] = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            self.param_groups.append(g)
        seen = set()
        for p in self._params():
            if not (torch.is_tensor(p) and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("TensorOptimizer: parameters are contiguous fp32 tensors (on the device by the first step)")
            if id(p) in seen:
                raise ValueError("TensorOptimizer: a parameter appears in more than one group")
            seen.add(id(p))
        self.state = {}
        self._bound = {}
        self._table = None   # (key, OptimTable, class indices) of the last step

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def zero_grad(self, set_to_none: bool = True):
        """the parameters' .grad, as torch does; a bound buffer is its owner's to overwrite"""
        for p in self._params():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def bind(self, param: torch.Tensor, grad_buffer: Optional[torch.Tensor]):
        """the step of `param` reads `grad_buffer` (contiguous fp32, on the device, of the parameter's size) from now on;
        None unbinds"""
        if not any(q is param for q in self._params()):
            raise KeyError("TensorOptimizer.bind: not a parameter of this optimizer")
        if grad_buffer is None:
            self._bound.pop(id(param), None)
        else:
            g = grad_buffer
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == param.numel()):
                raise ValueError("TensorOptimizer.bind: the gradient buffer is a contiguous fp32 device tensor of the parameter's size")
            self._bound[id(param)] = g
        self._table = None

    def _state_of(self, p):
        st = self.state.get(id(p))
        if st is None:
            if self.algo == "SGD":
                st = {"step": 0, "momentum_buffer": torch.zeros_like(p, requires_grad=False)}
            else:
                st = {"step": 0, "exp_avg": torch.zeros_like(p, requires_grad=False),
                      "exp_avg_sq": torch.zeros_like(p, requires_grad=False)}
            self.state[id(p)] = st
        return st

    @torch.no_grad()
    def step(self):
        rows = []   # (param, grad, group)
        for g in self.param_groups:
            for k in ("betas", "eps", "momentum"):
                if k in self.defaults and g[k] != self.defaults[k]:
                    raise ValueError(f"TensorOptimizer: {k} is the optimizer's, not a group's")
            for p in g["params"]:
                grad = self._bound.get(id(p))
                if grad is None and p.grad is not None:
                    grad = _dev_f32(p.grad, p.device)
                if grad is not None:
                    rows.append((p, grad, g))
        if not rows:
            return
        if not all(p.is_cuda for p, _, _ in rows):
            raise RuntimeError("TensorOptimizer.step: the parameters are not on the device; there is no CPU fallback")
        # the calls: rows of one step number, at most OPTIM_MAX_CLASSES (lr, weight_decay) pairs each -- one call in a loop
        # whose parameters step together and whose groups collapse to the reference's weights / biases / large-FC
        calls = {}
        for p, grad, g in rows:
            st = self._state_of(p)
            st["step"] += 1
            pair = (float(g["lr"]), float(g["weight_decay"]))
            for (step, part), c in calls.items():
                if step == st["step"] and (pair in c["classes"] or len(c["classes"]) < _lib.OPTIM_MAX_CLASSES):
                    break
            else:
                c = calls[(st["step"], len(calls))] = {"classes": [], "rows": [], "cls": []}
            if pair not in c["classes"]:
                c["classes"].append(pair)
            c["rows"].append((p, grad, st))
            c["cls"].append(c["classes"].index(pair))
        key = tuple((id(p), grad.data_ptr()) for c in calls.values() for p, grad, _ in c["rows"])
        if self._table is None or self._table[0] != key:
            tables = []
            for c in calls.values():
                sk = ("momentum_buffer", None) if self.algo == "SGD" else ("exp_avg", "exp_avg_sq")
                tables.append(OptimTable([(p.detach(), grad, st[sk[0]], st[sk[1]] if sk[1] else None, k)
                                          for (p, grad, st), k in zip(c["rows"], c["cls"])]))
            self._table = (key, tables)
        d = self.defaults
        for ((step, _), c), table in zip(calls.items(), self._table[1]):
            table.set_classes(c["cls"])
            optim_step_multi(table, c["classes"], self.algo, step, d.get("betas", (0.9, 0.999)), d.get("eps", 1e-8),
                             d.get("momentum", 0.0))

    def state_dict(self):
        order = {id(p): i for i, p in enumerate(self._params())}
        groups = [dict({k: v for k, v in g.items() if k != "params"}, params=[order[id(p)] for p in g["params"]])
                  for g in self.param_groups]
        return {"state": {order[k]: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in v.items()}
                          for k, v in self.state.items() if k in order}, "param_groups": groups, "algo": self.algo}

    def load_state_dict(self, sd):
        if sd.get("algo", self.algo) != self.algo:
            raise ValueError(f"TensorOptimizer.load_state_dict: a state of {sd['algo']!r} for an optimizer of {self.algo!r}")
        params = self._params()
        if len(sd["param_groups"]) != len(self.param_groups) or any(
                len(a["params"]) != len(b["params"]) for a, b in zip(sd["param_groups"], self.param_groups)):
            raise ValueError("TensorOptimizer.load_state_dict: the parameter groups do not match")
        for mine, theirs in zip(self.param_groups, sd["param_groups"]):
            mine.update({k: v for k, v in theirs.items() if k != "params"})
        self.state = {}
        for i, v in sd["state"].items():
            p = params[int(i)]
            self.state[id(p)] = {n: (t.detach().to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous().clone()
                                     if torch.is_tensor(t) else int(t)) for n, t in v.items()}
        self._table = None


class Stage2Trainer:
    """One fused stage-2 step on the device (reference processor/processor_uniprompt_stage2.py:88-135 without autograd):
    VitEncoder.forward_train, Stage2Head.step in the Uni-Prompt form, VitEncoder.backward into persistent gradient buffers, the
    gradient of the SIE table, ONE TensorOptimizer.step over every bound tensor, VitEncoder.sync_weights_batched -- all enqueued
    without a wait except the one of the re-pack.
    encoder: a VitEncoder after enable_training (the dense tower in the split precision; anything else is the encoder's
    NotImplementedError); head: the Stage2Head over the same model's parameters; optimizer: a TensorOptimizer.  Of the
    optimizer's parameters the trainer binds those it computes a gradient for: the encoder's masters, classifier.weight,
    bottleneck.weight / .bias, and cv_table.  classifier_proj.weight, bottleneck_proj.weight / .bias and anything else are NEVER
    bound: the reference's loss leaves cls_score_proj out, they have no .grad there, and torch skips them -- no update and no
    weight decay (the head's exact zeros for them would decay them under coupled Adam).  bottleneck_proj still runs in training
    mode in the reference's forward, so its running statistics move: one bn1d_train forward on f_proj does the same here.
    cv_table: the SIE table cv_embed [rows, width] (the encoder's cv_emb is sie_coe * cv_table[cv_index]); its gradient is
    sie_coe * the rows of d cv_emb summed per table row in batch order (rows_segment_sum with a window of one token).
    Not reproduced: autocast and GradScaler (the features and gradients are fp32-grade, nothing to scale).
    An MoE encoder: the step differentiates loss + aux_coef * l_aux (l_aux: the load-balancing loss of block 0's router logits,
    processor_uniprompt_stage2.py:121-128 with the documented one-layer contract) and reports that sum in Stage2Step.loss, with
    l_aux itself in Stage2Step.aux_loss; block 0's gate.weight is a master like any other and joins the optimizer's table; the
    experts and the later gates are no masters, so nothing touches them.  aux_coef: default 0.01 for an MoE tower, ignored
    for a dense one."""

    HEAD_BOUND = ("classifier.weight", "bottleneck.weight", "bottleneck.bias")

    def __init__(self, encoder: "VitEncoder", head: Stage2Head, optimizer: TensorOptimizer, text_features: torch.Tensor,
                 cv_table: Optional[torch.Tensor] = None, sie_coe: float = 3.0, pixel_mean=(0.5, 0.5, 0.5),
                 pixel_std=(0.5, 0.5, 0.5), aux_coef: Optional[float] = None):
        if not isinstance(encoder, VitEncoder):
            raise NotImplementedError("Stage2Trainer: the ViT tower in the split precision only (no RN50 tower)")
        self.moe = encoder.c_moe is not None
        self.aux_coef = (0.01 if aux_coef is None else float(aux_coef)) if self.moe else 0.0
        encoder._check_trainable("Stage2Trainer")
        if encoder.masters is None:
            raise RuntimeError("Stage2Trainer: call encoder.enable_training() first")
        if not isinstance(optimizer, TensorOptimizer):
            raise TypeError("Stage2Trainer: the optimizer is a TensorOptimizer (any other optimizer takes the autograd path)")
        self.enc, self.head, self.optimizer = encoder, head, optimizer
        self.text_features = _dev_f32(text_features, encoder.device)
        self.cv_table, self.sie_coe = cv_table, float(sie_coe)
        self.pixel_mean, self.pixel_std = tuple(pixel_mean), tuple(pixel_std)
        mine = {id(p) for p in optimizer._params()}
        self.grads = {}      # encoder key | "cv_embed" -> the persistent gradient buffer
        for key, m in encoder.masters.items():
            if id(m) in mine:
                self.grads[key] = torch.zeros_like(m, requires_grad=False)
                optimizer.bind(m, self.grads[key])
        self._want = list(self.grads)
        self._head_bound = [k for k in self.HEAD_BOUND if id(head.params[k]) in mine]
        self._cv_trained = cv_table is not None and id(cv_table) in mine
        if cv_table is not None:
            w = encoder.cfg["width"]
            if not (cv_table.is_cuda and cv_table.dtype == torch.float32 and cv_table.is_contiguous() and cv_table.dim() == 2
                    and cv_table.shape[1] == w):
                raise ValueError(f"Stage2Trainer: cv_table is a contiguous fp32 device tensor [rows, {w}]")
            if self._cv_trained:
                self.grads["cv_embed"] = torch.zeros_like(cv_table, requires_grad=False)
                optimizer.bind(cv_table, self.grads["cv_embed"])
                self._seg = torch.empty((cv_table.shape[0], 1, w), dtype=torch.float32, device=encoder.device)
        self._bufs = {}
        self._head_batch = None

    def _buffers(self, B: int):
        b = self._bufs.get(B)
        if b is None:
            dev, Dp = self.enc.device, self.head.Dp
            b = self._bufs[B] = dict(y=torch.empty((B, Dp), dtype=torch.float32, device=dev),
                                     mean=torch.empty(Dp, dtype=torch.float32, device=dev),
                                     invstd=torch.empty(Dp, dtype=torch.float32, device=dev))
            if self._cv_trained:
                b["d_cv"] = torch.empty((B, 1, self.enc.cfg["width"]), dtype=torch.float32, device=dev)
        return b

    @torch.no_grad()
    def step(self, img: torch.Tensor, target: torch.Tensor, cv_index: Optional[torch.Tensor] = None,
             validate: bool = False) -> Stage2Step:
        """img fp32 [B, 3, H, W] or uint8 [B, H, W, 3], target int64 [B], cv_index int64 [B] (rows of cv_table; needed exactly
        when the trainer has one) -> the Stage2Step of the batch BEFORE the update: device tensors the next step overwrites.
        The labels and the SIE indices address tables on the device: validate=True checks them on the host first, which
        waits for the device; a loop checks its whole label set once instead."""
        enc, head = self.enc, self.head
        if (cv_index is None) != (self.cv_table is None):
            raise ValueError("Stage2Trainer.step: cv_index comes exactly with a cv_table")
        B = img.shape[0]
        b = self._buffers(B)
        cv_emb = None
        if self.cv_table is not None:
            if validate:
                check_segment_index(cv_index, B, self.cv_table.shape[0])
            cv_index = _dev_i64(cv_index, enc.device)
            cv_emb = self.sie_coe * self.cv_table.detach()[cv_index]
        l_aux = None
        if self.moe:
            f_last, f, f_proj, _, l_aux = enc.forward_train(img, cv_emb, VIEW_ORIGINAL, self.pixel_mean, self.pixel_std,
                                                            want_router=True)
        else:
            f_last, f, f_proj = enc.forward_train(img, cv_emb, VIEW_ORIGINAL, self.pixel_mean, self.pixel_std)
        st = head.step(f_last, f, f_proj, target, self.text_features, form="uniprompt", validate=validate)
        st.aux_loss = l_aux
        if l_aux is not None:   # the loss the step reports is the one it differentiates
            st.loss.add_(l_aux, alpha=self.aux_coef)
        if self._head_batch != B:   # the head's gradient buffers are per batch size: bound once per size
            for k in self._head_bound:
                self.optimizer.bind(head.params[k], st.grads[k])
            self._head_batch = B
        # bottleneck_proj(f_proj) of the reference's training forward: nothing reads the output, the statistics move
        bp_w, bp_b = head.params["bottleneck_proj.weight"].detach(), head.params["bottleneck_proj.bias"].detach()
        rm, rv, nbt = head.bn["bottleneck_proj"]
        bn1d_train(f_proj, bp_w, bp_b, rm, rv, head.momentum, head.bn_eps, y=b["y"], mean=b["mean"], invstd=b["invstd"])
        nbt.add_(1)
        want, out = self._want, {k: self.grads[k] for k in self._want}
        if self._cv_trained:
            want, out = want + ["cv_emb"], dict(out, cv_emb=b["d_cv"].view(B, -1))
        # (d_f_last: exact zeros in the Uni-Prompt form -- a None seed is zero and costs nothing)
        # (an MoE tower's f_last is the last block's OUTPUT; its seed is exact zeros in the Uni-Prompt form all the same)
        enc.backward(img, cv_emb, None, st.d_f, st.d_f_proj, want, VIEW_ORIGINAL, self.pixel_mean, self.pixel_std, out=out,
                     aux_coef=self.aux_coef)
        if self._cv_trained:
            rows_segment_sum(b["d_cv"], cv_index, 0, 1, self.cv_table.shape[0], out=self._seg, validate=False)
            torch.mul(self._seg.view(self.cv_table.shape), self.sie_coe, out=self.grads["cv_embed"])
        self.optimizer.step()
        enc.sync_weights_batched()
        return st


def _np_getter(state_dict):
    """name -> numpy array of a ModifiedResNet state dict (keys optionally prefixed 'image_encoder.', numpy or torch)"""
    def get(name):
        for k in (name, "image_encoder." + name):
            if k in state_dict:
                v = state_dict[k]
                return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        raise KeyError(name)
    return get


def _rn50_blocks(struct, conv, width: int, layers):
    """The Bottlenecks of layer1..4 in order (model/clip/model.py:117-146) as a ctypes array of `struct`;
    conv(conv name, BatchNorm name) builds one folded convolution of the tower's kind."""
    blocks = []
    inplanes = width
    for li, (planes, nb, stride) in enumerate(zip((width, width * 2, width * 4, width * 8), layers, (1, 2, 2, 1)), 1):
        for b in range(nb):
            pre = f"layer{li}.{b}"
            blk = struct()
            blk.conv1, blk.conv2, blk.conv3 = (conv(f"{pre}.conv{i}", f"{pre}.bn{i}") for i in (1, 2, 3))
            blk.stride = stride if b == 0 else 1
            if blk.stride > 1 or inplanes != planes * 4:
                blk.down = conv(pre + ".downsample.0", pre + ".downsample.1")
            blocks.append(blk)
            inplanes = planes * 4
    return (struct * len(blocks))(*blocks)


def _fold_necks(bn: dict):
    """the eval BatchNorm necks (bottleneck over the pooled features, bottleneck_proj over the projected ones) as one
    y = x * scale + shift over the concatenated feature row: float64 (scale, shift), rounded once by the caller"""
    parts = []
    for name in ("bottleneck", "bottleneck_proj"):
        w_, b_, m_, v_ = (_np64(a) for a in bn[name])
        s_ = w_ / np.sqrt(v_ + 1e-5)
        parts.append((s_, b_ - m_ * s_))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


class Rn50Encoder:
    """Device-resident CLIP RN50 image encoder + the RN50 eval head of build_transformer.

    cfg keys: layers (4-tuple), width, heads, out_dim, h_res, w_res (mpreid.synth.RN50 layout);
    state_dict: ModifiedResNet key names (optionally prefixed 'image_encoder.'), numpy or torch;
    bn: optional dict(bottleneck=(w, b, mean, var), bottleneck_proj=(...)) applied when neck_after.
    Every BatchNorm2d is folded into its convolution here, once (fold_conv_bn); channel counts that are not
    multiples of 64 are stored zero-padded to 64 (the 32-channel stem; reduced test configurations)."""

    def __init__(self, cfg: dict, state_dict: dict, img_hw, neck_after: bool = False, bn: Optional[dict] = None,
                 device=None, ws_tag: str = "rn50", precision: str = "split"):
        """precision: 'fp16' = fp16 NHWC activations, implicit-GEMM convolutions on the fp16 matrix cores (the throughput
        path, relative feature error 2.6e-3); 'fp32' = everything fp32 on the exact fp32 matrix instruction
        (mpreid_rn50_forward_f32: ~1e-6); 'split' = fp32 activations, the convolutions of layer1-4 and the attention pool's
        k / v projections over fp16 PAIRS on the fp16 matrix cores (mpreid_rn50_forward_split: fp32-grade features -- the
        parity-grade mode that is also fast)."""
        assert precision in ("fp16", "fp32", "split"), precision
        self.tower, self.precision = "rn50", precision
        self.device = dev = device or _lib.require_gpu()
        self.ws_tag, self.cfg, self.img_hw = ws_tag, dict(cfg), tuple(img_hw)
        width, layers = cfg["width"], tuple(cfg["layers"])
        assert self.img_hw[0] // 16 == cfg["h_res"] and self.img_hw[1] // 16 == cfg["w_res"], (img_hw, cfg)
        if precision in ("fp32", "split"):
            self._init_f32(cfg, state_dict, neck_after, bn, split=precision == "split")
            return

        get = _np_getter(state_dict)

        def bn_of(prefix):
            return tuple(get(f"{prefix}.{a}") for a in ("weight", "bias", "running_mean", "running_var"))

        self._keep = []

        def conv(cname, bname):
            w = get(cname + ".weight")
            cout, cin, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            cs_in, cs_out = _pad_to(cin, 64), _pad_to(cout, 64)
            wk, bk = fold_conv_bn(w, bn_of(bname), cin_pad=cs_in)
            if wk.shape[0] < _pad_to(cs_out, 128):  # never: fold pads cout to 128 already
                raise AssertionError
            wk, bk = wk.to(dev).contiguous(), bk.to(dev).contiguous()
            self._keep += [wk, bk]
            return _lib.Rn50Conv(_ptr(wk), _ptr(bk), cs_in, cs_out, wk.shape[0], taps)

        # stem conv1 + bn1 folded, fp32, original [cout][c][kh][kw] order
        g1, b1, m1, v1 = (a.astype(np.float64) for a in bn_of("bn1"))
        sc = g1 / np.sqrt(v1 + 1e-5)
        s1w = torch.from_numpy((get("conv1.weight").astype(np.float64) * sc[:, None, None, None]).astype(np.float32)).to(dev)
        s1b = torch.from_numpy((b1 - m1 * sc).astype(np.float32)).to(dev)
        self._keep += [s1w, s1b]
        self.c_blocks = _rn50_blocks(_lib.Rn50Block, conv, width, layers)
        E, od = width * 32, cfg["out_dim"]
        self.feat_dim = E + od

        def lin(names, pad_rows=None):
            w = np.concatenate([get(f"attnpool.{n}.weight") for n in names]).astype(np.float32)
            b = np.concatenate([get(f"attnpool.{n}.bias") for n in names]).astype(np.float32)
            if pad_rows and w.shape[0] < pad_rows:
                w = np.concatenate([w, np.zeros((pad_rows - w.shape[0], w.shape[1]), np.float32)])
                b = np.concatenate([b, np.zeros(pad_rows - b.shape[0], np.float32)])
            wt, bt = torch.from_numpy(w).to(torch.float16).to(dev), torch.from_numpy(b).to(dev)
            self._keep += [wt, bt]
            return wt, bt

        vw, vb = lin(("v_proj",))
        # k_proj is used transposed (u_h = Wk_h^T q_h, see csrc/rn50.hip); its bias shifts every score of a head by the
        # same amount and cancels in the softmax
        ktw = torch.from_numpy(np.ascontiguousarray(get("attnpool.k_proj.weight").astype(np.float32).T)).to(
            torch.float16).to(dev)
        self._keep.append(ktw)
        qw, qb = lin(("q_proj",))
        cw, cb = lin(("c_proj",), pad_rows=_pad_to(od, 128))
        pos = torch.from_numpy(get("attnpool.positional_embedding").astype(np.float32)).to(dev)
        self._keep.append(pos)
        scale = shift = None
        if neck_after:
            assert bn is not None
            scale, shift = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in _fold_necks(bn))
            self._keep += [scale, shift]
        self.c_cfg = _lib.Rn50Cfg(self.img_hw[0], self.img_hw[1], width, len(self.c_blocks), cfg["heads"], od)
        self.c_w = _lib.Rn50Weights()
        self.c_w.stem1_w, self.c_w.stem1_b = _ptr(s1w), _ptr(s1b)
        self.c_w.stem2, self.c_w.stem3 = conv("conv2", "bn2"), conv("conv3", "bn3")
        self.c_w.blocks = C.cast(self.c_blocks, C.POINTER(_lib.Rn50Block))
        self.c_w.pos_emb = _ptr(pos)
        self.c_w.kt_w, self.c_w.v_w, self.c_w.v_b = _ptr(ktw), _ptr(vw), _ptr(vb)
        self.c_w.q_w, self.c_w.q_b = _ptr(qw), _ptr(qb)
        self.c_w.c_w, self.c_w.c_b = _ptr(cw), _ptr(cb)
        self.c_w.bn_scale, self.c_w.bn_shift = _ptr(scale), _ptr(shift)

    def _init_f32(self, cfg, state_dict, neck_after, bn, split=False):
        """fp32 mode: BatchNorm folded in fp64 and rounded once to fp32; real channel counts; [cout][kh][kw][cin] rows.
        split: the same folded fp32 matrices, those of layer1-4 and of k_proj / v_proj additionally as fp16 pair matrices
        [cout_pad128][hi(kseg) | lo(kseg)] of W * 2^e (mpreid_split_pack_f32; include/mpreid.h mpreid_rn50_conv_split)"""
        dev = self.device
        width, layers = cfg["width"], tuple(cfg["layers"])

        get = _np_getter(state_dict)
        self._keep = []

        def dev32(a):
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
            self._keep.append(t)
            return t

        def fold(cname, bname):
            w = get(cname + ".weight").astype(np.float64)
            g, b, m, v = (get(f"{bname}.{a}").astype(np.float64) for a in ("weight", "bias", "running_mean", "running_var"))
            sc = g / np.sqrt(v + 1e-5)
            return w * sc[:, None, None, None], b - m * sc

        def conv(cname, bname):
            w, b = fold(cname, bname)
            cout, cin, kh, kw = w.shape
            wk = dev32(w.transpose(0, 2, 3, 1).reshape(cout, kh * kw * cin))   # k order (kh, kw, c)
            return _lib.Rn50ConvF32(_ptr(wk), _ptr(dev32(b)), cin, cout, kh * kw)

        def pairs_of_(w2d, bias, cin, taps):
            conv, keep = pairs_of(w2d, bias, cin, taps, dev)
            self._keep += keep
            return conv

        def pairs_of_3x3_(w, bias):
            conv, keep = pairs_of_3x3(w, bias, dev)
            self._keep += keep
            return conv

        def conv_s(cname, bname):
            w, b = fold(cname, bname)
            cout, cin, kh, kw = w.shape
            if kh * kw == 9:
                return pairs_of_3x3_(w, b)
            return pairs_of_(w.transpose(0, 2, 3, 1).reshape(cout, kh * kw * cin), b, cin, kh * kw)

        s1w, s1b = fold("conv1", "bn1")
        self.c_blocks = _rn50_blocks(_lib.Rn50BlockF32, conv, width, layers)
        E, od = width * 32, cfg["out_dim"]
        self.feat_dim = E + od
        self.c_cfg = _lib.Rn50Cfg(self.img_hw[0], self.img_hw[1], width, len(self.c_blocks), cfg["heads"], od)
        cw = self.c_w = _lib.Rn50WeightsF32()
        if split:
            self.c_sblocks = _rn50_blocks(_lib.Rn50BlockSplit, conv_s, width, layers)
            self.c_ws = _lib.Rn50WeightsSplit()
            cw = self.c_ws.f32
            self.c_ws.blocks = C.cast(self.c_sblocks, C.POINTER(_lib.Rn50BlockSplit))
            self.c_ws.stem2, self.c_ws.stem3 = conv_s("conv2", "bn2"), conv_s("conv3", "bn3")
            for n in ("k", "v"):
                setattr(self.c_ws, n, pairs_of_(get(f"attnpool.{n}_proj.weight").astype(np.float64),
                                               get(f"attnpool.{n}_proj.bias").astype(np.float64), E, 1))
        cw.stem1_w, cw.stem1_b = _ptr(dev32(s1w)), _ptr(dev32(s1b))
        cw.stem2, cw.stem3 = conv("conv2", "bn2"), conv("conv3", "bn3")
        cw.blocks = C.cast(self.c_blocks, C.POINTER(_lib.Rn50BlockF32))
        cw.pos_emb = _ptr(dev32(get("attnpool.positional_embedding")))
        for n in ("q", "k", "v", "c"):
            setattr(cw, n + "_w", _ptr(dev32(get(f"attnpool.{n}_proj.weight"))))
            setattr(cw, n + "_b", _ptr(dev32(get(f"attnpool.{n}_proj.bias"))))
        if neck_after:
            assert bn is not None
            cw.bn_scale, cw.bn_shift = (_ptr(dev32(a)) for a in _fold_necks(bn))

    def forward(self, img: torch.Tensor, cv_emb=None, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5),
                out: Optional[torch.Tensor] = None, view: int = 0) -> torch.Tensor:
        """img: fp32 [B,3,H,W] (val_transforms applied) or uint8 [B,H,W,3] (after Resize).  cv_emb is ignored: the
        reference's RN50 branch has no SIE embedding (model/make_model.py:82-86).  view (split / fp32 towers): a
        test-time-augmentation view applied inside the stem's first convolution."""
        assert view == 0 or self.precision in ("fp32", "split"), "the fp16 tower takes materialised view tensors"
        return _forward_images(self, img, img.dtype == torch.uint8, view, None, pixel_mean, pixel_std, out)

    __call__ = forward

    def forward_u8(self, img_hwc, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5), cv_emb=None, out=None):
        return self.forward(img_hwc, None, pixel_mean, pixel_std, out)

    def forward_view(self, img, view, cv_emb=None, pixel_mean=(0.5, 0.5, 0.5), pixel_std=(0.5, 0.5, 0.5), out=None):
        """one test-time-augmentation view (VIEW_*) of fp32 [B,3,H,W] or uint8 [B,H,W,3] input, inside the stem (split / fp32)"""
        return self.forward(img, None, pixel_mean, pixel_std, out, view=int(view))
