"""Drop-in for ``processor/processor.py::do_inference`` (reference processor/processor.py:166-208).

Same loop, log lines and return value; the evaluator and the model are the HIP-backed ones.  The
reference wraps the model in nn.DataParallel when several GPUs are visible (processor/processor.py:178-182:
one process, the batch scattered over the devices).  Here multi-GPU evaluation is one process per GPU
(``python -m torch.distributed.run --nproc-per-node P test.py ...``): under WORLD_SIZE > 1 every rank runs this same
function on its own device, encodes only ITS shard of the validation set -- 1/P of the queries, then its row shard of
the gallery (mpreid.distributed.shard_range) -- and the per-rank ``R1_mAP_eval`` instances meet in ``compute()`` (one
all-gather of the query features, per-shard distance blocks, sharded ranking statistics, host concatenation on rank 0).
Every rank returns the same (Rank-1, Rank-5); rank 0 logs the results.
"""
import logging
import os

import torch

from mpreid import distributed as _D
from mpreid.pipeline import EncodePipeline
from utils.metrics import R1_mAP_eval, R1_mAP_eval_splits


class _ShardedLoader:
    """The samples [indices] of a validation loader, in order, re-batched with the loader's batch size.

    Fast paths: a loader that knows how to shard itself (``loader.shard(indices)``), and a ``torch.utils.data.DataLoader``
    (a new DataLoader over ``Subset(dataset, indices)`` with the same batch size, workers and collate function, so that
    each rank decodes only its own images).  Any other iterable is filtered: every batch is produced and the samples of
    other ranks are dropped before the model sees them."""

    def __init__(self, loader, indices):
        self.loader, self.indices = loader, list(indices)

    def __iter__(self):
        ld, idx = self.loader, self.indices
        if hasattr(ld, "shard"):
            yield from ld.shard(idx)
            return
        if isinstance(ld, torch.utils.data.DataLoader):
            sub = torch.utils.data.DataLoader(torch.utils.data.Subset(ld.dataset, idx), batch_size=ld.batch_size,
                                              shuffle=False, num_workers=ld.num_workers, collate_fn=ld.collate_fn,
                                              pin_memory=ld.pin_memory)
            yield from sub
            return
        want = set(idx)
        base = 0
        for batch in ld:
            n = len(batch[1])
            keep = [i for i in range(n) if base + i in want]
            base += n
            if keep:
                yield select_samples(batch, keep)


def select_samples(batch, keep):
    """the samples `keep` (positions inside the batch) of a loader batch (img, pids, camids, camids_t, viewids_t, paths)"""
    img, pids, camids, cam_t, view_t, paths = batch
    if len(keep) == len(pids):
        return batch
    if isinstance(img, (list, tuple)):
        img = type(img)(img[i] for i in keep)
    else:
        img = img[torch.as_tensor(keep)]
    sel = torch.as_tensor(keep)
    return (img, tuple(pids[i] for i in keep), tuple(camids[i] for i in keep), cam_t[sel], view_t[sel],
            tuple(paths[i] for i in keep))


def shard_val_loader(val_loader, num_query, n_total=None):
    """this rank's shard of a query-then-gallery validation loader: queries shard_range(num_query, rank, P) followed by
    gallery rows shard_range(n_total - num_query, rank, P); the loader itself when there is one rank"""
    rank, world = _D.rank_world()
    if world == 1:
        return val_loader
    if n_total is None:
        n_total = len(val_loader.dataset) if hasattr(val_loader, "dataset") else getattr(val_loader, "n", None)
    if n_total is None:
        raise ValueError("sharded evaluation needs the size of the validation set (loader.dataset or loader.n)")
    q_lo, q_hi = _D.shard_range(num_query, rank, world)
    g_lo, g_hi = _D.shard_range(n_total - num_query, rank, world)
    return _ShardedLoader(val_loader, list(range(q_lo, q_hi)) + list(range(num_query + g_lo, num_query + g_hi)))


#: images encoded per model call when the model does not say (``model.encode_group``).  The reference encodes one
#: loader batch (TEST.IMS_PER_BATCH = 64 in every shipped YAML) at a time; the persistent GEMMs want ~65 000 token rows
#: to fill 256 CUs without a ragged last round (22 k images/s at 64 per call, 36 k at 512), and a feature row does not
#: depend on which images share its batch (tests/test_gpu_vit.py: bit for bit), so consecutive loader batches are
#: encoded together -- cut at group boundaries, not batch boundaries -- and handed to the evaluator one loader batch at
#: a time, exactly as before.
ENCODE_GROUP = 512


def grouped_batches(val_loader, target):
    """consecutive loader batches whose image count reaches `target` (the last group may be smaller)"""
    group, n = [], 0
    for batch in val_loader:
        group.append(batch)
        n += len(batch[1])
        if n >= target:
            yield group
            group, n = [], 0
    if group:
        yield group


def merge_batches(group, device):
    """(images, camids tensor, viewids tensor) of a group of loader batches, on `device`"""
    imgs = [b[0] for b in group]
    if isinstance(imgs[0], (list, tuple)):           # decoded uint8 images: stay a flat list (RawImageBatch)
        img = type(imgs[0])(x for b in imgs for x in b)
    else:
        img = (imgs[0] if len(imgs) == 1 else torch.cat(imgs, dim=0)).to(device)
    camids = torch.cat([b[3] for b in group]).to(device)
    views = torch.cat([b[4] for b in group]).to(device)
    return img, camids, views


SAME_CAM_NOTE = ("TEST.REMOVE_SAME_CAM: for each query, gallery images of the same identity from the same camera are "
                 "removed before ranking (Market-1501 protocol)")


def _configure_evaluator(cfg, evaluator):
    """the evaluator attributes that come from config keys (shared by do_inference and do_inference_trials)"""
    # TEST.DISTANCE_MODE / TEST.RERANK_ALGO (not reference keys): arithmetic of the distance matrix -- 'exact' (default: the
    # bit-parity fp32 chain), 'split3' (fp16 matrix cores, |err| <= 1e-6), 'f16' (one pass, ~1e-4) -- and of the re-ranking
    # ('exact' | 'split3': blend-term distance rows from the fp16 matrix cores, ranks identical, outputs within 1e-6)
    from mpreid import ops as _ops
    evaluator.distance_mode = {"exact": _ops.GEMM_F32_EXACT, "split3": _ops.GEMM_F16_SPLIT3, "f16": _ops.GEMM_F16_FAST}[
        str(getattr(cfg.TEST, "DISTANCE_MODE", "exact"))]
    evaluator.rerank_algo = {"exact": _ops.RERANK_AUTO, "split3": _ops.RERANK_SPARSE_SPLIT3}[
        str(getattr(cfg.TEST, "RERANK_ALGO", "exact"))]
    # TEST.REMOVE_SAME_CAM (not a reference key): the Market-1501 protocol of utils/metrics.py, default off like upstream
    evaluator.remove_same_cam = bool(getattr(cfg.TEST, "REMOVE_SAME_CAM", False))
    # TEST.RANK_LIST_K (not a reference key): R1_mAP_eval also keeps every query's first K gallery items (last_rank_lists)
    evaluator.rank_list_k = int(getattr(cfg.TEST, "RANK_LIST_K", 0) or 0)
    configure_query_expansion(cfg, evaluator)
    configure_extra_metrics(cfg, evaluator)
    evaluator.reset()


def configure_extra_metrics(cfg, evaluator):
    """TEST.EXTRA_METRICS / ROC_FPRS / PAIR_HIST_BINS / PAIR_HIST_RANGE (not reference keys): mINP and the pair statistics
    of utils/metrics.py, default off (R1_mAP_eval_splits takes the switch alone: per-split mINP)"""
    evaluator.extra_metrics = bool(getattr(cfg.TEST, "EXTRA_METRICS", False))
    if hasattr(evaluator, "roc_fprs"):
        evaluator.roc_fprs = tuple(float(f) for f in getattr(cfg.TEST, "ROC_FPRS", (1e-4, 1e-3, 1e-2)))
        evaluator.pair_hist_bins = int(getattr(cfg.TEST, "PAIR_HIST_BINS", 0) or 0)
        evaluator.pair_hist_range = tuple(float(x) for x in getattr(cfg.TEST, "PAIR_HIST_RANGE", (0.0, 4.0)))


def write_pair_hist(path, metrics):
    """the pair-distance histograms of one evaluation (R1_mAP_eval.last_metrics) as an .npz: edges float32 [bins + 1],
    pos / neg int64 [bins + 2] (underflow, the bins (e_{b-1}, e_b], overflow), P, Nn.  Returns the file name."""
    import numpy as np
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    t = metrics["tpr_at_fpr"]
    np.savez(path, edges=metrics["pair_hist_edges"], pos=metrics["pair_hist_pos"], neg=metrics["pair_hist_neg"],
             P=np.int64(t["P"]), Nn=np.int64(t["Nn"]))
    return path


def report_extra_metrics(cfg, logger, evaluator):
    """the lines after "mAP:" when TEST.EXTRA_METRICS is on -- mINP and one TPR@FPR line per rate -- and, with OUTPUT_DIR set
    and PAIR_HIST_BINS > 0, <OUTPUT_DIR>/pair_hist.npz"""
    m = getattr(evaluator, "last_metrics", None)
    if not m:
        return
    logger.info("mINP: {:.1%}".format(m["mINP"]))
    t = m["tpr_at_fpr"]
    for f, tpr in zip(t["fprs"], t["tpr"]):
        logger.info("TPR@FPR={:.0e}: {:.1%}".format(f, tpr))
    if "pair_hist_edges" in m and cfg.OUTPUT_DIR:
        logger.info("TEST.PAIR_HIST_BINS: pair-distance histograms -> {}".format(
            write_pair_hist(os.path.join(cfg.OUTPUT_DIR, "pair_hist.npz"), m)))


def configure_query_expansion(cfg, evaluator):
    """TEST.QE_K / QE_ALPHA / QE_TIMES (not reference keys): query expansion in feature space before ranking
    (utils/metrics.py:expand_features), default off; one log line when it is on"""
    evaluator.qe_k = int(getattr(cfg.TEST, "QE_K", 0) or 0)
    evaluator.qe_alpha = float(getattr(cfg.TEST, "QE_ALPHA", 3.0))
    evaluator.qe_times = int(getattr(cfg.TEST, "QE_TIMES", 1))
    if evaluator.qe_k > 0:
        logging.getLogger("transreid.test").info(
            "TEST.QE_K: query expansion over query + gallery before ranking -- every feature becomes the mean of its first "
            "{} neighbours weighted by cosine ** {}, {} round(s)".format(evaluator.qe_k, evaluator.qe_alpha,
                                                                         evaluator.qe_times))


def rank_list_file(cfg):
    """where do_inference writes the ranked lists: TEST.RANK_LIST_FILE, else <OUTPUT_DIR>/rank_lists.npz, else '' (nowhere)"""
    name = str(getattr(cfg.TEST, "RANK_LIST_FILE", "") or "")
    if name:
        return name
    return os.path.join(cfg.OUTPUT_DIR, "rank_lists.npz") if cfg.OUTPUT_DIR else ""


def write_rank_lists(path, lists, pids, camids, paths, num_query, remove_same_cam=False, reranking=False):
    """the ranked lists of one evaluation as an .npz: `lists` = R1_mAP_eval.last_rank_lists, `pids` / `camids` / `paths`
    the evaluated images in update() order (queries first).  Arrays: indices int32 [nq, k] (gallery-relative: row numbers
    of g_pids / g_paths; -1 padded), distances float32 [nq, k] (+inf padded), counts int32 [nq], q_pids, q_camids, g_pids,
    g_camids (int64), q_paths, g_paths (str), k, remove_same_cam, reranking.  Returns the file name numpy wrote."""
    import numpy as np
    idx, val, cnt = lists
    nq = int(num_query)
    pids, camids = np.asarray(pids, dtype=np.int64), np.asarray(camids, dtype=np.int64)
    paths = np.asarray([str(x) for x in paths], dtype=str)
    assert idx.shape[0] == nq and pids.shape[0] == camids.shape[0] == paths.shape[0] >= nq
    if not path.endswith(".npz"):
        path += ".npz"   # (np.savez would append it silently)
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, indices=np.asarray(idx, dtype=np.int32), distances=np.asarray(val, dtype=np.float32),
             counts=np.asarray(cnt, dtype=np.int32), q_pids=pids[:nq], q_camids=camids[:nq], g_pids=pids[nq:],
             g_camids=camids[nq:], q_paths=paths[:nq], g_paths=paths[nq:], k=np.int64(idx.shape[1]),
             remove_same_cam=np.bool_(remove_same_cam), reranking=np.bool_(reranking))
    return path


def _encode_into(cfg, model, loader, evaluator):
    """the reference's loop body (`img = img.to(device); feat = model(img, ...); evaluator.update(...)`, :187-198) as a
    pipeline: a stager thread drains the loader into pinned group buffers and uploads them on a copy stream while
    earlier groups are encoded on two alternating streams (mpreid/pipeline.py); the evaluator sees the loader's own
    batches, in order.  MPREID_PIPELINE="stage=pinned,streams=1,slots=4" overrides the defaults (measurements).
    Returns (image paths, pipeline statistics)."""
    img_path_list = []
    opts = dict(kv.split("=", 1) for kv in os.environ.get("MPREID_PIPELINE", "").split(",") if "=" in kv)
    pipe = EncodePipeline(model, group=int(opts.get("group", getattr(model, "encode_group", ENCODE_GROUP))),
                          sie_camera=bool(cfg.MODEL.SIE_CAMERA), sie_view=bool(cfg.MODEL.SIE_VIEW),
                          streams=int(opts.get("streams", 2)), slots=int(opts.get("slots", 3)),
                          stage=opts.get("stage", "direct"))
    for feat, (_, pid, camid, _, _, imgpath) in pipe.run(loader):
        evaluator.update((feat, pid, camid))
        img_path_list.extend(imgpath)
    return img_path_list, pipe.stats


def do_inference(cfg, model, val_loader, num_query):
    device = "cuda"
    logger = logging.getLogger("transreid.test")
    logger.info("Enter inferencing")

    reranking = bool(getattr(cfg.TEST, "RE_RANKING", False))  # upstream defines the key but never reads it
    evaluator = R1_mAP_eval(num_query, max_rank=50, feat_norm=cfg.TEST.FEAT_NORM, reranking=reranking)
    _configure_evaluator(cfg, evaluator)

    # the reference's test.py never initialises a process group (test.py:39,65): under a launcher (WORLD_SIZE > 1) this
    # call does, and binds the rank to cuda:LOCAL_RANK, before anything touches a device (raises when the ranks of the
    # node cannot each see their own device -- MODEL.DEVICE_ID must list them: INTEGRATION.md section C)
    rank, world = _D.ensure_group_from_env(logger)
    if evaluator.remove_same_cam and rank == 0:
        logger.info(SAME_CAM_NOTE)
    model.to(device)
    model.eval()
    if world > 1:
        logger.info("rank {} of {}: encoding 1/{} of the queries and its gallery shard".format(rank, world, world))
        val_loader = shard_val_loader(val_loader, num_query)
    img_paths, do_inference.last_pipeline_stats = _encode_into(cfg, model, val_loader, evaluator)

    cmc, mAP, _, _, _, _, _ = evaluator.compute()
    do_inference.last_evaluator = evaluator   # (measurements: bench.py times compute() again on the same features)
    if evaluator.rank_list_k > 0:
        out = rank_list_file(cfg)
        logger.info("TEST.RANK_LIST_K: the first {} gallery images of each of the {} queries -> {}".format(
            evaluator.rank_list_k, num_query, out or "evaluator.last_rank_lists only (no RANK_LIST_FILE / OUTPUT_DIR)"))
        if out:
            write_rank_lists(out, evaluator.last_rank_lists, evaluator.pids, evaluator.camids, img_paths, num_query,
                             evaluator.remove_same_cam, reranking)
    if rank == 0:
        logger.info("Validation Results ")
        logger.info("mAP: {:.1%}".format(mAP))
        report_extra_metrics(cfg, logger, evaluator)
        for r in [1, 5, 10]:
            logger.info("CMC curve, Rank-{:<3}:{:.1%}".format(r, cmc[r - 1]))
    return cmc[0], cmc[4]


def do_inference_trials(cfg, model, pool_loader, splits):
    """The reference's VehicleID branch (test.py:46-63) with the pool encoded ONCE: `pool_loader` yields every test image
    one time, `splits` is a list of (q_idx, g_idx) index lists into it, one per trial
    (datasets.make_dataloader.vehicleid_trial_splits, or any other protocol's lists).  Same encode pipeline and config keys
    as do_inference (TEST.DISTANCE_MODE, RERANK_ALGO, REMOVE_SAME_CAM, RE_RANKING); the evaluator is R1_mAP_eval_splits.
    Logs the reference's per-trial line (its missing placeholder supplied) and its averaged line; returns
    (rank1 [S], rank5 [S], mAP [S]).  Single-process: under WORLD_SIZE > 1 the evaluator raises NotImplementedError."""
    import numpy as np
    device = "cuda"
    logger = logging.getLogger("transreid.test")
    logger.info("Enter inferencing: {} trials over one encoded pool".format(len(splits)))
    reranking = bool(getattr(cfg.TEST, "RE_RANKING", False))
    evaluator = R1_mAP_eval_splits(splits, max_rank=50, feat_norm=cfg.TEST.FEAT_NORM, reranking=reranking)
    _configure_evaluator(cfg, evaluator)
    if evaluator.remove_same_cam:
        logger.info(SAME_CAM_NOTE)
    model.to(device)
    model.eval()
    _, do_inference_trials.last_pipeline_stats = _encode_into(cfg, model, pool_loader, evaluator)
    cmcs, mAPs, _, _, _ = evaluator.compute()
    do_inference_trials.last_evaluator = evaluator
    rank1 = np.array([c[0] for c in cmcs])
    rank5 = np.array([c[min(4, len(c) - 1)] for c in cmcs])   # (a gallery of fewer than 5 items: its last rank)
    for trial in range(len(cmcs)):
        logger.info("rank_1:{:.1%}, rank_5 {:.1%}, mAP {:.1%} : trial : {}".format(rank1[trial], rank5[trial], mAPs[trial],
                                                                                  trial))
        if evaluator.last_metrics:
            logger.info("mINP: {:.1%} : trial : {}".format(evaluator.last_metrics["mINP"][trial], trial))
    n = float(len(cmcs))
    logger.info("sum_rank_1:{:.1%}, sum_rank_5 {:.1%}, sum_mAP {:.1%}".format(rank1.sum() / n, rank5.sum() / n,
                                                                              mAPs.sum() / n))
    return rank1, rank5, mAPs
