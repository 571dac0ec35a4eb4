"""The extra metrics through the evaluators and the callers: R1_mAP_eval.extra_metrics -> last_metrics (mINP, TPR at a
false-positive rate, pair-distance histograms) against the host definitions applied to the returned distmat;
R1_mAP_eval_splits per-split mINP; do_inference's log lines; test.py's pair_hist.npz.  With the option off nothing changes:
the 7-tuple is the same bytes and no new kernel is launched."""
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, NG = 60, 400


@pytest.fixture(scope="module")
def feats():
    """~60 + 400 clustered features (12 identities, 3 cameras), not normalised; one query identity is absent from the gallery"""
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((12, 48))
    pid = rng.integers(0, 12, NQ + NG)
    pid[0] = 77
    f = (centres[pid % 12] + 0.6 * rng.standard_normal((NQ + NG, 48))).astype(np.float32) * 3.0
    cam = rng.integers(0, 3, NQ + NG)
    return f, pid, cam


def _run(feats, extra, rerank, same_cam, bins=0, fprs=None):
    from utils.metrics import R1_mAP_eval
    f, pid, cam = feats
    ev = R1_mAP_eval(NQ, max_rank=50, feat_norm=True, reranking=rerank)
    ev.remove_same_cam = same_cam
    ev.extra_metrics = extra
    ev.pair_hist_bins = bins
    if fprs is not None:
        ev.roc_fprs = fprs
    ev.reset()
    for lo in range(0, NQ + NG, 128):
        ev.update((torch.from_numpy(f[lo:lo + 128]), pid[lo:lo + 128], cam[lo:lo + 128]))
    return ev, ev.compute()


def _same_bytes(a, b):
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes()
    assert np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
    assert a[2].dtype == np.float32 and a[2].tobytes() == b[2].tobytes()
    assert [int(x) for x in a[3]] == [int(x) for x in b[3]] and [int(x) for x in a[4]] == [int(x) for x in b[4]]
    assert a[5].numpy().tobytes() == b[5].numpy().tobytes() and a[6].numpy().tobytes() == b[6].numpy().tobytes()


@pytest.mark.parametrize("same_cam", [False, True])
@pytest.mark.parametrize("rerank", [False, True])
def test_last_metrics_equal_the_host_definitions(feats, rerank, same_cam, monkeypatch):
    from mpreid import _lib
    from utils import metrics
    L = _lib.load()
    launches = {"rank": 0, "pairs": 0}
    for name, key in (("mpreid_eval_rank_positions", "rank"), ("mpreid_eval_rank_positions_cam", "rank"),
                      ("mpreid_pair_bucket_counts", "pairs")):
        real = getattr(L, name)

        def counted(*a, real=real, key=key):
            launches[key] += 1
            return real(*a)
        monkeypatch.setattr(L, name, counted)
    ev_off, off = _run(feats, False, rerank, same_cam)
    assert ev_off.last_metrics is None and launches == {"rank": 1, "pairs": 0}      # off: nothing new is launched
    launches.update(rank=0, pairs=0)
    fprs = (1e-4, 1e-3, 1e-2, 0.2)
    ev, on = _run(feats, True, rerank, same_cam, bins=40, fprs=fprs)
    assert launches["rank"] == 1 and launches["pairs"] >= 2                          # ONE ranking launch
    _same_bytes(on, off)
    m = ev.last_metrics
    pids, cams = np.asarray(on[3]), np.asarray(on[4])
    labels = (pids[:NQ], pids[NQ:], cams[:NQ], cams[NQ:])
    host = metrics.eval_metrics(on[2], *labels, max_rank=50, remove_same_cam=same_cam)
    assert np.array_equal(m["cmc"], on[0]) and np.array_equal(m["cmc"], host["cmc"])
    assert m["mAP"] == on[1] and abs(m["mAP"] - host["mAP"]) < 1e-12     # (eval_func sums the dense row: eval_func_device's note)
    for k in ("all_AP", "all_INP"):
        assert m[k].dtype == np.float64 and np.array_equal(m[k], host[k]), k
    assert np.float64(m["mINP"]).tobytes() == np.float64(host["mINP"]).tobytes()
    assert np.array_equal(m["first_hit"], host["first_hit"]) and np.array_equal(m["valid"], host["valid"])
    assert not m["valid"][0] and m["valid"].sum() == m["all_INP"].size
    t, th = m["tpr_at_fpr"], metrics.tpr_at_fpr(on[2], *labels, remove_same_cam=same_cam, fprs=fprs)
    for k in ("budgets", "fprs", "tp", "fp", "tpr", "fpr"):
        assert np.array_equal(t[k], th[k]), k
    assert t["tau"].tobytes() == th["tau"].tobytes() and (t["P"], t["Nn"]) == (th["P"], th["Nn"])
    edges = np.linspace(0.0, 4.0, 41).astype(np.float32)
    assert m["pair_hist_edges"].tobytes() == edges.tobytes()
    hp, hn = metrics.pair_histograms(metrics.pair_counts(on[2], edges, *labels, remove_same_cam=same_cam))
    assert np.array_equal(m["pair_hist_pos"], hp) and np.array_equal(m["pair_hist_neg"], hn)
    assert hp.sum() == t["P"] and hn.sum() == t["Nn"] and hp.shape == (42,)
    # without bins the histograms are absent
    ev2, _ = _run(feats, True, rerank, same_cam)
    assert "pair_hist_pos" not in ev2.last_metrics and ev2.last_metrics["tpr_at_fpr"]["fprs"].tolist() == [1e-4, 1e-3, 1e-2]


def test_extra_metrics_are_single_process_and_validated_first(feats, monkeypatch):
    from mpreid import distributed as D
    from utils.metrics import R1_mAP_eval
    ev = R1_mAP_eval(NQ)
    ev.extra_metrics = True
    ev.pair_hist_bins = 5000
    ev.reset()
    with pytest.raises(ValueError):
        ev.compute()
    monkeypatch.setattr(D, "sharded_active", lambda: True)
    with pytest.raises(NotImplementedError, match="extra metrics are single-process"):
        ev.compute()


def test_splits_evaluator_reports_per_split_minp(feats):
    from utils import metrics
    f, pid, cam = feats
    rng = np.random.default_rng(3)
    n = NQ + NG
    splits = []
    for _ in range(3):
        perm = rng.permutation(n)
        splits.append((np.sort(perm[:50]), perm[50:300]))
    for same_cam in (False, True):
        ev = metrics.R1_mAP_eval_splits(splits)
        ev.remove_same_cam = same_cam
        assert ev.last_metrics is None
        ev.reset()
        ev.update((torch.from_numpy(f), pid, cam))
        off = ev.compute()
        assert ev.last_metrics is None
        ev.extra_metrics = True
        on = ev.compute()
        assert all(np.array_equal(a, b) for a, b in zip(on[0], off[0])) and on[1].tobytes() == off[1].tobytes()
        d = ev.last_dist.cpu().numpy()
        got = ev.last_metrics
        assert got["mINP"].shape == (3,) and got["mINP"].dtype == np.float64
        for i, (q, g) in enumerate(splits):
            host = metrics.eval_metrics(d[np.ix_(q, g)], pid[q], pid[g], cam[q], cam[g], remove_same_cam=same_cam)
            assert np.float64(got["mINP"][i]).tobytes() == np.float64(host["mINP"]).tobytes()
            assert np.array_equal(got["all_INP"][i], host["all_INP"])


OVERRIDES = ["DATASETS.SYNTH_QUERY", 24, "DATASETS.SYNTH_GALLERY", 72, "DATASETS.SYNTH_IDS", 6, "TEST.IMS_PER_BATCH", 32]


def test_do_inference_logs_the_new_lines(caplog):
    from config import cfg_base
    from datasets.make_dataloader import make_dataloader
    from model.make_model import make_model
    from processor.processor import do_inference
    out = {}
    for on in (False, True):
        cfg = cfg_base.clone()
        cfg.defrost()
        cfg.merge_from_list(OVERRIDES + ["TEST.EXTRA_METRICS", str(on)])
        cfg.freeze()
        _, _, val_loader, num_query, num_classes, cam_num, view_num = make_dataloader(cfg)
        model = make_model(cfg, num_class=num_classes, camera_num=cam_num, view_num=view_num)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.test"):
            out[on] = do_inference(cfg, model, val_loader, num_query)
        lines = [r.getMessage() for r in caplog.records]
        ev = do_inference.last_evaluator
        new = [x for x in lines if x.startswith("mINP: ") or x.startswith("TPR@FPR=")]
        if not on:
            assert ev.last_metrics is None and not new
            continue
        m = ev.last_metrics
        want = ["mINP: {:.1%}".format(m["mINP"])] + ["TPR@FPR={:.0e}: {:.1%}".format(f, t) for f, t in
                                                    zip((1e-4, 1e-3, 1e-2), m["tpr_at_fpr"]["tpr"])]
        assert new == want and want[1].startswith("TPR@FPR=1e-04: ")
        at = lines.index(want[0])
        assert lines[at - 1].startswith("mAP: ") and lines[at + 4].startswith("CMC curve, Rank-1")
    assert float(out[True][0]) == float(out[False][0]) and float(out[True][1]) == float(out[False][1])


def test_test_py_writes_pair_hist(tmp_path):
    spec = importlib.util.spec_from_file_location("mpreid_test_cli_extra", os.path.join(ROOT, "mp-reid_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--config_file", ""] + [str(x) for x in OVERRIDES]
    plain = cli.main(base)
    got = cli.main(base + ["TEST.EXTRA_METRICS", "True", "TEST.PAIR_HIST_BINS", "40", "OUTPUT_DIR", str(tmp_path)])
    assert float(got[0]) == float(plain[0]) and float(got[1]) == float(plain[1])
    z = np.load(os.path.join(str(tmp_path), "pair_hist.npz"))
    assert sorted(z.files) == ["Nn", "P", "edges", "neg", "pos"]
    assert z["edges"].shape == (41,) and z["pos"].shape == (42,) and z["neg"].shape == (42,)
    assert int(z["pos"].sum()) == int(z["P"]) and int(z["neg"].sum()) == int(z["Nn"])
    assert int(z["P"]) + int(z["Nn"]) == 24 * 72 and int(z["P"]) > 0
    for h in logging.getLogger("transreid").handlers[:]:      # the file handler of this run's OUTPUT_DIR
        if isinstance(h, logging.FileHandler):
            h.close()
            logging.getLogger("transreid").removeHandler(h)
