"""The stage-2 head without a GPU: the float64 restatements of tests/stage2_head_cases.py against what the reference's own loss
classes gave (tests/golden/stage2_head.npz), the drop-in modules' torch path against the same numbers, every branch of make_loss
against a composition of the restatements, the premises of the GPU cases, the workspace query and the refusals."""
import numpy as np
import pytest
import torch

import stage2_head_cases as hc
from config import cfg as _base_cfg
from loss.make_loss import CenterLoss, make_loss
from loss.softmax_loss import CrossEntropyLabelSmooth, cross_entropy
from loss.triplet_loss import TripletLoss
from mpreid import _lib, ops


@pytest.fixture(scope="module")
def golden():
    return np.load(hc.GOLDEN)


# ---- the restatements and the drop-in modules against the reference's numbers ---------------------------------------------------
@pytest.mark.parametrize("case", hc.GOLDEN_TRIPLET, ids=hc.triplet_key)
def test_triplet_restatement_and_torch_path_against_the_reference(case, golden):
    """triplet_f64 against the reference's TripletLoss in float64: loss, dist_ap, dist_an and the gradient within 1e-12; the
    drop-in module on float64 host tensors the same"""
    x, y = hc.triplet_case(*case)
    key = "tri_" + hc.triplet_key(case)
    loss, g, ap, an = hc.triplet_f64(x, y, case[2])[:4]
    assert abs(loss - float(golden[key + "_loss"])) <= 1e-12
    assert np.abs(ap - golden[key + "_ap"]).max() <= 1e-12 and np.abs(an - golden[key + "_an"]).max() <= 1e-12
    X = torch.from_numpy(x).double().requires_grad_(True)
    l2, ap2, an2 = (TripletLoss() if case[2] is None else TripletLoss(case[2]))(X, torch.from_numpy(y))
    assert abs(float(l2.detach()) - float(golden[key + "_loss"])) <= 1e-12
    assert np.abs(ap2.detach().numpy() - golden[key + "_ap"]).max() <= 1e-12
    assert np.abs(an2.detach().numpy() - golden[key + "_an"]).max() <= 1e-12
    (g2,) = torch.autograd.grad(l2, [X])
    assert hc.rel_l2(g2.numpy(), g) <= 1e-12
    if key + "_grad" in golden:
        assert hc.rel_l2(g, golden[key + "_grad"]) <= 1e-12


@pytest.mark.parametrize("case", hc.GOLDEN_XENT, ids=hc.xent_key)
def test_label_smoothing_restatement_and_torch_path_against_the_reference(case, golden):
    """xent_f64 against the reference's CrossEntropyLabelSmooth on float64 logits within 1e-6 (the reference builds its targets
    in fp32; measured 2.8e-7 at 64 x 751); the drop-in module on float64 host tensors the same"""
    rows, classes, eps, _ = case
    logits, labels = hc.xent_case(*case)
    key = "xent_" + hc.xent_key(case)
    loss, g = hc.xent_f64(logits, labels, eps)
    ref = float(golden[key + "_loss"])
    assert abs(loss - ref) <= 1e-6 * max(abs(ref), 1.0)
    x = torch.from_numpy(logits).double().requires_grad_(True)
    l2 = CrossEntropyLabelSmooth(classes, epsilon=eps, use_gpu=False)(x, torch.from_numpy(labels))
    assert abs(float(l2.detach()) - loss) <= 1e-12 * max(abs(loss), 1.0)
    (g2,) = torch.autograd.grad(l2, [x])
    if classes > 1:
        assert hc.rel_l2(g2.numpy(), g) <= 1e-12
        if key + "_grad" in golden:
            assert hc.rel_l2(g, golden[key + "_grad"]) <= 1e-6
    else:
        assert not g.any() and float(np.abs(g2.numpy()).max()) <= 1e-16
    if eps == 0:
        assert abs(float(cross_entropy(x, torch.from_numpy(labels)).detach()) - loss) <= 1e-12 * max(abs(loss), 1.0)


def test_head_restatement_is_the_torch_head():
    """head_f64 (the appendix's restatement) against BatchNorm in training mode, a bias-free linear layer and the smoothed loss
    under torch autograd in float64"""
    s = hc.head_setup(128, 64)
    loss, dW, dgamma, df, mu, var = hc.head_f64(s["f"], s["bottleneck.weight"], s["bottleneck.bias"], s["classifier.weight"],
                                                s["target"], 0.1)
    losses, g = hc.head_host(s, "uniprompt", torch.float64, id_weight=1.0, triplet_weight=0.0, i2t_weight=0.0)
    assert abs(losses[1] - loss) <= 1e-12 * loss
    assert hc.rel_l2(g["classifier.weight"], dW) <= 1e-12 and hc.rel_l2(g["bottleneck.weight"], dgamma) <= 1e-12
    assert hc.rel_l2(g["f"], df) <= 1e-11
    B = len(s["target"])
    assert hc.rel_l2(g["bottleneck.running_mean"], 0.9 * s["bottleneck.running_mean"].astype(np.float64) + 0.1 * mu) <= 1e-12
    assert hc.rel_l2(g["bottleneck.running_var"], 0.9 * s["bottleneck.running_var"].astype(np.float64) + 0.1 * var * B / (B - 1)) <= 1e-12
    # the unused branch of the Uni-Prompt form: exact zeros
    for k in ("f_last", "classifier_proj.weight", "bottleneck_proj.weight", "bottleneck_proj.bias"):
        assert not g[k].any()


def test_bn_restatement_is_torch_batch_norm():
    x, dy, gamma, beta, rm, rv = hc.bn_case(65, 5)
    want = hc.bn_f64(x, dy, gamma, beta, rm, rv)
    X, G, Bt = (torch.from_numpy(t).double().requires_grad_(True) for t in (x, gamma, beta))
    m, v = torch.from_numpy(rm).double(), torch.from_numpy(rv).double()
    y = torch.nn.functional.batch_norm(X, m, v, G, Bt, True, hc.BN_MOMENTUM, hc.BN_EPS)
    dx, dg, db = torch.autograd.grad(y, [X, G, Bt], torch.from_numpy(dy).double())
    for got, k in ((y.detach(), "y"), (dx, "dx"), (dg, "dgamma"), (db, "dbeta"), (m, "running_mean"), (v, "running_var")):
        assert hc.rel_l2(got.numpy(), want[k]) <= 1e-11, k


# ---- make_loss -----------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    c = _base_cfg.clone()
    c.defrost()
    c.merge_from_list([v for pair in kw.items() for v in pair])
    return c


def test_config_defaults_are_the_references():
    c = _base_cfg
    assert (c.MODEL.ID_LOSS_WEIGHT, c.MODEL.TRIPLET_LOSS_WEIGHT, c.MODEL.I2T_LOSS_WEIGHT) == (1.0, 1.0, 1.0)
    assert (c.MODEL.METRIC_LOSS_TYPE, c.MODEL.NO_MARGIN, c.MODEL.IF_LABELSMOOTH) == ("triplet", False, "on")
    assert (c.DATALOADER.SAMPLER, c.DATALOADER.NUM_INSTANCE, c.SOLVER.MARGIN) == ("softmax", 16, 0.3)


@pytest.mark.parametrize("smooth", ["on", "off"])
@pytest.mark.parametrize("no_margin", [False, True])
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("i2t", [False, True])
def test_make_loss_branches_against_the_restatements(smooth, no_margin, lists, i2t):
    """softmax_triplet: ID_LOSS_WEIGHT * identity + TRIPLET_LOSS_WEIGHT * triplet [+ I2T_LOSS_WEIGHT * image-to-text], tensors
    or lists, smoothed or plain, margin or soft margin, in float64 on the host against xent_f64 and triplet_f64"""
    c = _cfg(**{"DATALOADER.SAMPLER": "softmax_triplet", "MODEL.IF_LABELSMOOTH": smooth, "MODEL.NO_MARGIN": no_margin,
                "MODEL.ID_LOSS_WEIGHT": 0.25, "MODEL.TRIPLET_LOSS_WEIGHT": 2.0, "MODEL.I2T_LOSS_WEIGHT": 0.5})
    s = hc.head_setup(128, 64, classes=37)
    rng = np.random.default_rng(3)
    scores = [rng.standard_normal((hc.HEAD_B, 37)) for _ in range(2)]
    logits = rng.standard_normal((hc.HEAD_B, 37))
    feats = [s["f_last"], s["f"], s["f_proj"]]
    loss_func, center = make_loss(c, 37)
    assert isinstance(center, CenterLoss) and tuple(center.centers.shape) == (37, 2048)
    y = torch.from_numpy(s["target"])
    sc_t = [torch.from_numpy(v) for v in scores] if lists else torch.from_numpy(scores[0])
    ft_t = [torch.from_numpy(v).double() for v in feats] if lists else torch.from_numpy(feats[1]).double()
    got = float(loss_func(sc_t, ft_t, y, None, torch.from_numpy(logits) if i2t else None))
    eps, margin = (0.1 if smooth == "on" else 0.0), (None if no_margin else 0.3)
    want = 0.25 * sum(hc.xent_f64(v, s["target"], eps)[0] for v in (scores if lists else scores[:1]))
    want += 2.0 * sum(hc.triplet_f64(v, s["target"], margin)[0] for v in (feats if lists else feats[1:2]))
    if i2t:
        want += 0.5 * hc.xent_f64(logits, s["target"], eps)[0]
    assert abs(got - want) <= 1e-12 * abs(want)


def test_make_loss_softmax_sampler_and_bad_settings():
    s = hc.head_setup(128, 64, classes=37)
    score = torch.from_numpy(np.random.default_rng(5).standard_normal((hc.HEAD_B, 37)))
    loss_func, _ = make_loss(_cfg(**{"DATALOADER.SAMPLER": "softmax"}), 37)
    got = float(loss_func(score, None, torch.from_numpy(s["target"])))
    assert abs(got - hc.xent_f64(score.numpy(), s["target"], 0.0)[0]) <= 1e-12 * got
    with pytest.raises(ValueError):
        make_loss(_cfg(**{"DATALOADER.SAMPLER": "triplet"}), 37)
    with pytest.raises(ValueError):
        make_loss(_cfg(**{"DATALOADER.SAMPLER": "softmax_triplet", "MODEL.METRIC_LOSS_TYPE": "center"}), 37)


def test_center_loss_is_the_mean_squared_distance_to_the_own_centre():
    c = CenterLoss(num_classes=5, feat_dim=8, use_gpu=False)
    x, y = torch.randn(6, 8, generator=torch.Generator().manual_seed(1)), torch.tensor([0, 1, 4, 4, 2, 0])
    want = ((x - c.centers.detach()[y]) ** 2).sum(1).mean()
    assert abs(float(c(x, y).detach()) - float(want)) <= 1e-6 * float(want)


# ---- the premises of the GPU cases ------------------------------------------------------------------------------------------------
def test_hot_cross_entropy_cases_hold_a_logit_that_overflows_an_unstabilised_exp():
    for case in hc.xent_cases():
        logits, labels = hc.xent_case(*case)
        assert logits.shape == case[:2] and labels.min() >= 0 and labels.max() < case[1]
        if case[3] == hc.XENT_SCALE_HOT:
            assert case[1] == 64 and float(logits.max()) > hc.OVERFLOW_LOGIT
    assert len([c for c in hc.xent_cases() if c[3] == hc.XENT_SCALE_HOT]) == 12


@pytest.mark.parametrize("case", [c for c in hc.triplet_cases() if c[2] is not None], ids=hc.triplet_key)
def test_margin_cases_keep_every_hinge_away_from_its_corner(case):
    """|ap - an + margin| >= 4 (ap + an) D 2^-23 in float64 for every anchor of every margin case"""
    x, y = hc.triplet_case(*case)
    assert hc.margin_premise(x, y, case[2]) >= 1.0


def test_triplet_case_shapes_and_tie_cases():
    sizes = {"2x1": 2, "2x2": 4, "16x4": 64, "13x5": 65, "4x16": 64, "ragged63": 63, "ragged65": 65, "ragged257": 257, "equal5": 5}
    for g, n in sizes.items():
        x, y = hc.triplet_case(g, 4, None)
        assert x.shape == (n, 4) and y.shape == (n,)
        xt, yt = hc.triplet_tie_case(g)
        d2 = hc.pair_d2(xt)
        assert np.array_equal(d2, np.round(d2)) and d2.max() <= 64          # exact small integers in fp32
        if n >= 63:
            d = hc.triplet_f64(xt, yt, None)[6]
            pos = yt[:, None] == yt[None, :]
            assert any((np.where(pos[a], d[a], -1) == np.where(pos[a], d[a], -1).max()).sum() > 1 for a in range(n))   # real ties
    assert len(np.unique(hc.triplet_case("ragged63", 4, None)[1], return_counts=True)[1]) > 5
    assert not hc.triplet_f64(*hc.triplet_case("equal5", 5, 0.3), 0.3)[1].any()       # no negatives: no loss, no gradient


def test_bn_cases_hold_a_column_of_equal_values():
    for b in hc.BN_BATCHES:
        for d in hc.BN_DIMS:
            x = hc.bn_case(b, d)[0]
            assert x.shape == (b, d) and (x[:, -1] == 1.5).all()
            assert hc.bn_f64(*hc.bn_case(b, d))["invstd"][-1] == pytest.approx(1 / np.sqrt(hc.BN_EPS))


def test_the_learning_run_learns_in_float64():
    curve = hc.learn_curve_host(torch.float64)
    assert len(curve) == hc.LEARN["steps"] and curve[-1] < 0.5 * curve[0]


# ---- the workspace query and the refusals, none of which needs a device ---------------------------------------------------------
def test_triplet_workspace_query_needs_no_device():
    L = _lib.load()
    for b, d in ((1, 1), (64, 768), (1024, 512)):
        n = L.mpreid_triplet_workspace_bytes(b, d)
        assert n >= 4 * b * b + 12 * b and n % 256 == 0
    assert L.mpreid_triplet_workspace_bytes(0, 4) == 0 and L.mpreid_triplet_workspace_bytes(1025, 4) == 0
    assert L.mpreid_triplet_workspace_bytes(4, 0) == 0
    assert _lib.TRIPLET_MAX_BATCH == 1024


def test_the_new_symbols_are_declared_and_exported():
    L = _lib.load()
    for name in ("mpreid_xent_rows_f32", "mpreid_triplet_workspace_bytes", "mpreid_triplet_hard_f32", "mpreid_bn1d_train_forward_f32",
                 "mpreid_bn1d_train_backward_f32", "mpreid_matmul_f32", "mpreid_stage2_total_f32"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    assert _lib.VERSION == 102


def test_argument_errors_are_found_before_anything_is_launched():
    """NULL pointers and bad sizes: the entry points return MPREID_ERR_ARG / MPREID_ERR_UNSUPPORTED on a host without a device"""
    L = _lib.load()
    one = 256   # a non-NULL, aligned address that is never dereferenced: every call below fails its argument check
    assert L.mpreid_bn1d_train_forward_f32(one, one, one, 1, 4, 1e-5, 0.1, one, one, one, None, None, None) == _lib.ERR_ARG
    assert b"batch of 1" in L.mpreid_last_error()
    assert L.mpreid_bn1d_train_forward_f32(one, one, one, 2, 4, 1e-5, 0.1, one, one, one, one, None, None) == _lib.ERR_ARG
    assert L.mpreid_bn1d_train_backward_f32(one, one, one, one, one, None, 1, 4, one, one, None, None) == _lib.ERR_ARG
    assert L.mpreid_triplet_hard_f32(one, one, 1025, 4, 0.3, 0, 0.0, 1.0, one, one, one, one, one, None, one, 1 << 30, None) == _lib.ERR_UNSUPPORTED
    assert L.mpreid_triplet_hard_f32(one, one, 4, 4, 0.3, 0, 0.0, 1.0, one, one, one, one, one, None, one, 16, None) == _lib.ERR_WORKSPACE
    assert L.mpreid_triplet_hard_f32(one, one, 0, 4, 0.3, 0, 0.0, 1.0, one, one, one, one, one, None, one, 1 << 30, None) == _lib.ERR_ARG
    assert L.mpreid_xent_rows_f32(one, 3, one, 2, 4, 0.1, 1.0, one, one, None, None, None) == _lib.ERR_ARG       # ld < classes
    assert L.mpreid_xent_rows_f32(one, 4, one, 2, 0, 0.1, 1.0, one, one, None, None, None) == _lib.ERR_ARG
    assert L.mpreid_xent_rows_f32(one, 4, one, 2, 4, 1.5, 1.0, one, one, None, None, None) == _lib.ERR_ARG       # epsilon
    assert L.mpreid_matmul_f32(one, 4, 1, one, 4, 1, 2, 2, 0, None, one, 2, None) == _lib.ERR_ARG
    assert L.mpreid_matmul_f32(one, 4, 1, one, 4, 1, 2, 3, 4, None, one, 2, None) == _lib.ERR_ARG                 # ldc < n
    assert L.mpreid_stage2_total_f32(one, 0, 0, 0, one, None) == _lib.ERR_ARG


def test_wrappers_and_modules_refuse_what_they_cannot_answer():
    with pytest.raises(ValueError):
        ops.check_class_labels(torch.tensor([0, 3, 7]), 3, 7)
    with pytest.raises(ValueError):
        ops.check_class_labels(torch.tensor([0, -1, 2]), 3, 7)
    with pytest.raises(ValueError):
        ops.check_class_labels(torch.tensor([0.0, 1.0, 2.0]), 3, 7)
    ops.check_class_labels(torch.tensor([0, 6, 2]), 3, 7)
    with pytest.raises(NotImplementedError):
        TripletLoss(0.3)(torch.zeros(4, 4), torch.tensor([0, 0, 1, 1]), normalize_feature=True)
    with pytest.raises((RuntimeError, IndexError)):
        CrossEntropyLabelSmooth(4, use_gpu=False)(torch.zeros(2, 4), torch.tensor([0, 4]))
    # a batch above 1024: the drop-in answers it in torch (ragged groups and all), the library refuses it
    x, y = torch.randn(1030, 3, generator=torch.Generator().manual_seed(0)), torch.arange(1030) % 7
    loss = TripletLoss(0.3)(x, y)[0]
    assert abs(float(loss) - hc.triplet_f64(x.numpy(), y.numpy(), 0.3)[0]) <= 1e-5 * float(loss)
