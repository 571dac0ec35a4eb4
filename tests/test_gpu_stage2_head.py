"""The stage-2 head on the GPU (csrc/stage2_head.hip through mpreid.ops, the drop-in losses and the model): row cross-entropy,
the batch-hard triplet loss, BatchNorm1d in training mode and the linear products against float64, their memory discipline and
run-to-run bits; Stage2Head.step in both forms against the float64 head under torch autograd; make_loss under autograd on
device tensors; a run that learns; the model's head and the invalidation of its folded encoder.  The bound everywhere is
stage1_cases.BOUND = 2e-5 (relative error of a loss, relative L2 of a gradient).  Inputs and float64 restatements:
tests/stage2_head_cases.py."""
import numpy as np
import pytest
import torch

import stage1_cases as sc
import stage2_head_cases as hc
from mpreid import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345   # a NaN pattern


def _guarded(shape, dtype=torch.float32, guard=64):
    """(the view of `shape` in the middle of an int32 buffer of sentinels, a function that says the guards are intact)"""
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    view = buf[guard:guard + n].view(dtype).view(*shape)

    def intact():
        return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())
    return view, intact


def _nan_tail(a, rows=8):
    """the array on the device followed by NaN guard rows in the same allocation -> (the view of the data, the guard rows)"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0] + rows,) + tuple(a.shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = a.cuda()
    return buf[:a.shape[0]], buf[a.shape[0]:]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _written(*ts):
    """no element keeps the sentinel"""
    return all(not bool((_bits(t) == SENTINEL).any()) for t in ts)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(got, want):
    want = float(want)
    return abs(float(got) - want) / abs(want) if want else abs(float(got))


# ---- 1. row cross-entropy ------------------------------------------------------------------------------------------------------
XENT_LOSS_SCALE = 3.0


@pytest.mark.parametrize("case", hc.xent_cases(), ids=hc.xent_key)
def test_xent_against_float64(case):
    """loss within 2e-5 relative, d_logits within 2e-5 relative L2 of float64, at scale 3; argmax is numpy's; classes = 1 gives
    loss 0 and gradient 0 exactly.  The fp32 autograd figure of the host is printed beside each.
    Largest figures measured on an MI355X over the 132 cases: loss 1.5e-7 (65 x 65, epsilon 0; the host's fp32 autograd: 7.8e-9),
    d_logits 1.5e-7 (1 x 2, epsilon 0: a loss of 1e-3 -- the host: 1.6e-5, it forms p - 1 from a rounded p); with the hot logits
    (largest above 89) loss 1.0e-7 and d_logits 6.3e-8."""
    rows, classes, eps, scale = case
    logits, labels = hc.xent_case(*case)
    want_loss, want_grad = hc.xent_want(rows, classes, eps, scale, XENT_LOSS_SCALE)
    loss, grad, am = ops.xent_rows(_cuda(logits), _cuda(labels), eps, XENT_LOSS_SCALE, need_argmax=True)
    loss, grad, am = float(loss.cpu()[0]), grad.cpu().numpy(), am.cpu().numpy()
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert np.array_equal(am, logits.argmax(1))
    if classes == 1:
        assert loss == 0.0 and not grad.any()
        return
    host = hc.xent_torch(logits, labels, eps, XENT_LOSS_SCALE, torch.float32)
    fig = (_rel(loss, want_loss), hc.rel_l2(grad, want_grad))
    print("xent %s: loss %.3e d_logits %.3e; fp32 autograd on the host %.3e %.3e"
          % (hc.xent_key(case), fig[0], fig[1], _rel(host[0], want_loss), hc.rel_l2(host[1], want_grad)))
    assert max(fig) <= hc.BOUND, fig


def test_xent_argmax_takes_the_lowest_of_equal_maxima_and_strided_rows():
    """a row of constructed equal maxima, in several waves and rounds of the workgroup; logits as a column slice of a wider
    matrix (leading dimension above the class count)"""
    logits, labels = hc.xent_case(65, 1025, 0.1, hc.XENT_SCALE)
    x = logits.copy()
    top = float(x.max()) + 1.0
    x[0, [900, 3, 259, 64]] = top
    x[1, :] = 0.25                      # every class equal
    x[2, [1024, 1023]] = top
    wide = torch.full((65, 1100), float("nan"), device="cuda")
    wide[:, 40:1065] = _cuda(x)
    loss, grad, am = ops.xent_rows(wide[:, 40:1065], _cuda(labels), 0.1, 1.0, need_argmax=True)
    am = am.cpu().numpy()
    assert am[0] == 3 and am[1] == 0 and am[2] == 1023 and np.array_equal(am, x.argmax(1))
    want = hc.xent_f64(x, labels, 0.1)
    assert _rel(loss.cpu()[0], want[0]) <= hc.BOUND and hc.rel_l2(grad.cpu().numpy(), want[1]) <= hc.BOUND


@pytest.mark.parametrize("case", [(65, 257, 0.1, hc.XENT_SCALE), (1, 1, 0.1, hc.XENT_SCALE), (3, 1025, 0.0, hc.XENT_SCALE)], ids=hc.xent_key)
def test_xent_writes_its_outputs_and_nothing_else(case):
    """NaN guard rows behind the logits, sentinel guards around every output; each optional output NULL in turn leaves the
    others' bits; a second call gives the same bits"""
    logits, labels = hc.xent_case(*case)
    rows, classes = logits.shape
    X, gx = _nan_tail(logits)
    y = _cuda(labels)
    outs = [_guarded((1,)), _guarded((rows,)), _guarded((rows, classes)), _guarded((rows,), torch.int32)]
    (loss, ok0), (rl, ok1), (dl, ok2), (am, ok3) = outs
    ops.xent_rows(X, y, case[2], 3.0, need_argmax=True, loss=loss, row_loss=rl, d_logits=dl, argmax=am)
    torch.cuda.synchronize()
    assert ok0() and ok1() and ok2() and ok3() and bool(torch.isnan(gx).all()) and _written(loss, rl, dl, am)
    for kw in (dict(need_grad=False, need_argmax=True), dict(need_grad=True, need_argmax=False), dict(need_grad=True, need_argmax=True)):
        (l2, k0), (r2, k1) = _guarded((1,)), _guarded((rows,))
        _, d2, a2 = ops.xent_rows(X, y, case[2], 3.0, loss=l2, row_loss=r2, **kw)
        torch.cuda.synchronize()
        assert k0() and k1() and torch.equal(_bits(l2), _bits(loss)) and torch.equal(_bits(r2), _bits(rl))
        assert (d2 is None) == (not kw["need_grad"]) and (a2 is None) == (not kw["need_argmax"])
        assert d2 is None or torch.equal(_bits(d2), _bits(dl))
        assert a2 is None or torch.equal(a2, am)


def test_xent_label_outside_the_classes_belongs_to_no_class():
    """the library treats such a label as data (no one-hot term); the wrapper refuses it beforehand"""
    logits, labels = hc.xent_case(3, 65, 0.1, hc.XENT_SCALE)
    bad = labels.copy()
    bad[1] = 65
    with pytest.raises(ValueError):
        ops.xent_rows(_cuda(logits), _cuda(bad), 0.1)
    for v in (65, -1, 2 ** 40):
        bad[1] = v
        loss, grad, _ = ops.xent_rows(_cuda(logits), _cuda(bad), 0.1, validate=False)
        s = logits.astype(np.float64)
        lp = s - s.max(1, keepdims=True) - np.log(np.exp(s - s.max(1, keepdims=True)).sum(1, keepdims=True))
        t = np.full(s.shape, 0.1 / 65)
        t[[0, 2], labels[[0, 2]]] += 0.9
        assert _rel(loss.cpu()[0], -(t * lp).sum() / 3) <= hc.BOUND
        assert hc.rel_l2(grad.cpu().numpy(), (np.exp(lp) - t) / 3) <= hc.BOUND


# ---- 2. batch-hard triplet loss ---------------------------------------------------------------------------------------------------
def _triplet_check(x, y, margin, exact_indices):
    """one call against float64 -> the figures (loss, gradient, worst distance excess of a mined index / its allowance)"""
    B, D = x.shape
    loss, ap, an, p, n, g = ops.triplet_hard(_cuda(x), _cuda(y), margin, scale=3.0)
    loss, ap, an, p, n, g = float(loss.cpu()[0]), ap.cpu().numpy(), an.cpu().numpy(), p.cpu().numpy(), n.cpu().numpy(), g.cpu().numpy()
    w_loss, _, w_ap, w_an, w_p, w_n, d = hc.triplet_f64(x, y, margin)
    assert np.isfinite(loss) and np.isfinite(g).all() and np.isfinite(ap).all()
    has_n = w_n >= 0
    assert np.array_equal(n >= 0, has_n) and np.isinf(an[~has_n]).all() and (an[~has_n] > 0).all()
    assert (p >= 0).all() and (p < B).all() and (n < B).all() and (y[p] == y).all() and (y[n[has_n]] != y[has_n]).all()
    if exact_indices:
        assert np.array_equal(p, w_p) and np.array_equal(n, w_n)
    # the float64 distance of each mined index is within D 2^-22 (relative) of the float64 optimum
    ar = np.arange(B)
    tol = D * 2.0 ** -22
    excess = max(float(np.max((w_ap - d[ar, p]) / w_ap)), float(np.max((d[ar, n][has_n] - w_an[has_n]) / w_an[has_n])) if has_n.any() else 0.0)
    assert excess <= tol, (excess, tol)
    assert np.allclose(ap, d[ar, p], rtol=tol, atol=0) and np.allclose(an[has_n], d[ar, n][has_n], rtol=tol, atol=0)
    # the gradient against float64 WITH the mined indices
    c_loss, c_g = hc.triplet_f64(x, y, margin, p, n)[:2]
    if not has_n.any():
        assert loss == 0.0 and not g.any()
        return 0.0, 0.0, excess / tol
    return _rel(loss, 3.0 * w_loss), (hc.rel_l2(g, 3.0 * c_g) if c_g.any() else float(np.abs(g).max())), excess / tol


@pytest.mark.parametrize("case", hc.triplet_cases(), ids=hc.triplet_key)
def test_triplet_against_float64(case):
    """loss within 2e-5 relative of float64; every mined index within D 2^-22 (relative, in float64 distance) of the float64
    optimum; d_feat within 2e-5 relative L2 of the float64 gradient computed with the mined indices; an anchor without negatives
    has n_idx -1, dist_an +inf and contributes nothing.  The fp32 autograd figure of the host is printed beside each.
    Largest figures measured on an MI355X over the 90 cases: loss 2.8e-6 and d_feat 2.9e-6 (2 x 1 at D = 512, soft margin: each
    anchor's positive is itself; the host: 2.8e-6 and 2.9e-6); the float64 distance of every mined index equalled the float64
    optimum (nothing of the D 2^-22 allowance was used)."""
    x, y = hc.triplet_case(*case)
    fig = _triplet_check(x, y, case[2], exact_indices=False)
    w = hc.triplet_want(*case)
    host = hc.triplet_torch(x, y, case[2], torch.float32)
    print("triplet %s: loss %.3e d_feat %.3e index excess / allowance %.3f; fp32 autograd on the host %.3e %.3e"
          % (hc.triplet_key(case), fig[0], fig[1], fig[2], _rel(host[0], w[0]) if w[0] else abs(host[0]),
             hc.rel_l2(host[1], w[1]) if w[1].any() else 0.0))
    assert max(fig[:2]) <= hc.BOUND, fig


@pytest.mark.parametrize("margin", hc.TRIPLET_FORMS, ids=["margin", "soft"])
@pytest.mark.parametrize("groups", hc.TRIPLET_GROUPS)
def test_triplet_exact_ties_take_the_lowest_index(groups, margin):
    """small-integer features at D = 4: every squared distance is exact in fp32, so the mined indices are float64's own, ties
    to the lowest index"""
    x, y = hc.triplet_tie_case(groups)
    fig = _triplet_check(x, y, margin, exact_indices=True)
    assert max(fig[:2]) <= hc.BOUND, fig


@pytest.mark.parametrize("case", [("ragged65", 5, hc.MARGIN), ("13x5", 512, None), ("equal5", 4, hc.MARGIN), ("ragged257", 64, None)],
                         ids=hc.triplet_key)
def test_triplet_writes_its_outputs_and_nothing_else(case):
    """NaN guard rows behind the features, sentinel guards around every output, d_feat NULL leaves the others' bits, a second
    call gives the same bits"""
    x, y = hc.triplet_case(*case)
    B, D = x.shape
    L = _lib.load()
    X, gx = _nan_tail(x)
    yd = _cuda(y)
    ws = torch.empty(L.mpreid_triplet_workspace_bytes(B, D), dtype=torch.uint8, device="cuda")

    def call(with_grad):
        outs = [_guarded((1,)), _guarded((B,)), _guarded((B,)), _guarded((B,), torch.int32), _guarded((B,), torch.int32), _guarded((B, D))]
        ptr = [ops._ptr(o[0]) for o in outs]
        if not with_grad:
            ptr[5] = None
        _lib.check(L.mpreid_triplet_hard_f32(ops._ptr(X), ops._ptr(yd), B, D, float(case[2] or 0.0), int(case[2] is None), 0.0, 3.0,
                                             *ptr, ops._ptr(ws), ws.numel(), _lib.stream_ptr()), "triplet")
        torch.cuda.synchronize()
        assert all(ok() for _, ok in outs) and bool(torch.isnan(gx).all())
        n_out = 6 if with_grad else 5
        assert _written(*[o[0] for o in outs[:n_out]])
        assert with_grad or bool((_bits(outs[5][0]) == SENTINEL).all())
        return [o[0] for o in outs[:n_out]]
    first, no_grad, again = call(True), call(False), call(True)
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(first, no_grad):
        assert torch.equal(_bits(a), _bits(b))


def test_triplet_limits():
    with pytest.raises(ValueError):
        ops.triplet_hard(torch.zeros(1025, 4, device="cuda"), torch.zeros(1025, dtype=torch.int64, device="cuda"))
    x, y = hc.triplet_case("ragged65", 5, None)
    big = np.tile(x, (16, 1))[:1024]
    yb = np.tile(y, 16)[:1024]
    fig = _triplet_check(big, yb, None, exact_indices=False)     # the largest batch: duplicates, pairs at distance 0
    assert max(fig[:2]) <= hc.BOUND
    one = ops.triplet_hard(torch.ones(1, 3, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), 0.3)
    assert float(one[0].cpu()[0]) == 0.0 and int(one[4].cpu()[0]) == -1 and not one[5].cpu().numpy().any()


# ---- 3. BatchNorm1d in training mode --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", hc.BN_DIMS)
@pytest.mark.parametrize("batch", hc.BN_BATCHES)
def test_bn_against_float64(batch, dim):
    """forward, saved statistics, running statistics, dx, dgamma and dbeta within 2e-5 relative L2 of float64; the column of equal
    values comes out as beta exactly; guards intact, dbeta NULL and a second call leave the bits.
    Largest figures measured on an MI355X over the 16 cases: dx 4.5e-6 (2 x 768), everything else at most 7.6e-7."""
    x, dy, gamma, beta, rm, rv = hc.bn_case(batch, dim)
    want = hc.bn_f64(x, dy, gamma, beta, rm, rv)
    X, gx = _nan_tail(x)
    DY, gdy = _nan_tail(dy)
    G, Bt = _cuda(gamma), _cuda(beta)
    (y, k0), (mean, k1), (inv, k2), (r_m, k3), (r_v, k4) = (_guarded(s) for s in ((batch, dim), (dim,), (dim,), (dim,), (dim,)))
    r_m.copy_(_cuda(rm))
    r_v.copy_(_cuda(rv))
    ops.bn1d_train(X, G, Bt, r_m, r_v, hc.BN_MOMENTUM, hc.BN_EPS, y=y, mean=mean, invstd=inv)
    (dx, k5), (dg, k6), (db, k7) = (_guarded(s) for s in ((batch, dim), (dim,), (dim,)))
    ops.bn1d_train_backward(X, DY, G, mean, inv, dx=dx, dweight=dg, dbias=db)
    torch.cuda.synchronize()
    assert all(k() for k in (k0, k1, k2, k3, k4, k5, k6, k7)) and bool(torch.isnan(gx).all()) and bool(torch.isnan(gdy).all())
    assert _written(y, mean, inv, dx, dg, db)
    got = dict(y=y, mean=mean, invstd=inv, running_mean=r_m, running_var=r_v, dx=dx, dgamma=dg, dbeta=db)
    fig = {k: hc.rel_l2(v.cpu().numpy(), want[k]) for k, v in got.items()}
    print("bn %dx%d: %s" % (batch, dim, " ".join("%s %.2e" % kv for kv in fig.items())))
    assert max(fig.values()) <= hc.BOUND, fig
    assert np.array_equal(y[:, -1].cpu().numpy(), np.full(batch, beta[-1], np.float32))
    # no running statistics, no dbeta, and again: the other outputs keep their bits
    y2, m2, i2 = ops.bn1d_train(X, G, Bt)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(m2), _bits(mean)) and torch.equal(_bits(i2), _bits(inv))
    dx2, dg2, db2 = ops.bn1d_train_backward(X, DY, G, mean, inv, need_dbeta=False)
    assert db2 is None and torch.equal(_bits(dx2), _bits(dx)) and torch.equal(_bits(dg2), _bits(dg))
    add = _cuda(dy[::-1].copy())
    dx3 = ops.bn1d_train_backward(X, DY, G, mean, inv, dx_add=add)[0]
    assert torch.equal(_bits(dx3), _bits(dx + add))


def test_bn_refuses_a_batch_of_one():
    with pytest.raises(ValueError):
        ops.bn1d_train(torch.zeros(1, 4, device="cuda"), torch.ones(4, device="cuda"), torch.zeros(4, device="cuda"))


# ---- 4. the linear products --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", hc.LINEAR_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_linear_products_against_float64(size):
    """S = f W^T, d_f = dS W (and + add), dW = dS^T f within 2e-5 relative L2 of float64; guards intact; the same bits twice.
    Measured on an MI355X at (64, 768, 751): S 4.9e-7, d_f 4.9e-7, dW 1.4e-7."""
    f, W, dS = hc.linear_case(*size)
    B, D, C = size
    F, gf = _nan_tail(f)
    Wd, gw = _nan_tail(W)
    dSd, gs = _nan_tail(dS)
    (S, k0), (df, k1), (dW, k2) = _guarded((B, C)), _guarded((B, D)), _guarded((C, D))
    ops.linear_forward(F, Wd, out=S)
    ops.linear_grad_input(dSd, Wd, out=df)
    ops.linear_grad_weight(dSd, F, out=dW)
    torch.cuda.synchronize()
    assert k0() and k1() and k2() and all(bool(torch.isnan(g).all()) for g in (gf, gw, gs)) and _written(S, df, dW)
    f64, W64, dS64 = (t.astype(np.float64) for t in (f, W, dS))
    fig = (hc.rel_l2(S.cpu().numpy(), f64 @ W64.T), hc.rel_l2(df.cpu().numpy(), dS64 @ W64), hc.rel_l2(dW.cpu().numpy(), dS64.T @ f64))
    print("linear %s: S %.2e d_f %.2e dW %.2e" % (size, fig[0], fig[1], fig[2]))
    assert max(fig) <= hc.BOUND, fig
    assert torch.equal(_bits(ops.linear_forward(F, Wd)), _bits(S)) and torch.equal(_bits(ops.linear_grad_weight(dSd, F)), _bits(dW))
    add = _cuda(f[::-1].copy())
    assert torch.equal(_bits(ops.linear_grad_input(dSd, Wd, add=add)), _bits(df + add))


# ---- 5. Stage2Head.step ------------------------------------------------------------------------------------------------------------
def _make_head(s, on_update=None, **kw):
    p = {k: _cuda(s[k]) for k in hc.PARAMS}
    bn = {}
    for name in ("bottleneck", "bottleneck_proj"):
        bn[name] = dict(weight=p[name + ".weight"], bias=p[name + ".bias"], running_mean=_cuda(s[name + ".running_mean"]),
                        running_var=_cuda(s[name + ".running_var"]), num_batches_tracked=torch.tensor(0, dtype=torch.long, device="cuda"))
    head = ops.Stage2Head(p["classifier.weight"], p["classifier_proj.weight"], bn["bottleneck"], bn["bottleneck_proj"],
                          on_update=on_update, **kw)
    return head, p, bn


@pytest.mark.parametrize("form", ops.Stage2Head.FORMS)
@pytest.mark.parametrize("widths", hc.HEAD_WIDTHS, ids=lambda w: "%dx%d" % w)
def test_head_step_against_the_float64_head_under_autograd(widths, form):
    """the loss and its three parts, the three feature gradients, the six parameter gradients and the running statistics of one
    step (B = 64 as 16 x 4, 751 identities, 751 text features) against the float64 head under torch autograd on the host; the
    zeros of the unused branch of the Uni-Prompt form are exact; a second step on the same inputs gives the same bits.
    Largest figures measured on an MI355X over the four cases: loss 3.9e-7 (the host's fp32 autograd: 3.9e-7), gradients 1.4e-6
    (d_f_proj at 768 / 512, Uni-Prompt form; the host: 5.2e-7), parameter gradients 5.9e-7, running statistics 2.7e-8."""
    s = hc.head_setup(*widths)
    head, p, bn = _make_head(s, epsilon=0.1, margin=hc.MARGIN, **hc.HEAD_WEIGHTS)
    args = [_cuda(s[k]) for k in ("f_last", "f", "f_proj", "target")]
    out = head.step(*args, text_features=_cuda(s["text"]), form=form, validate=True, write_grad=True)
    want_loss, want = hc.head_host(s, form, torch.float64)
    host_loss, host = hc.head_host(s, form, torch.float32)
    got_loss = np.array([float(out.loss.cpu()[0]), float(out.id_loss.cpu()), float(out.triplet_loss.cpu()), float(out.i2t_loss.cpu())])
    got = {"f_last": out.d_f_last, "f": out.d_f, "f_proj": out.d_f_proj, **out.grads}
    for name in ("bottleneck", "bottleneck_proj"):
        got[name + ".running_mean"], got[name + ".running_var"] = bn[name]["running_mean"], bn[name]["running_var"]
    fig = {"loss": float(np.max(np.abs(got_loss - want_loss) / want_loss))}
    hfig = {"loss": float(np.max(np.abs(host_loss - want_loss) / want_loss))}
    unused = ("f_last", "classifier_proj.weight", "bottleneck_proj.weight", "bottleneck_proj.bias") if form == "uniprompt" else ()
    for k, v in got.items():
        v = v.cpu().numpy()
        assert v.shape == want[k].shape, k
        if k in unused:
            assert not v.any() and not want[k].any(), k
        else:
            fig[k], hfig[k] = hc.rel_l2(v, want[k]), hc.rel_l2(host[k], want[k])
    print("head %s %s: %s\n  fp32 autograd on the host: %s" % (widths, form, " ".join("%s %.2e" % kv for kv in fig.items()),
                                                               " ".join("%s %.2e" % kv for kv in hfig.items())))
    assert max(fig.values()) <= hc.BOUND, fig
    used = 1 if form == "uniprompt" else 2
    assert int(bn["bottleneck"]["num_batches_tracked"]) == 1 and int(bn["bottleneck_proj"]["num_batches_tracked"]) == used - 1
    for k in hc.PARAMS:
        assert torch.equal(p[k].grad, out.grads[k])
    y = s["target"]
    logits = s["f_proj"].astype(np.float64) @ s["text"].astype(np.float64).T
    assert abs(float(out.acc) - float((logits.argmax(1) == y).mean())) <= 1e-6
    assert hc.rel_l2(out.i2t_logits.cpu().numpy(), logits) <= hc.BOUND
    # the same inputs again (the running statistics put back): the same bits
    keep = {k: v.clone() for k, v in got.items()}
    keep_loss = out.loss.clone()
    for name in ("bottleneck", "bottleneck_proj"):
        bn[name]["running_mean"].copy_(_cuda(s[name + ".running_mean"]))
        bn[name]["running_var"].copy_(_cuda(s[name + ".running_var"]))
    out2 = head.step(*args, text_features=_cuda(s["text"]), form=form)
    got2 = {"f_last": out2.d_f_last, "f": out2.d_f, "f_proj": out2.d_f_proj, **out2.grads}
    assert torch.equal(_bits(out2.loss), _bits(keep_loss))
    for k, v in got2.items():
        assert torch.equal(_bits(v), _bits(keep[k])), k


def test_head_list_form_without_text_features_and_plain_settings():
    """the list form without the image-to-text term, plain cross-entropy and the soft margin"""
    s = hc.head_setup(128, 64)
    head, p, bn = _make_head(s, epsilon=None, margin=None, **hc.HEAD_WEIGHTS)
    out = head.step(*[_cuda(s[k]) for k in ("f_last", "f", "f_proj", "target")], form="list")
    want_loss, want = hc.head_host(s, "list", torch.float64, epsilon=0.0, margin=None, with_text=False)
    assert out.acc is None and out.i2t_logits is None and float(out.i2t_loss.cpu()) == 0.0
    assert _rel(out.loss.cpu()[0], want_loss[0]) <= hc.BOUND
    got = {"f_last": out.d_f_last, "f": out.d_f, "f_proj": out.d_f_proj, **out.grads}
    for k, v in got.items():
        assert hc.rel_l2(v.cpu().numpy(), want[k]) <= hc.BOUND, k
    with pytest.raises(ValueError):
        head.step(*[_cuda(s[k]) for k in ("f_last", "f", "f_proj", "target")], form="uniprompt")
    bad = _cuda(s["target"]).clone()
    bad[0] = hc.HEAD_C
    with pytest.raises(ValueError):
        head.step(*[_cuda(s[k]) for k in ("f_last", "f", "f_proj")], bad, form="list", validate=True)


# ---- 6. make_loss under autograd on device tensors -----------------------------------------------------------------------------
@pytest.mark.parametrize("lists", [False, True], ids=["tensors", "lists"])
def test_make_loss_on_device_tensors_gives_the_heads_gradients(lists):
    """loss_func of make_loss on CUDA tensors that require gradients: every term is an autograd function over the kernels;
    value and gradients against float64 autograd of the same composition on the host"""
    from config import cfg as base
    from loss.make_loss import make_loss
    c = base.clone()
    c.defrost()
    c.merge_from_list(["DATALOADER.SAMPLER", "softmax_triplet", "MODEL.ID_LOSS_WEIGHT", 0.25, "MODEL.I2T_LOSS_WEIGHT", 0.5])
    s = hc.head_setup(128, 64)
    rng = np.random.default_rng(8)
    arrays = {"score": rng.standard_normal((hc.HEAD_B, hc.HEAD_C)).astype(np.float32) * 2,
              "score_proj": rng.standard_normal((hc.HEAD_B, hc.HEAD_C)).astype(np.float32) * 2,
              "i2t": rng.standard_normal((hc.HEAD_B, hc.HEAD_C)).astype(np.float32) * 2,
              "f_last": s["f_last"], "f": s["f"], "f_proj": s["f_proj"]}
    loss_func, _ = make_loss(c, hc.HEAD_C)

    def run(dev, dtype):
        t = {k: torch.from_numpy(v).to(device=dev, dtype=dtype).requires_grad_(True) for k, v in arrays.items()}
        y = torch.from_numpy(s["target"]).to(dev)
        if lists:
            loss = loss_func([t["score"], t["score_proj"]], [t["f_last"], t["f"], t["f_proj"]], y, None, t["i2t"])
            keys = list(arrays)
        else:
            loss = loss_func(t["score"], t["f"], y, None, t["i2t"])
            keys = ["score", "f", "i2t"]
        grads = torch.autograd.grad(loss, [t[k] for k in keys])
        return loss, dict(zip(keys, grads))
    loss, grads = run("cuda", torch.float32)
    names = set()
    todo, seen = [loss.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo += [n for n, _ in fn.next_functions]
    assert any(n.startswith("_XentRows") for n in names) and any(n.startswith("_TripletHard") for n in names)
    w_loss, w_grads = run("cpu", torch.float64)
    assert _rel(loss.detach().cpu(), w_loss.detach()) <= hc.BOUND
    for k, g in grads.items():
        assert g.is_cuda and hc.rel_l2(g.cpu().numpy(), w_grads[k].numpy()) <= hc.BOUND, k


# ---- 7. a run that learns ---------------------------------------------------------------------------------------------------------
def test_forty_steps_learn_and_follow_the_float64_curve():
    """40 steps on fixed clustered features (6 identities x 8, widths 128 / 64), the list form without text features; the head's
    six parameters are updated with ops.adam_step from the head's gradients.  The loss curve stays within 1e-3 relative of the
    same loop in float64 on the host (the figure of the stage-1 curve test), and the last loss is below half of the first.
    Measured on an MI355X: loss 3.6540 -> 0.8715, largest deviation from the float64 curve 1.4e-7 (the fp32 host loop: 3.1e-7)."""
    s = hc.learn_setup()
    head, p, bn = _make_head(s, epsilon=0.1, margin=hc.MARGIN)
    args = [_cuda(s[k]) for k in ("f_last", "f", "f_proj", "target")]
    state = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in p.items()}
    curve = []
    for step in range(1, hc.LEARN["steps"] + 1):
        out = head.step(*args, form="list")
        curve.append(out.loss.clone())
        for k, v in p.items():
            ops.adam_step(v, out.grads[k], state[k][0], state[k][1], step, hc.LEARN["lr"], (sc.BETA1, sc.BETA2), sc.EPS, 0.0, False)
    curve = torch.cat(curve).cpu().numpy().astype(np.float64)
    want = hc.learn_curve_host(torch.float64)
    dev = sc.curve_deviation(curve, want)
    print("learning run: loss %.4f -> %.4f, largest relative deviation from the float64 curve %.3e (fp32 host loop: %.3e)"
          % (curve[0], curve[-1], dev, sc.curve_deviation(hc.learn_curve_host(torch.float32), want)))
    assert dev <= 1e-3 and curve[-1] < 0.5 * curve[0]
    assert int(bn["bottleneck"]["num_batches_tracked"]) == hc.LEARN["steps"]


# ---- 8. the model's head -----------------------------------------------------------------------------------------------------------
def test_model_head_step_changes_what_the_eval_forward_folds():
    """model.stage2_head(cfg).step(...) on a make_model model, then model.eval()(x) with TEST.NECK_FEAT 'after': the features are
    those of the updated running statistics, so the step has dropped the folded encoder"""
    from config import cfg as base
    from model.make_model import make_model
    from mpreid import synth
    c = base.clone()
    c.defrost()
    c.merge_from_list(["TEST.NECK_FEAT", "after", "INPUT.SIZE_TRAIN", [64, 32], "INPUT.SIZE_TEST", [64, 32]])
    model = make_model(c, 37, 1, 1).to("cuda")
    x = torch.from_numpy(synth.synthetic_images(4, 64, 32, seed=3))
    model.eval()
    before = model(x).clone()
    s = hc.head_setup(768, 512, classes=37)
    head = model.stage2_head(c)
    out = head.step(*[_cuda(s[k]) for k in ("f_last", "f", "f_proj", "target")], text_features=_cuda(s["text"]), validate=True)
    assert float(out.loss.cpu()[0]) > 0 and int(model.bottleneck.num_batches_tracked) == 1
    rm = model.bottleneck.running_mean.cpu().numpy()
    assert hc.rel_l2(rm, 0.1 * s["f"].astype(np.float64).mean(0)) <= hc.BOUND          # from zeros, momentum 0.1
    assert model._encoder is None
    after = model(x)
    # the first 768 features pass the bottleneck whose statistics moved; the projected ones keep theirs in the Uni-Prompt form
    assert not torch.equal(after[:, :768], before[:, :768]) and torch.equal(after[:, 768:], before[:, 768:])
    raw_cfg = c.clone()
    raw_cfg.merge_from_list(["TEST.NECK_FEAT", "before"])
    raw = make_model(raw_cfg, 37, 1, 1)
    raw.load_state_dict(model.state_dict())
    pooled = raw.eval()(x)[:, :768].double().cpu()
    bn = model.bottleneck
    want = (pooled - bn.running_mean.double().cpu()) / torch.sqrt(bn.running_var.double().cpu() + 1e-5) * bn.weight.double().cpu() \
        + bn.bias.double().cpu()
    assert hc.rel_l2(after[:, :768].cpu().numpy(), want.numpy()) <= 1e-4
