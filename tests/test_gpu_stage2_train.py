"""Stage-2 training on the GPU (csrc/optim.hip through mpreid.ops and the drop-in modules): the multi-tensor optimizer step
against the single-tensor Adam kernel bit for bit and against the float64 lines of SGD, its memory discipline and run-to-run
bits; the per-tensor largest finite entry against torch's expression; the batched re-pack against sync_weights() byte for byte;
the fused Stage2Trainer step against float64 on the reduced tower; do_train_stage2 on the Uni-Prompt model against the autograd
path with its checkpoint round trip.  Inputs and float64 oracles: tests/stage2_train_cases.py."""
import logging

import numpy as np
import pytest
import torch

import stage1_cases as sc
import stage2_head_cases as hc
import stage2_train_cases as s2
import vit_grad_cases as vg
from mpreid import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345   # a NaN pattern
GUARD = 64              # int32 words on either side: 256 bytes, so the view keeps the allocation's 16-byte alignment


def _guarded(a, misalign=False):
    """the fp32 array on the device between sentinel guards (misalign: 4 bytes past a 16-byte boundary) -> (view, intact())"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    n, off = a.size, GUARD + (1 if misalign else 0)
    buf = torch.full((off + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    view = buf[off:off + n].view(torch.float32)
    view.copy_(torch.from_numpy(a))
    assert (view.data_ptr() % 16 == 4) if misalign else (view.data_ptr() % 16 == 0)

    def intact():
        return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())
    return view, intact


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _table(sizes, classes, misalign=None, seed=0):
    """entries (p, g, s1, s2, class) over guarded device buffers of the given sizes, the host arrays, and the guards' checks;
    misalign = (entry, buffer 0..3): that one buffer sits 4 bytes past a 16-byte boundary"""
    entries, host, checks = [], [], []
    for i, n in enumerate(sizes):
        arrays = s2.opt_state(n, seed + i)
        dev = []
        for j, a in enumerate(arrays):
            view, intact = _guarded(a, misalign == (i, j))
            dev.append(view)
            checks.append(intact)
        entries.append(tuple(dev) + (i % len(classes),))
        host.append(arrays)
    return entries, host, checks


def _adam_expected(entries, classes, step, decoupled):
    """ops.adam_step on copies of every entry -> [(p, m, v)] bits"""
    out = []
    for p, g, m, v, k in entries:
        p, m, v = p.clone(), m.clone(), v.clone()
        ops.adam_step(p, g.clone(), m, v, step, classes[k][0], (sc.BETA1, sc.BETA2), sc.EPS, classes[k][1], decoupled)
        out.append((_bits(p), _bits(m), _bits(v)))
    return out


# ---- 1. the optimizer table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", s2.OPT_STEPS)
@pytest.mark.parametrize("algo", ["Adam", "AdamW"])
def test_adam_table_is_bit_equal_to_the_single_tensor_kernel(algo, step):
    """every size of OPT_SIZES in ONE table (1 class, and the three of the reference), steps 1, 2 and 1000: each tensor carries the
    bits of ops.adam_step on a copy; the guards around all 36 buffers are intact, the gradients keep their bits, and a second
    run from the same state gives the same bits"""
    for classes in ([s2.CLASSES8[0]], s2.CLASSES8[:3]):
        entries, _, checks = _table(s2.OPT_SIZES, classes, seed=step)
        want = _adam_expected(entries, classes, step, algo == "AdamW")
        grads = [_bits(e[1]) for e in entries]
        again = [tuple(t.clone() for t in e[:4]) + (e[4],) for e in entries]
        ops.optim_step_multi(ops.OptimTable(entries), classes, algo, step, (sc.BETA1, sc.BETA2), sc.EPS)
        ops.optim_step_multi(ops.OptimTable(again), classes, algo, step, (sc.BETA1, sc.BETA2), sc.EPS)
        for (p, g, m, v, _), (p2, _, m2, v2, _), (wp, wm, wv), g0, n in zip(entries, again, want, grads, s2.OPT_SIZES):
            assert np.array_equal(_bits(p), wp) and np.array_equal(_bits(m), wm) and np.array_equal(_bits(v), wv), n
            assert np.array_equal(_bits(g), g0), n
            assert np.array_equal(_bits(p2), wp) and np.array_equal(_bits(m2), wm) and np.array_equal(_bits(v2), wv), n
        assert all(c() for c in checks)


@pytest.mark.parametrize("which", range(4), ids=["param", "grad", "exp_avg", "exp_avg_sq"])
def test_one_misaligned_buffer_takes_the_one_element_path_with_the_same_bits(which):
    """each of the four buffers of an entry 4 bytes past a 16-byte boundary in turn (the other three aligned), at 5, 1025 and one
    chunk + 1 elements, beside aligned entries of the same sizes in the same table: the bits of ops.adam_step, guards intact"""
    sizes = s2.OPT_MISALIGNED_SIZES + s2.OPT_MISALIGNED_SIZES
    classes = s2.CLASSES8[:2]
    for bad in range(3):
        entries, _, checks = _table(sizes, classes, misalign=(bad, which), seed=10 * which + bad)
        want = _adam_expected(entries, classes, 2, False)
        ops.optim_step_multi(ops.OptimTable(entries), classes, "Adam", 2, (sc.BETA1, sc.BETA2), sc.EPS)
        for (p, _, m, v, _), (wp, wm, wv) in zip(entries, want):
            assert np.array_equal(_bits(p), wp) and np.array_equal(_bits(m), wm) and np.array_equal(_bits(v), wv)
        assert all(c() for c in checks)


@pytest.mark.parametrize("n_entries,n_classes", [(1, 1), (200, 8)])
def test_table_of_one_and_of_two_hundred_entries(n_entries, n_classes):
    """1 entry with 1 class, 200 entries (four launches) with 8 classes: the bits of ops.adam_step per tensor, and the launch
    count the header documents"""
    sizes = [s2.OPT_SIZES[i % 6] + (i // 6) for i in range(n_entries)]     # 1 .. 1058 elements
    if n_entries > 1:
        sizes[77], sizes[150] = s2.CHUNK + 1, 2 * s2.CHUNK
    classes = s2.CLASSES8[:n_classes]
    entries, _, checks = _table(sizes, classes, seed=500)
    want = _adam_expected(entries, classes, 3, True)
    ops.optim_step_multi(ops.OptimTable(entries), classes, "AdamW", 3, (sc.BETA1, sc.BETA2), sc.EPS)
    for i, ((p, _, m, v, _), (wp, wm, wv)) in enumerate(zip(entries, want)):
        assert np.array_equal(_bits(p), wp) and np.array_equal(_bits(m), wm) and np.array_equal(_bits(v), wv), i
    assert all(c() for c in checks)
    assert ops.optim_step_launches(n_entries) == (n_entries + 63) // 64
    assert ops.optim_step_launches(155) <= 8


@pytest.mark.parametrize("wd", s2.SGD_WD)
@pytest.mark.parametrize("step", [1, 2])
def test_sgd_table_within_one_ulp_of_the_float64_lines(step, wd):
    """SGD with momentum over every size of OPT_SIZES (one of them misaligned), steps 1 and 2, weight decay 0 and 5e-4: parameter
    and momentum buffer within 1 fp32 ulp of the three lines computed in float64 and rounded to fp32 line by line; state2 is NULL;
    step 1 ignores what the momentum buffer held; guards intact, gradients unchanged, two runs the same bits"""
    classes = [(s2.SGD_LR, wd), (2 * s2.SGD_LR, 0.0)]
    entries, host, checks = _table(s2.OPT_SIZES, classes, misalign=(5, 2), seed=40 + step)
    sgd = [(p, g, m, None, k) for p, g, m, _, k in entries]
    again = [(p.clone(), g.clone(), m.clone(), None, k) for p, g, m, _, k in entries]
    v0 = [_bits(e[3]) for e in entries]
    ops.optim_step_multi(ops.OptimTable(sgd), classes, "SGD", step, momentum=s2.SGD_MU)
    ops.optim_step_multi(ops.OptimTable(again), classes, "SGD", step, momentum=s2.SGD_MU)
    worst = 0.0
    for (p, g, m, v, k), (p2, _, m2, _, _), (hp, hg, hm, _), vb in zip(entries, again, host, v0):
        wp, wm = s2.sgd_lines(hp, hg, hm, step, classes[k][0], s2.SGD_MU, classes[k][1])
        for got, want in ((p, wp), (m, wm)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - want) / sc.ulp32(want)
            worst = max(worst, float(err.max()))
        assert np.array_equal(_bits(g), hg.view(np.uint32)) and np.array_equal(_bits(v), vb)     # (exp_avg_sq: not SGD's)
        assert np.array_equal(_bits(p), _bits(p2)) and np.array_equal(_bits(m), _bits(m2))
    print(f"SGD step {step} wd {wd}: largest deviation {worst:.2f} ulp")
    assert worst <= 1.0
    assert all(c() for c in checks)


def test_table_errors_are_found_before_anything_is_launched():
    """on the device too: a bad entry among good ones is MPREID_ERR_ARG and NO tensor of the table has changed"""
    classes = s2.CLASSES8[:2]
    entries, _, _ = _table((5, 1025), classes)
    before = [[_bits(t) for t in e[:4]] for e in entries]
    tab = ops.OptimTable(entries)
    tab.c[1].hyper = 2
    with pytest.raises(RuntimeError, match="table entry 1"):
        ops.optim_step_multi(tab, classes, "Adam", 1)
    tab.c[1].hyper = 0
    with pytest.raises(RuntimeError):
        ops.optim_step_multi(tab, classes, "Adam", 0)
    with pytest.raises(RuntimeError):
        ops.optim_step_multi(tab, [(float("nan"), 0.0), (1e-3, 0.0)], "Adam", 1)
    torch.cuda.synchronize()
    for e, b in zip(entries, before):
        assert all(np.array_equal(_bits(t), x) for t, x in zip(e[:4], b))


# ---- 2. the largest finite entry ----------------------------------------------------------------------------------------------
def test_absmax_multi_is_bit_equal_to_the_torch_expression():
    """sizes 1, 63, 64, 65, 4097 and a 768 x 3072 matrix, plain; with NaN, +Inf and -Inf planted (at the front, the back and the
    chunk edge); tensors that hold nothing but NaN / Inf; an all-zero tensor; a misaligned view -- all in one table, every output
    bit-equal to torch.nan_to_num(t, 0, 0, 0).abs().max(); the guards around the output intact"""
    tensors = []
    for shape in s2.ABSMAX_SHAPES:
        a = s2.absmax_input(shape)
        tensors.append(torch.from_numpy(a).cuda())
        b = a.copy().reshape(-1)
        b[0] = np.nan
        b[-1] = np.inf
        b[b.size // 2] = -np.inf
        if b.size > s2.CHUNK:
            b[s2.CHUNK - 1], b[s2.CHUNK] = np.inf, np.nan
            b[int(np.argmax(np.where(np.isfinite(b), np.abs(b), 0)))] = np.nan     # the largest finite entry goes too
        tensors.append(torch.from_numpy(b.reshape(shape)).cuda())
    tensors += [torch.full((n,), v, device="cuda") for n in (1, 65, 4097) for v in (float("nan"), float("inf"), float("-inf"))]
    tensors += [torch.zeros(4097, device="cuda"), torch.zeros(1, device="cuda")]
    odd = torch.from_numpy(s2.absmax_input((4101,), 1)).cuda()
    tensors.append(odd[1:])
    assert tensors[-1].data_ptr() % 16 == 4
    want = torch.stack([s2.absmax_torch(t) for t in tensors])
    buf = torch.full((GUARD + len(tensors) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + len(tensors)].view(torch.float32)
    ops.absmax_multi(tensors, out=out)
    assert np.array_equal(_bits(out), _bits(want)), (out, want)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + len(tensors):] == SENTINEL).all())
    assert float(want[len(s2.ABSMAX_SHAPES) * 2]) == 0.0 and float(out[-3]) == 0.0
    one = ops.absmax_multi(tensors[10:11])
    assert np.array_equal(_bits(one), _bits(want[10:11]))


# ---- 3. the batched re-pack ---------------------------------------------------------------------------------------------------
def _reduced_encoder(ws_tag):
    s = s2.train_setup()
    enc = ops.VitEncoder(s["cfg"], s["sd"], s2.TRAIN["img_hw"], ws_tag=ws_tag)
    enc.enable_training()
    return s, enc


def _struct_state(enc):
    """every scale and every pointer of the library's structs, as numbers"""
    out = {"conv_s": enc.c_w.conv_s}
    for name, _ in _lib.VitWeights._fields_:
        if name not in ("layers", "conv_s"):
            out[name] = getattr(enc.c_w, name)
    for i in range(enc.cfg["layers"]):
        for name, _ in _lib.VitLayer._fields_:
            out[f"{i}.{name}"] = getattr(enc._layers[i], name)
        for name, _ in _lib.TextLayerT._fields_:
            out[f"{i}.t.{name}"] = getattr(enc._layers_t[i], name)
    return out


def test_sync_weights_batched_is_byte_equal_to_sync_weights():
    """masters perturbed (each tensor by its own power of two, so that the scales move apart), then sync_weights(): snapshot.
    Pairs, transposes and scales are then destroyed and
    sync_weights_batched() must restore all of them byte for byte, every struct pointer and scale equal, forward_train
    bit-equal"""
    s, enc = _reduced_encoder("s2_sync")
    imgs = torch.from_numpy(s["imgs"]).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for j, (key, m) in enumerate(enc.masters.items()):
            m.mul_(2.0 ** ((j % 7) - 3)).add_(torch.randn(m.shape, device="cuda", generator=g) * 1e-3)
    enc.sync_weights()
    want_feats = [_bits(t) for t in enc.forward_train(imgs)]
    want_pairs = {k: v.clone() for k, v in enc._pairs.items()}
    want_wt = {k: v.clone() for k, v in enc._wt.items()}
    want_struct = _struct_state(enc)
    assert len(want_pairs) == 1 + 4 * enc.cfg["layers"] and len({want_struct[f"{i}.fc_s"] for i in range(3)} | {want_struct["conv_s"]}) > 1
    for v in list(enc._pairs.values()) + list(enc._wt.values()):
        v.fill_(7.0)
    enc.c_w.conv_s = 0.0
    for i in range(enc.cfg["layers"]):
        for f in ("in_proj_s", "out_proj_s", "fc_s", "proj_s"):
            setattr(enc._layers[i], f, 0.0)
    enc.sync_weights_batched()
    torch.cuda.synchronize()
    assert _struct_state(enc) == want_struct
    for k, v in want_pairs.items():
        assert torch.equal(enc._pairs[k].view(torch.int16), v.view(torch.int16)), k
    for k, v in want_wt.items():
        assert np.array_equal(_bits(enc._wt[k]), _bits(v)), k
    assert all(np.array_equal(_bits(t), w) for t, w in zip(enc.forward_train(imgs), want_feats))


def test_enable_training_adopts_given_masters():
    """masters given as a dict (keys with the model's prefix) ARE the encoder's masters: no clone, an update of them followed by
    sync_weights_batched() changes the features like the same update of a cloning encoder; a wrong dtype or shape is refused"""
    s, enc = _reduced_encoder("s2_adopt_a")
    own = {"image_encoder." + k: v.detach().clone() for k, v in enc.masters.items()}
    other = ops.VitEncoder(s["cfg"], s["sd"], s2.TRAIN["img_hw"], ws_tag="s2_adopt_b")
    got = other.enable_training(own)
    assert all(got[k] is own["image_encoder." + k] for k in got)
    imgs = torch.from_numpy(s["imgs"]).cuda()
    with torch.no_grad():
        for m in list(own.values()) + list(enc.masters.values()):
            m.mul_(1.5)
    enc.sync_weights()
    other.sync_weights_batched()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(enc.forward_train(imgs), other.forward_train(imgs)))
    bad = dict(own)
    bad["image_encoder.proj"] = own["image_encoder.proj"].double()
    with pytest.raises(ValueError, match="proj"):
        other.enable_training(bad)
    del bad["image_encoder.proj"]
    with pytest.raises(KeyError):
        other.enable_training(bad)


# ---- 4. the fused step on the reduced tower -----------------------------------------------------------------------------------
def _trainer(sie, algo, ws_tag):
    """(setup, encoder, head, optimizer, trainer, {name: the trained tensor}, the head's tensors) from train_setup"""
    s, c = s2.train_setup(), s2.TRAIN
    enc = ops.VitEncoder(s["cfg"], s["sd"], c["img_hw"], ws_tag=ws_tag)
    masters = enc.enable_training()
    h = {k: torch.from_numpy(v).cuda() for k, v in s["head"].items() if v.dtype == np.float32}

    def bn(name):
        return dict(weight=h[name + ".weight"], bias=h[name + ".bias"], running_mean=h[name + ".running_mean"],
                    running_var=h[name + ".running_var"], num_batches_tracked=torch.zeros((), dtype=torch.long, device="cuda"))
    bns = bn("bottleneck"), bn("bottleneck_proj")
    head = ops.Stage2Head(h["classifier.weight"], h["classifier_proj.weight"], bns[0], bns[1])
    cv_table = torch.from_numpy(s["cv_table"]).cuda() if sie else None
    tensors = dict(masters)
    tensors.update({k: h[k] for k in hc.PARAMS})       # the never-bound three are IN the optimizer, as in the reference
    if sie:
        tensors["cv_embed"] = cv_table
    base_lr = c["adam_lr"] if algo != "SGD" else c["sgd_lr"]
    groups = [{"params": [t], "lr": base_lr * s2.group_of(k)[0], "weight_decay": s2.group_of(k)[1]} for k, t in tensors.items()]
    opt = ops.TensorOptimizer(groups, algo, betas=(sc.BETA1, sc.BETA2), eps=sc.EPS, momentum=c["sgd_mu"])
    tr = ops.Stage2Trainer(enc, head, opt, h["text"], cv_table=cv_table, sie_coe=c["sie_coe"])
    return s, enc, head, opt, tr, tensors, (h, bns)


def _batch(s, sie):
    return (torch.from_numpy(s["imgs"]).cuda(), torch.from_numpy(s["head"]["target"]).cuda(),
            torch.from_numpy(s["cv_index"]).cuda() if sie else None)


@pytest.mark.parametrize("sie", [False, True], ids=["plain", "sie"])
def test_one_fused_step_against_float64_and_the_single_tensor_kernel(sie):
    """one Stage2Trainer.step (Adam): the loss and every gradient buffer within 2e-5 of float64 (relative error / relative L2;
    the unused row of the SIE table exactly 0); every bound tensor carries the bits of ops.adam_step applied to the trainer's own
    gradient buffer with its group's lr and weight decay; the three never-bound parameters keep their bits; the running
    statistics of BOTH bottlenecks move to the float64 values and both num_batches_tracked are 1; the features of a second
    forward are those of the updated parameters (the re-pack ran).  Measured on an MI355X: loss 6.0e-8 / 2.9e-8 (plain / SIE),
    largest gradient figure 1.41e-5 (ln_post.weight, plain) / 1.23e-6 (SIE)."""
    s, enc, head, opt, tr, tensors, (h, bns) = _trainer(sie, "Adam", "s2_one_" + str(sie))
    want = s2.train_f64(sie, "Adam", 1)
    names = s2.trained_names(sie)
    before = {k: t.detach().clone() for k, t in tensors.items()}
    img, target, idx = _batch(s, sie)
    st = tr.step(img, target, idx, validate=True)
    loss = float(st.loss)
    assert abs(loss - want["losses"][0]) <= s2.BOUND * abs(want["losses"][0]), (loss, want["losses"][0])
    grads = dict(tr.grads, **{k: st.grads[k] for k in s2.HEAD_BOUND})
    assert sorted(grads) == sorted(names)
    worst = ("", 0.0)
    for k in names:
        fig = vg.rel_l2(grads[k], want["grads"][k])
        worst = max(worst, (k, fig), key=lambda x: x[1])
        assert fig <= s2.BOUND, (k, fig)
    print(f"one step (sie={sie}): loss deviation {abs(loss - want['losses'][0]) / abs(want['losses'][0]):.2e}, "
          f"largest gradient figure {worst[1]:.2e} ({worst[0]})")
    if sie:
        assert not grads["cv_embed"][2].any() and grads["cv_embed"][3].any()
    base_lr = s2.TRAIN["adam_lr"]
    for k in names:
        p, m, v = before[k].clone(), torch.zeros_like(before[k]), torch.zeros_like(before[k])
        ops.adam_step(p, grads[k].reshape(p.shape).contiguous(), m, v, 1, base_lr * s2.group_of(k)[0], (sc.BETA1, sc.BETA2), sc.EPS,
                      s2.group_of(k)[1], False)
        assert np.array_equal(_bits(tensors[k]), _bits(p)), k
        assert not np.array_equal(_bits(p), _bits(before[k])), k
    for k in s2.NEVER_BOUND:
        assert np.array_equal(_bits(tensors[k]), _bits(before[k])), k
        assert id(tensors[k]) not in opt.state
    for name, bn in zip(("bottleneck", "bottleneck_proj"), bns):
        assert int(bn["num_batches_tracked"]) == 1
        for n in ("running_mean", "running_var"):
            assert vg.rel_l2(bn[n], want["stats"][f"{name}.{n}"]) <= s2.BOUND, (name, n)
    fresh = ops.VitEncoder(s["cfg"], {k: v.detach().cpu().numpy() for k, v in enc.masters.items()}, s2.TRAIN["img_hw"],
                           ws_tag="s2_fresh")
    cv = s2.TRAIN["sie_coe"] * tensors["cv_embed"][idx] if sie else None
    f_new = enc.forward_train(img, cv)
    assert np.array_equal(_bits(torch.cat(f_new[1:], 1)), _bits(fresh(img, cv)))


def test_one_fused_step_on_uint8_pixels_has_the_bits_of_the_step_on_the_normalised_tensor():
    """step() takes uint8 [B, H, W, 3] as the loader has it after Resize: the forward and the recomputed patch operands of the
    conv1.weight gradient normalise the pixels in their first kernel.  The loss, every gradient buffer and every trained tensor
    after the update carry the bits of a twin trainer stepped on the fp32 tensor ((u8 / 255) - 0.5) / 0.5 made with the same two
    fp32 divisions on the host; and the step moved the parameters"""
    s, enc, head, opt, tr, tensors, _ = _trainer(True, "Adam", "s2_u8")
    _, _, _, _, twin, twin_tensors, _ = _trainer(True, "Adam", "s2_u8_twin")
    img, target, idx = _batch(s, True)
    rng = np.random.default_rng(23)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(img.shape[0], img.shape[2], img.shape[3], 3), dtype=np.uint8))
    x = ((u8.permute(0, 3, 1, 2).float() / 255) - 0.5) / 0.5
    before = {k: t.detach().clone() for k, t in tensors.items()}
    st = tr.step(u8.cuda(), target, idx, validate=True)
    want = twin.step(x.contiguous().cuda(), target, idx, validate=True)
    assert bool(torch.isfinite(st.loss).all())
    assert np.array_equal(_bits(st.loss), _bits(want.loss))
    for k in tr.grads:
        assert np.array_equal(_bits(tr.grads[k]), _bits(twin.grads[k])), k
    assert bool(tr.grads["conv1.weight"].any())
    for k in tensors:
        assert np.array_equal(_bits(tensors[k]), _bits(twin_tensors[k])), k
    for k in s2.trained_names(True):
        assert not np.array_equal(_bits(tensors[k]), _bits(before[k])), k


@pytest.mark.parametrize("algo", ["SGD", "Adam"])
def test_ten_fused_steps_follow_the_float64_curve(algo):
    """ten steps with the SIE table: the loss before each update within 2e-5 (relative) of the float64 loop's; after ten steps of
    SGD every trained tensor within 2e-5 (relative L2) of float64 -- not compared for Adam, whose g / (|g| + eps) is steep at
    zero.  Measured on an MI355X: SGD loss curve 1.65e-7 (7.2247 -> 2.6764), parameters 3.37e-7 (cv_embed); Adam loss curve
    2.54e-7 (7.2247 -> 1.4830)."""
    steps = s2.TRAIN["steps"]
    s, enc, head, opt, tr, tensors, _ = _trainer(True, algo, "s2_ten_" + algo)
    want = s2.train_f64(True, algo, steps)
    img, target, idx = _batch(s, True)
    curve = []
    for _ in range(steps):
        curve.append(tr.step(img, target, idx).loss.clone())
    curve = torch.cat(curve).cpu().numpy().astype(np.float64)
    dev = sc.curve_deviation(curve, want["losses"])
    print(f"{algo}: largest loss deviation over {steps} steps {dev:.2e}; loss {want['losses'][0]:.4f} -> {want['losses'][-1]:.4f}")
    assert dev <= s2.BOUND
    assert want["losses"][-1] < want["losses"][0]
    if algo == "SGD":
        worst = max((vg.rel_l2(tensors[k], want["params"][k]), k) for k in s2.trained_names(True))
        print(f"SGD: largest parameter deviation after {steps} steps {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= s2.BOUND
    sd = opt.state_dict()
    assert all(v["step"] == steps for v in sd["state"].values()) and len(sd["state"]) == len(s2.trained_names(True))


def test_trainer_refuses_other_towers():
    s = s2.train_setup()
    enc = ops.VitEncoder(s["cfg"], s["sd"], s2.TRAIN["img_hw"], precision="fp16", ws_tag="s2_refuse")
    with pytest.raises(NotImplementedError, match="split precision"):
        ops.Stage2Trainer(enc, None, None, torch.zeros(1, 1))


# ---- 5. the model and the loop ------------------------------------------------------------------------------------------------
class _TrainLoader:
    """two batches of eight 32 x 32 images: four identities of two among seven, cameras 0 .. 2"""
    batch_size = 8

    def __init__(self):
        g = torch.Generator().manual_seed(23)
        self.img = torch.randn(16, 3, 32, 32, generator=g)
        self.vid = torch.tensor([3, 0, 6, 6, 1, 3, 0, 1, 2, 5, 5, 4, 2, 4, 6, 6])
        self.cam = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 2, 1, 0, 0])

    def __len__(self):
        return 2

    def __iter__(self):
        for s in (0, 8):
            yield self.img[s:s + 8], self.vid[s:s + 8], self.cam[s:s + 8], torch.zeros(8, dtype=torch.int64)


def _stage2_model(out_dir):
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["INPUT.SIZE_TRAIN", [32, 32], "INPUT.SIZE_TEST", [32, 32], "MODEL.SIE_CAMERA", True,
                         "DATALOADER.SAMPLER", "softmax_triplet", "OUTPUT_DIR", str(out_dir), "DATASETS.EXP_SETTING", "exp"])
    cfg.SOLVER.STAGE2.update(IMS_PER_BATCH=8, WARMUP_ITERS=0, BIAS_LR_FACTOR=2, WEIGHT_DECAY_BIAS=0.0)
    return cfg, mu.make_model(cfg, num_class=7, camera_num=3, view_num=1)


def _adam_f64_device(p0, grads, lr, wd):
    """stage1_cases.adam_f64 over the steps' gradients, in float64 on the device -> the parameter after the last step"""
    p = p0.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lr, wd, b1, b2, eps = (sc.f32(x) for x in (lr, wd, sc.BETA1, sc.BETA2, sc.EPS))
    for step, g in enumerate(grads, 1):
        g = g.double() + wd * p
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        p = p - lr / (1.0 - b1 ** step) * (m / (v.sqrt() / np.sqrt(1.0 - b2 ** step) + eps))
    return p


def test_do_train_stage2_fused_against_autograd_and_checkpoint_round_trip(tmp_path, caplog, monkeypatch):
    """the real ViT-B/16 on 32 x 32 images with the SIE table, one epoch of two batches of eight through do_train_stage2: with
    the TensorOptimizer of make_optimizer_2astage (the fused step) and with torch.optim.Adam(foreach=False) through the
    training-mode forward and make_loss (the autograd path), from the same state.  The two losses of each path agree to 2e-5;
    the total update of the trained parameters is as close to float64 Adam over the path's own gradients as torch's fp32 step
    is to float64 Adam over its own, within the factor 4 of test_adam_twenty_steps_against_torch_optim (a different but
    equally valid rounding order); across the paths all but a sliver of the elements (at most 1 %) agree to 3e-3 of the
    learning rate, as in the stage-1 loop's test; the parameters without a gradient keep their bits on both paths; the
    checkpoint of the loop loads into a fresh model whose .eval() features carry the bits of the trained model's.  Measured on an
    MI355X: losses 35.91782 and 129.18022 on both paths; against float64 Adam fused 2.211e-6, torch 2.213e-6; 9 810 of
    86 054 400 elements apart, a third of every attn.in_proj_bias (the K third: exact gradient 0)."""
    from loss.make_loss import make_loss
    from processor.processor_uniprompt_stage2 import do_train_stage2
    from solver.lr_scheduler import WarmupMultiStepLR
    from solver.make_optimizer_prompt import make_optimizer_2astage
    cfg, m = _stage2_model(tmp_path)
    m.enable_stage2_training()
    loss_fn, center = make_loss(cfg, 7)
    loader = _TrainLoader()
    s2c = cfg.SOLVER.STAGE2
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def sched(opt):
        return WarmupMultiStepLR(opt, s2c.STEPS, s2c.GAMMA, s2c.WARMUP_FACTOR, s2c.WARMUP_ITERS, s2c.WARMUP_METHOD)

    def run(opt, opt_center):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid.train"):
            do_train_stage2(cfg, m, center, loader, [], opt, opt_center, sched(opt), loss_fn, 0, 0, 1, 1, 1, 100)
        return caplog.text

    fused_losses, auto_losses = [], []
    step = ops.Stage2Trainer.step

    fused_grads = []

    def recording(self, *a, **k):
        st = step(self, *a, **k)
        fused_losses.append(float(st.loss))
        g = {("cv_embed" if key == "cv_embed" else "image_encoder." + key): buf.clone() for key, buf in self.grads.items()}
        g.update({key: st.grads[key].clone() for key in s2.HEAD_BOUND})
        fused_grads.append(g)
        return st
    monkeypatch.setattr(ops.Stage2Trainer, "step", recording)
    opt, opt_center = make_optimizer_2astage(cfg, m, center)
    names = [n for n, p in m.named_parameters()]
    assert isinstance(opt, ops.TensorOptimizer) and len(opt.param_groups) == len(names)
    text = run(opt, opt_center)
    assert "fused (mpreid.ops.Stage2Trainer)" in text and "Epoch[1] Iteration[2/2] Loss:" in text and "nan" not in text.lower()
    assert opt.param_groups[0]["lr"] == s2c.BASE_LR and opt.param_groups[0]["initial_lr"] == s2c.BASE_LR
    fused = {k: v.detach().clone() for k, v in m.state_dict().items()}
    no_grad = ("classifier_proj.weight", "bottleneck_proj.weight", "bottleneck_proj.bias", "visual_prompt")
    trained = [n for n in names if n not in no_grad]
    assert sorted(len(v) for v in (opt.state,)) == [len(trained)] and all(v["step"] == 2 for v in opt.state.values())
    assert ops.optim_step_launches(len(trained)) <= 8

    # the checkpoint -> a fresh model -> the same evaluation features
    path = tmp_path / "exp" / "ViT-B-16_1.pth"
    assert path.exists()
    m.eval()
    x, cam = loader.img[:8].cuda(), loader.cam[:8].cuda()
    with torch.no_grad():
        feat = m(x=x, cam_label=cam).clone()
    _, fresh = _stage2_model(tmp_path)
    fresh.load_param(str(path))
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh(x=x, cam_label=cam), feat)
    del fresh

    # the autograd path from the same state
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(start[k])
    params = dict(m.named_parameters())
    topt = torch.optim.Adam([{"params": [params[n]], "lr": s2c.BASE_LR * (2 if "bias" in n else 1),
                              "weight_decay": 0.0 if "bias" in n else s2c.WEIGHT_DECAY} for n in names], foreach=False)
    seen = []
    topt.register_step_pre_hook(lambda o, a, k: seen.append({n: params[n].grad.detach().clone() for n in trained}))

    def recording_loss(*a):
        loss = loss_fn(*a)
        auto_losses.append(float(loss.detach()))
        return loss
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="transreid.train"):
        do_train_stage2(cfg, m, center, loader, [], topt, opt_center, sched(topt), recording_loss, 0, 0, 1, 1, 1, 100)
    assert "autograd step" in caplog.text and len(seen) == 2
    assert all(params[n].grad is None for n in no_grad)
    assert len(fused_losses) == len(auto_losses) == 2
    for a, b in zip(fused_losses, auto_losses):
        assert abs(a - b) <= s2.BOUND * abs(b), (fused_losses, auto_losses)
    # each path's two steps against float64 Adam over ITS OWN gradients: what the step's arithmetic adds, the figure of
    # test_adam_twenty_steps_against_torch_optim.  (Across the paths the gradients differ in their last bits, and Adam's
    # g / (|g| + eps) turns that into a different step wherever |g| is of the order of eps -- the K third of every
    # attn.in_proj_bias, whose exact gradient is 0, is nothing else: the elementwise comparison below.)
    assert len(fused_grads) == 2 and sorted(fused_grads[0]) == sorted(trained)
    num_f = num_h = den = 0.0
    far, total, worst = 0, 0, []
    for n in trained:
        lr, wd = s2c.BASE_LR * (2 if "bias" in n else 1), (0.0 if "bias" in n else s2c.WEIGHT_DECAY)
        p0 = start[n].double()
        want_h = _adam_f64_device(start[n], [g[n] for g in seen], lr, wd) - p0
        want_f = _adam_f64_device(start[n], [g[n].reshape(p0.shape) for g in fused_grads], lr, wd) - p0
        num_f += float(((fused[n].double() - p0) - want_f).pow(2).sum())
        num_h += float(((params[n].detach().double() - p0) - want_h).pow(2).sum())
        den += float(want_h.pow(2).sum())
        assert not torch.equal(fused[n], start[n]), n
        apart = int(((fused[n] - params[n].detach()).abs() > 3e-3 * lr).sum())
        far, total = far + apart, total + p0.numel()
        worst.append((apart / p0.numel(), n))
    fig, host = (num_f / den) ** 0.5, (num_h / den) ** 0.5
    print(f"do_train_stage2: losses fused {fused_losses} autograd {auto_losses}; two steps against float64 Adam: fused {fig:.3e}, "
          f"torch.optim in fp32 {host:.3e}; {far} of {total} elements differ between the paths by more than 3e-3 lr; most: "
          f"{sorted(worst, reverse=True)[:4]}")
    assert fig <= 4 * host
    assert far <= 0.01 * total
    for n in no_grad:
        assert torch.equal(fused[n], start[n]) and torch.equal(params[n].detach(), start[n]), n
    for k in ("bottleneck", "bottleneck_proj"):
        assert int(fused[k + ".num_batches_tracked"]) == 2 and int(m.state_dict()[k + ".num_batches_tracked"]) == 2
        assert vg.rel_l2(fused[k + ".running_mean"], m.state_dict()[k + ".running_mean"]) <= s2.BOUND
