"""The training input path without a GPU: the numpy restatements the GPU tests compare against (Pillow's bicubic resample,
Philox4x32-10), the identity sampler against the reference's index sequences, the host draws of TrainAugment, the training
loaders of make_dataloader, and the argument checks of the two new C entry points.  Cases: tests/train_input_cases.py."""
import ctypes
import random

import numpy as np
import pytest
import torch

import train_input_cases as tc
from mpreid import _lib, ops


@pytest.fixture(scope="module")
def gold(golden):
    return golden("train_input.npz")


def _resize_inputs():
    for name, in_hw, out_hw, seed in tc.RESIZE_CASES:
        yield name, tc.make_image(in_hw[0], in_hw[1], seed), out_hw
    for i, (h, w) in enumerate(tc.RAGGED_SIZES):
        yield f"ragged_{i}", tc.make_image(h, w, tc.RAGGED_SEED + i), tc.RAGGED_OUT


def test_numpy_bicubic_equals_the_golden_byte_for_byte(gold):
    clamped = 0
    for name, img, out_hw in _resize_inputs():
        assert tc.crc(img) == int(gold["crc_" + name]), f"{name}: the seeded input is not the one the golden was made from"
        got = tc.np_resize(img, out_hw, "bicubic")
        assert got.dtype == np.uint8 and np.array_equal(got, gold["bicubic_" + name]), name
        clamped += int(((got == 0) | (got == 255)).sum())
    assert clamped > 1000     # the planted edges do drive the filter into the clamp


def test_numpy_resample_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    for name, img, out_hw in _resize_inputs():
        pil = Image.fromarray(img, "RGB")
        for filt, mode in (("bicubic", Image.BICUBIC), ("bilinear", Image.BILINEAR)):
            assert np.array_equal(tc.np_resize(img, out_hw, filt), np.asarray(pil.resize((out_hw[1], out_hw[0]), mode))), (name, filt)


# ---------------------------------------------------------------- RandomIdentitySampler
def _sampler():
    from datasets.sampler import RandomIdentitySampler
    data = tc.sampler_list()
    return data, RandomIdentitySampler(data, tc.SAMPLER_BATCH, tc.SAMPLER_K)


@pytest.mark.parametrize("seed", tc.SAMPLER_SEEDS)
def test_sampler_yields_the_references_index_sequence(gold, seed):
    data, s = _sampler()
    random.seed(seed)
    np.random.seed(seed)
    got = list(s)
    assert all(type(i) is int or isinstance(i, np.integer) for i in got)
    assert [int(i) for i in got] == gold[f"sampler_{seed}"].tolist()


def test_sampler_groups_batches_and_length():
    data, s = _sampler()
    assert len(s) == tc.sampler_len(data, tc.SAMPLER_K) == 36     # 8 + 4 + 4 + 4 + 8 + 4 + 4
    assert list(s.index_dic) == list(dict.fromkeys(d[1] for d in data))     # first-appearance order
    random.seed(3)
    np.random.seed(3)
    idx = [int(i) for i in s]
    K, B = tc.SAMPLER_K, tc.SAMPLER_BATCH
    assert len(idx) % B == 0 and 0 < len(idx) <= len(s)
    for g in range(0, len(idx), K):
        assert len({data[i][1] for i in idx[g:g + K]}) == 1
    for b in range(0, len(idx), B):
        assert len({data[i][1] for i in idx[b:b + B]}) == B // K
    short = [i for i in idx if data[i][1] == 4]                  # the identity with one image: drawn with replacement
    assert len(short) in (0, K) and len(set(short)) <= 1


# ---------------------------------------------------------------- TrainAugment.draw
def _seed_all(seed):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def test_draw_is_reproducible_and_valid():
    aug = ops.TrainAugment(tc.AUG_HW, flip_p=0.5, pad=3, erase_p=0.5)
    _seed_all(11)
    a = aug.draw(300)
    _seed_all(11)
    b = aug.draw(300)
    _seed_all(12)
    c = aug.draw(300)
    assert a.dtype == np.int32 and a.shape == (300, 8) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert all(tc.row_is_valid(r, tc.AUG_HW[0], tc.AUG_HW[1], 3) for r in a)
    assert set(a[:, 0]) == {0, 1} and a[:, 1].min() == 0 and a[:, 1].max() == 6 and a[:, 2].max() == 6
    big = ops.TrainAugment((256, 128), pad=10)
    _seed_all(13)
    assert all(tc.row_is_valid(r, 256, 128, 10) for r in big.draw(200))


def test_draw_without_erasing_and_without_padding():
    _seed_all(5)
    t = ops.TrainAugment(tc.AUG_HW, flip_p=0.5, pad=3, erase_p=0.0).draw(200)
    assert not t[:, 3:7].any() and t[:, 0].any()
    # pad 0: no crop draw -- the torch generator advances by the flip draws alone
    _seed_all(6)
    t0 = ops.TrainAugment(tc.AUG_HW, flip_p=0.5, pad=0, erase_p=0.5).draw(50)
    after = torch.rand(1).item()
    torch.manual_seed(6)
    flips = [int(bool(torch.rand(1) < 0.5)) for _ in range(50)]
    assert not t0[:, 1:3].any() and t0[:, 0].tolist() == flips and torch.rand(1).item() == after


def test_draw_follows_the_stated_order_of_draws():
    """the flip from torch.rand(1), the crop from two torch.randint, the erase decision and box from `random`: replayed here"""
    import math
    H, W = tc.AUG_HW
    _seed_all(21)
    t = ops.TrainAugment(tc.AUG_HW, flip_p=0.3, pad=2, erase_p=0.7).draw(40)
    _seed_all(21)
    for r in t:
        assert r[0] == int(bool(torch.rand(1) < 0.3))
        assert r[1] == int(torch.randint(0, 5, (1,))) and r[2] == int(torch.randint(0, 5, (1,)))
        box = (0, 0, 0, 0)
        if not random.random() > 0.7:
            for _ in range(10):
                target = random.uniform(0.02, 1 / 3) * H * W
                ar = math.exp(random.uniform(math.log(0.3), math.log(1 / 0.3)))
                h, w = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
                if w < W and h < H:
                    box = (random.randint(0, H - h), random.randint(0, W - w), h, w)
                    break
        assert tuple(r[3:7]) == box


def test_share_of_erased_images():
    n, p = 2000, 0.5
    _seed_all(2024)
    t = ops.TrainAugment(tc.AUG_HW, pad=3, erase_p=p).draw(n)
    share = float((t[:, 5] > 0).mean())
    print(f"erased share {share:.4f} of {n} draws (erase_p {p})")
    assert abs(share - p) < 5 * np.sqrt(p * (1 - p) / n)


# ---------------------------------------------------------------- Philox
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10, on both forms; then the two forms against each other on random inputs"""
    for ctr, key, want in tc.PHILOX_KAT:
        assert tuple(int(v) for v in tc.philox4x32_10(np.array(ctr, np.uint32), key)) == want
        assert tc.philox4x32_10_scalar(ctr, key) == want
    rng = np.random.default_rng(9)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    key = (0x12345678, 0x9ABCDEF0)
    got = tc.philox4x32_10(ctr, key)
    for i in range(64):
        assert tuple(int(v) for v in got[i]) == tc.philox4x32_10_scalar(ctr[i], key)


def test_noise_restatement_moments():
    z = tc.erase_noise_f64(5, 7, 255, 127).ravel()
    n = z.size
    assert n == 97155 and abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((np.abs(z) > 3).mean() - 0.0027) < 5 * np.sqrt(0.0027 * 0.9973 / n)


# ---------------------------------------------------------------- loaders
def _cfg(*opts):
    from config import cfg_base
    c = cfg_base.clone()
    c.defrost()
    c.merge_from_list(["DATASETS.SYNTH_QUERY", 4, "DATASETS.SYNTH_GALLERY", 8, "TEST.IMS_PER_BATCH", 4] + list(opts))
    return c


def test_make_dataloader_training_loaders():
    from datasets.make_dataloader import RawImageBatch, RawTrainBatch, TrainLoader, make_dataloader, raw_train_collate_fn
    c = _cfg()
    assert c.INPUT.PROB == 0.5 and c.INPUT.PADDING == 10 and c.INPUT.RE_PROB == 0.5 and c.DATASETS.SYNTH_TRAIN == 0
    tl, tn = make_dataloader(c)[:2]
    assert tl is None and tn is None
    c = _cfg("DATASETS.SYNTH_TRAIN", 40, "DATASETS.SYNTH_IDS", 7, "DATALOADER.SAMPLER", "softmax_triplet",
             "DATALOADER.NUM_INSTANCE", 4, "SOLVER.STAGE2.IMS_PER_BATCH", 8, "SOLVER.STAGE1.IMS_PER_BATCH", 16)
    tl, tn, _, _, num_classes, cam_num, _ = make_dataloader(c)
    assert isinstance(tl, TrainLoader) and tl.batch_size == 8 and tn.batch_size == 16 and num_classes == 7 and cam_num == 6
    counts = np.bincount([d[1] for d in tl.dataset.train], minlength=7)
    assert counts.sum() == 40 and counts.min() >= 1 and counts.min() < 4 < counts.max()
    assert all(0 <= d[2] <= 5 for d in tl.dataset.train)
    _seed_all(1)
    batches = list(tl)
    assert 0 < len(batches) <= len(tl)
    for img, pids, camids, viewids in batches:
        assert isinstance(img, RawTrainBatch) and img.shape == (8, 3, 256, 128) and img.sample_ids.dtype == np.int64
        assert all(a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 for a in img)
        assert len({a.shape for a in img}) > 1                                  # ragged
        assert pids.dtype == camids.dtype == viewids.dtype == torch.int64 and pids.shape == (8,)
        assert [tl.dataset.train[i][1] for i in img.sample_ids] == pids.tolist()
        assert all(len(set(pids[g:g + 4].tolist())) == 1 for g in (0, 4)) and len(set(pids.tolist())) == 2   # P x K
    seen = []
    for img, pids, camids, viewids in tn:
        assert type(img) is RawImageBatch and img.to("cuda") is img and pids.dtype == torch.int64 and len(img) == len(pids)
        seen += [(a.shape, int(p)) for a, p in zip(img, pids)]
    assert len(tn) == 3 and len(seen) == 40
    assert sorted(seen) == sorted((tl.dataset[i][0].shape, tl.dataset[i][1]) for i in range(40))     # every image once
    shuffled = make_dataloader(_cfg("DATASETS.SYNTH_TRAIN", 40, "DATASETS.SYNTH_IDS", 7, "SOLVER.STAGE2.IMS_PER_BATCH", 8))[0]
    assert sorted(int(i) for b in shuffled for i in b[0].sample_ids) == list(range(40))      # softmax: a permutation
    with pytest.raises(ValueError, match="SAMPLER"):
        make_dataloader(_cfg("DATASETS.SYNTH_TRAIN", 40, "DATASETS.SYNTH_IDS", 7, "DATALOADER.SAMPLER", "other"))
    # the collate function alone: ids from indices or from paths, no augmentation bound -> a clear error
    b = raw_train_collate_fn([(np.zeros((3, 2, 3), np.uint8), 1, 2, 0, 5), (np.zeros((5, 4, 3), np.uint8), 3, 4, 0, "b.jpg")])
    assert b[0].sample_ids[0] == 5 and b[1].tolist() == [1, 3] and b[2].tolist() == [2, 4] and b[0].shape == (2,)
    assert b[0].sample_ids[1] == raw_train_collate_fn([(None, 0, 0, 0, "b.jpg")])[0].sample_ids[0]
    with pytest.raises(RuntimeError, match="augment"):
        b[0].to("cuda")


# ---------------------------------------------------------------- the C entry points refuse bad arguments (nothing is launched)
FAKE = ctypes.c_void_p(0x1000)      # never read: every call below fails its checks first


def _last_error():
    return _lib.load().mpreid_last_error().decode()


def test_resize_u8_refuses_an_unknown_filter_and_a_small_workspace():
    L = _lib.load()
    need = L.mpreid_resize_workspace_bytes(2, 10, 8)
    assert need >= 2 * 10 * 8 * 3
    assert L.mpreid_resize_u8(FAKE, FAKE, FAKE, 2, 10, 16, 8, 2, FAKE, FAKE, need, None) == _lib.ERR_ARG
    assert "filter = 2" in _last_error()
    assert L.mpreid_resize_u8(FAKE, FAKE, FAKE, 2, 10, 16, 8, _lib.RESIZE_BICUBIC, FAKE, FAKE, need - 1, None) == _lib.ERR_WORKSPACE
    assert "workspace too small" in _last_error()
    assert L.mpreid_resize_u8(FAKE, FAKE, FAKE, 0, 10, 16, 8, _lib.RESIZE_BICUBIC, FAKE, FAKE, need, None) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="filter"):
        ops.resize_u8([np.zeros((2, 2, 3), np.uint8)], (4, 4), "lanczos")


def _augment_rc(rows, H=16, W=8, pad=3, std=(0.5, 0.5, 0.5)):
    t = np.ascontiguousarray(rows, np.int32)
    ids = np.arange(len(t), dtype=np.int64)
    m, s = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(*std)
    return _lib.load().mpreid_train_augment_f32(FAKE, len(t), H, W, pad, t.ctypes.data, ids.ctypes.data, 1, m, s, FAKE, None)


@pytest.mark.parametrize("field,col,value", [("flip", 0, 2), ("flip", 0, -1), ("crop_top", 1, 7), ("crop_top", 1, -1),
                                             ("crop_left", 2, 7), ("erase_top", 3, 12), ("erase_top", 3, -1),
                                             ("erase_left", 4, 6), ("erase_h", 5, 16), ("erase_h", 5, -2),
                                             ("erase_w", 6, 8), ("erase_w", 6, 0), ("reserved", 7, 1)])
def test_train_augment_names_the_image_and_the_field(field, col, value):
    """one bad field in row 2 of three otherwise valid rows (a 5 x 3 box at (11, 5): the largest top / left that fit)"""
    rows = [[0, 3, 3, 0, 0, 0, 0, 0], [1, 6, 0, 0, 0, 15, 7, 0], [1, 6, 6, 11, 5, 5, 3, 0]]
    assert all(tc.row_is_valid(r, 16, 8, 3) for r in rows)
    rows[2][col] = value
    assert not tc.row_is_valid(rows[2], 16, 8, 3)
    assert _augment_rc(rows) == _lib.ERR_ARG
    msg = _last_error()
    assert f"params[2].{field}" in msg and f"= {value}" in msg, msg


def test_train_augment_refuses_bad_scalars():
    ok = [[0, 0, 0, 0, 0, 0, 0, 0]]
    assert _augment_rc(ok, pad=-1) == _lib.ERR_ARG
    assert _augment_rc(ok, H=0) == _lib.ERR_ARG
    assert _augment_rc(ok, pad=0, std=(0.5, 0.0, 0.5)) == _lib.ERR_ARG and "std[1]" in _last_error()
    assert _augment_rc([[0, 1, 0, 0, 0, 0, 0, 0]], pad=0) == _lib.ERR_ARG and "params[0].crop_top" in _last_error()
