"""The training input path on the GPU: the bicubic resize against Pillow's bytes, the augmentation kernel against its numpy
restatement (bitwise outside the erase box, 2e-5 inside), the noise's moments, the 64-per-launch chunking, TrainAugment.apply on
a ragged RawTrainBatch, and train_uniprompt.main end to end.  Cases and restatements: tests/train_input_cases.py.

The bound inside the box: u1 and u2 are exact in fp32; a 1-2 ulp logf at -2 ln u1 <= 33.3 moves r <= 5.8 by about 2e-6; the
angle is handed to sincospif exactly, so what remains is the 1-2 ulp of sine / cosine and of the product, below 1e-6 at
|z| <= 5.8; 2e-5 leaves more than a fourfold margin.  Measured on an MI355X: at most 2.8e-7 over the 16 x 8
cases, 4.0e-7 over the 97 155 values of the large box (largest |z| there 4.64)."""
import logging
import random
import re

import numpy as np
import pytest
import torch

import train_input_cases as tc
from mpreid import ops

pytestmark = pytest.mark.gpu
NOISE_TOL = 2e-5
NORMS = [((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("train_input.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- resize
def test_bicubic_resize_equals_pillow_on_every_shape(gold):
    for name, in_hw, out_hw, seed in tc.RESIZE_CASES:
        img = tc.make_image(in_hw[0], in_hw[1], seed)
        got = ops.resize_u8([img], out_hw, "bicubic")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + tuple(out_hw) + (3,)
        assert np.array_equal(got[0].cpu().numpy(), gold["bicubic_" + name]), name


def test_bicubic_resize_of_a_ragged_batch_in_one_call(gold):
    imgs = [tc.make_image(h, w, tc.RAGGED_SEED + i) for i, (h, w) in enumerate(tc.RAGGED_SIZES)]
    got = ops.resize_u8(imgs, tc.RAGGED_OUT, "bicubic").cpu().numpy()
    for i in range(len(imgs)):
        assert np.array_equal(got[i], gold[f"bicubic_ragged_{i}"]), i
    packed = ops.upload_raw_images([torch.from_numpy(a) for a in imgs])     # tensors, and an already packed batch
    assert np.array_equal(ops.resize_u8(packed, tc.RAGGED_OUT, "bicubic").cpu().numpy(), got)


def test_bilinear_filter_is_byte_equal_to_resize_bilinear_u8():
    imgs = [tc.make_image(h, w, tc.RAGGED_SEED + i) for i, (h, w) in enumerate(tc.RAGGED_SIZES)] + [tc.make_image(1, 1, 1)]
    for out_hw in (tc.RAGGED_OUT, (256, 128), (3, 2)):
        a, b = ops.resize_u8(imgs, out_hw, "bilinear"), ops.resize_bilinear_u8(imgs, out_hw)
        assert torch.equal(a, b)
        assert np.array_equal(a[1].cpu().numpy(), tc.np_resize(imgs[1], out_hw, "bilinear"))
        assert not torch.equal(a, ops.resize_u8(imgs, out_hw, "bicubic"))


# ---------------------------------------------------------------- the augmentation kernel
def _check_batch(got, imgs, table, pad, mean, std, seed, ids):
    """got fp32 [B, 3, H, W] against the restatement -> the largest deviation inside the boxes"""
    worst = 0.0
    for b in range(len(imgs)):
        want, mask, noise = tc.np_augment(imgs[b], table[b], pad, mean, std, seed, ids[b])
        g = got[b]
        assert np.array_equal(_bits(g[:, ~mask]), _bits(want[:, ~mask])), (b, table[b].tolist())
        if noise is not None:
            eh, ew = int(table[b][5]), int(table[b][6])
            dev = np.abs(g[:, mask].reshape(3, eh, ew).astype(np.float64) - noise).max()
            assert dev < NOISE_TOL, (b, dev)
            worst = max(worst, float(dev))
    return worst


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("norm", [0, 1])
def test_augment_kernel_against_the_numpy_restatement(pad, norm):
    H, W = tc.AUG_HW
    mean, std = NORMS[norm]
    rng = np.random.default_rng(100 + pad)
    imgs = rng.integers(0, 256, (6, H, W, 3), dtype=np.uint8)
    ids = np.array([3, 1 << 40, -5, 0, 77, 2 ** 63 - 1], np.int64)
    dev_imgs = torch.from_numpy(imgs).cuda()
    worst = 0.0
    for table in tc.aug_tables(pad):
        assert all(tc.row_is_valid(r, H, W, pad) for r in table)
        got = ops.train_augment(dev_imgs, pad, table, ids, 0xDEADBEEF12345678, mean, std)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, 3, H, W)
        again = ops.train_augment(dev_imgs, pad, table, ids, 0xDEADBEEF12345678, mean, std)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))              # two runs, the same bits
        worst = max(worst, _check_batch(got.cpu().numpy(), imgs, table, pad, mean, std, 0xDEADBEEF12345678, ids))
    if pad:   # the pad ring of the crop at (0, 0): uint8 0 through the same arithmetic
        got = ops.train_augment(dev_imgs, pad, tc.aug_tables(pad)[0], ids, 1, mean, std).cpu().numpy()
        ring = ((np.float32(0) / np.float32(255) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).astype(np.float32)
        for c in range(3):
            assert (_bits(got[2, c, :pad, :]) == _bits(ring[c])).all() and (_bits(got[2, c, :, :pad]) == _bits(ring[c])).all()
            assert (_bits(got[3, c, H - pad:, :]) == _bits(ring[c])).all()
    print(f"augment pad {pad} norm {norm}: largest deviation inside the boxes {worst:.3e}")


def test_noise_depends_on_seed_sample_id_and_box_only():
    H, W = tc.AUG_HW
    rng = np.random.default_rng(7)
    one = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    other = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    imgs = np.concatenate([one[None], other[:3], one[None], other[3:]])              # the image at positions 0 and 4
    row = [1, 2, 4, 2, 1, 9, 5, 0]
    table = np.array([row, [0, 3, 3, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 2, 2, 0], [1, 6, 6, 0, 0, 0, 0, 0], row, row, row], np.int32)
    ids = np.array([42, 1, 2, 3, 42, 43, 42], np.int64)
    imgs[5], imgs[6] = one, one
    a = ops.train_augment(torch.from_numpy(imgs).cuda(), 3, table, ids, 99).cpu().numpy()
    b = ops.train_augment(torch.from_numpy(imgs).cuda(), 3, table, ids, 100).cpu().numpy()
    box = (slice(None), slice(2, 11), slice(1, 6))
    assert np.array_equal(_bits(a[0]), _bits(a[4])) and np.array_equal(_bits(a[0]), _bits(a[6]))     # same id: same bits
    assert not np.array_equal(_bits(a[0][box]), _bits(a[5][box]))                                      # another sample id
    assert not np.array_equal(_bits(a[0][box]), _bits(b[0][box]))                                      # another seed
    out = np.ones(a[0].shape, bool)
    out[box] = False
    assert np.array_equal(_bits(a[0][out]), _bits(a[5][out])) and np.array_equal(_bits(a[0][out]), _bits(b[0][out]))


def test_noise_moments_on_one_large_box():
    seed, sid, H, W = 5, 7, 256, 128
    ref = tc.erase_noise_f64(seed, sid, H - 1, W - 1)
    n = ref.size

    def check(z):
        z = np.asarray(z, np.float64).ravel()
        assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
        assert abs((np.abs(z) > 3).mean() - 0.0027) < 5 * np.sqrt(0.0027 * 0.9973 / n)
    assert n == 97155
    check(ref)                                                                    # the chosen seed passes on the restatement
    img = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    got = ops.train_augment(img, 0, np.array([[0, 0, 0, 1, 1, H - 1, W - 1, 0]], np.int32), [sid], seed).cpu().numpy()
    z = got[0, :, 1:, 1:]
    check(z)
    dev = float(np.abs(z - ref).max())
    print(f"noise on a 255 x 127 box: largest deviation from float64 {dev:.3e}, largest |z| {np.abs(z).max():.3f}")
    assert dev < NOISE_TOL
    assert (got[0, :, 0, :] == -1.0).all() and (got[0, :, :, 0] == -1.0).all()    # outside the box: (0 / 255 - 0.5) / 0.5


def test_a_batch_of_70_is_bit_equal_to_64_plus_6():
    H, W, pad = tc.AUG_HW[0], tc.AUG_HW[1], 3
    rng = np.random.default_rng(70)
    imgs = torch.from_numpy(rng.integers(0, 256, (70, H, W, 3), dtype=np.uint8)).cuda()
    torch.manual_seed(70)
    random.seed(70)
    table = ops.TrainAugment((H, W), pad=pad, erase_p=0.7).draw(70)
    assert (table[64:, 5] > 0).any() and (table[:64, 5] > 0).any()
    ids = np.arange(1000, 1070, dtype=np.int64)
    whole = ops.train_augment(imgs, pad, table, ids, 8)
    parts = torch.cat([ops.train_augment(imgs[:64], pad, table[:64], ids[:64], 8),
                       ops.train_augment(imgs[64:], pad, table[64:], ids[64:], 8)])
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    assert not torch.equal(whole[5], whole[69])


def test_table_errors_launch_nothing_on_the_device():
    H, W = tc.AUG_HW
    imgs = torch.zeros((66, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((66, 3, H, W), 7.0, device="cuda")
    table = np.zeros((66, 8), np.int32)
    table[65, 5:7] = (H, 1)                        # the bad row sits in the SECOND launch's chunk
    with pytest.raises(RuntimeError, match=r"params\[65\]\.erase_h"):
        ops.train_augment(imgs, 0, table, np.arange(66), 1, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_train_augment_apply_on_a_ragged_raw_train_batch():
    from datasets.make_dataloader import RawTrainBatch
    H, W, pad = 32, 16, 2
    mean, std = NORMS[1]
    imgs = [tc.make_image(h, w, 60 + i) for i, (h, w) in enumerate(tc.RAGGED_SIZES)]
    ids = np.array([11, 12, 13, 14, 15], np.int64)
    aug = ops.TrainAugment((H, W), flip_p=0.5, pad=pad, erase_p=0.8, mean=mean, std=std, seed=314)
    torch.manual_seed(4)
    random.seed(4)
    table = aug.draw(5)
    assert (table[:, 5] > 0).any() and table[:, 0].any()
    batch = RawTrainBatch(imgs, ids, aug)
    got = aug.apply(batch, ids, params=table)
    assert tuple(got.shape) == batch.shape == (5, 3, H, W) and got.is_cuda and got.dtype == torch.float32
    resized = np.stack([tc.np_resize(a, (H, W), "bicubic") for a in imgs])
    worst = _check_batch(got.cpu().numpy(), resized, table, pad, mean, std, 314, ids)
    torch.manual_seed(4)
    random.seed(4)
    drawn = batch.to("cuda")                        # the loop's call: the same draws, the same tensor
    assert torch.equal(drawn.view(torch.int32), got.view(torch.int32))
    print(f"TrainAugment.apply: largest deviation inside the boxes {worst:.3e}")


# ---------------------------------------------------------------- end to end
def _main_opts(out_dir, checkpoints):
    period = 1 if checkpoints else 100
    opts = ["INPUT.SIZE_TRAIN", "[32, 32]", "INPUT.SIZE_TEST", "[32, 32]", "INPUT.PADDING", "2", "DATASETS.SYNTH_TRAIN", "32",
            "DATASETS.SYNTH_IDS", "4", "DATASETS.SYNTH_QUERY", "8", "DATASETS.SYNTH_GALLERY", "16", "DATASETS.SYNTH_RAW", "True",
            "TEST.IMS_PER_BATCH", "8", "DATALOADER.SAMPLER", "softmax_triplet", "DATALOADER.NUM_INSTANCE", "4",
            "SOLVER.SEED", "77", "OUTPUT_DIR", str(out_dir), "DATASETS.EXP_SETTING", "exp",
            "SOLVER.STAGE2.IMS_PER_BATCH", "8", "SOLVER.STAGE2.MAX_EPOCHS", "1", "SOLVER.STAGE2.LOG_PERIOD", "1",
            "SOLVER.STAGE2.CHECKPOINT_PERIOD", str(period), "SOLVER.STAGE2.EVAL_PERIOD", "100", "SOLVER.STAGE2.WARMUP_ITERS", "0"]
    for s in ("STAGE1", "STAGE1A", "STAGE1B"):
        opts += [f"SOLVER.{s}.IMS_PER_BATCH", "16", f"SOLVER.{s}.MAX_EPOCHS", "1", f"SOLVER.{s}.LOG_PERIOD", "1",
                 f"SOLVER.{s}.CHECKPOINT_PERIOD", str(period), f"SOLVER.{s}.WARMUP_EPOCHS", "0"]
    return opts


def test_train_uniprompt_main_runs_every_stage(tmp_path, caplog, monkeypatch):
    """the real ViT-B/16 on 32 x 32: 32 synthetic images of 4 identities, 2 x 4 batches, one epoch per stage, PADDING 2"""
    import os
    import train_uniprompt
    # main() selects the device through the environment when nothing has (os.environ.setdefault): keep that out of the tests that
    # run after this one and start ranks of their own
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))

    def run(out_dir, checkpoints):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="transreid"):
            res = train_uniprompt.main(_main_opts(out_dir, checkpoints))
        return res, caplog.text

    res, text = run(tmp_path / "a", True)
    assert len(res) == 2 and all(np.isfinite(float(v)) for v in res)
    for marker in ("Start training stage 1a", "Start training stage 1b", "2a stage", "2b stage", "fused (mpreid.ops.Stage2Trainer)",
                   "Enter inferencing", "Validation Results"):
        assert marker in text, marker
    assert text.count("start training") == 2
    stage2 = [float(v) for v in re.findall(r"Iteration\[\d+/\d+\] Loss: ([-\w.]+), Acc", text)]
    stage1 = [float(v) for v in re.findall(r"Iteration\[\d+/\d+\] Loss: ([-\w.]+), Base", text)]
    assert len(stage1) == 4 and len(stage2) >= 4 and np.isfinite(stage1 + stage2).all(), (stage1, stage2)
    for f in ("ViT-B-16_stage1a_1.pth", "ViT-B-16_stage1b_1.pth", os.path.join("exp", "ViT-B-16_1.pth"),
              os.path.join("exp", "train_log.txt")):
        assert os.path.getsize(tmp_path / "a" / f) > 0, f
    _, text2 = run(tmp_path / "b", False)
    again = [float(v) for v in re.findall(r"Iteration\[\d+/\d+\] Loss: ([-\w.]+), Acc", text2)]
    print(f"train_uniprompt.main: stage-1 losses {stage1}, stage-2 losses {stage2}, (rank1, rank5) {res}")
    assert again == stage2
