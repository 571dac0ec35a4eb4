"""``make_dataloader(cfg)`` with the reference's return tuple (datasets/make_dataloader.py:111):
(train_loader, train_loader_normal, val_loader, num_query, num_classes, cam_num, view_num).

Only DATASETS.NAMES == 'synthetic' exists here (neither box has Market-1501 / MSMT17 / MMMP; their directory parsers are
out of scope).  The two training loaders are None unless DATASETS.SYNTH_TRAIN > 0 (below).
The synthetic val set keeps the reference's conventions: query images first, then gallery
(:101); batches are (img, pids, camids, camids_tensor, viewids_tensor, img_paths) (:39-43); images
are float32 NCHW in the value range left by Normalize(mean=0.5, std=0.5).

DATASETS.SYNTH_RAW moves val_transforms (:57-61: Resize, ToTensor, Normalize) to the GPU: the loader then yields
a RawImageBatch -- the DECODED uint8 RGB images, any sizes, exactly what PIL hands to T.Resize -- and the model
resizes (bit-exact with Pillow), scales and normalises on the device (mpreid.ops.resize_bilinear_u8 +
VitEncoder.forward_u8).  A real dataset plugs in the same way: decode to uint8 HWC in the workers, collate with
``raw_val_collate_fn``.

DATASETS.SYNTH_TRAIN > 0 (the number of training images) adds the training side in the same shape: ``SyntheticTrainSet``
yields decoded uint8 images, the stage-2 ``TrainLoader`` draws P x K batches with ``datasets.sampler.RandomIdentitySampler``
(DATALOADER.SAMPLER containing 'triplet') or shuffled ones ('softmax') and collates them into a ``RawTrainBatch``, whose
``.to(device)`` runs the reference's train_transforms on the GPU (mpreid.ops.TrainAugment); the stage-1 loader is shuffled and
yields ``RawImageBatch`` es on the val_transforms path.  A real training set plugs in by yielding (decoded uint8 HWC image, pid,
camid, viewid, index or path) and collating with ``raw_train_collate_fn`` / ``raw_normal_collate_fn``.
"""
import numpy as np
import torch

from mpreid import synth


class RawImageBatch(list):
    """A batch of decoded uint8 [h, w, 3] RGB images of possibly different sizes (numpy arrays or tensors).
    ``model(batch, ...)`` runs val_transforms on the GPU.  ``.to(device)`` is a no-op returning self so that the
    reference's ``img = img.to(device)`` line in do_inference keeps working; the upload happens packed, through
    pinned staging buffers, inside the model call."""

    def to(self, *a, **k):
        return self

    @property
    def shape(self):
        return (len(self),)


def raw_val_collate_fn(batch):
    """val_collate_fn (datasets/make_dataloader.py:41-45) for datasets that yield decoded uint8 images"""
    imgs, pids, camids, viewids, img_paths = zip(*batch)
    return (RawImageBatch(imgs), pids, camids, torch.tensor(camids, dtype=torch.int64),
            torch.tensor(viewids, dtype=torch.int64), img_paths)


class RawTrainBatch(RawImageBatch):
    """A stage-2 training batch of decoded uint8 images: ``.to(device)`` runs the reference's train_transforms on the GPU
    (mpreid.ops.TrainAugment.apply: bicubic Resize, flip, pad + crop, ToTensor, Normalize, RandomErasing; the random decisions
    are drawn on the host at that moment, in the reference's order) and returns the fp32 [B, 3, H, W] tensor, so the loop's
    ``img = img.to(device)`` / ``img.shape[0]`` lines work unchanged.  ``sample_ids``: one int64 per image that names the IMAGE
    (its dataset index), the counter of its erase noise."""

    def __init__(self, images, sample_ids, augment=None):
        super().__init__(images)
        self.sample_ids = np.asarray(sample_ids, dtype=np.int64)
        assert self.sample_ids.shape == (len(self),)
        self.augment = augment

    def to(self, *a, **k):
        if self.augment is None:
            raise RuntimeError("RawTrainBatch.to: no augmentation bound; collate with "
                               "functools.partial(raw_train_collate_fn, augment=mpreid.ops.TrainAugment(...))")
        return self.augment.apply(self, self.sample_ids)

    @property
    def shape(self):
        if self.augment is None:
            return (len(self),)
        return (len(self), 3) + tuple(self.augment.size_hw)


def _sample_id(key):
    """the int64 that names an image: an integer index as it is, anything else (a path) through a 64-bit digest of its text"""
    if isinstance(key, (int, np.integer)):
        return int(key)
    import hashlib
    return int.from_bytes(hashlib.blake2b(str(key).encode("utf-8"), digest_size=8).digest(), "little", signed=True)


def raw_train_collate_fn(batch, augment=None):
    """train_collate_fn (datasets/make_dataloader_uniprompt.py:36-44) for datasets that yield decoded uint8 images: items
    (img, pid, camid, viewid, index or path) -> (RawTrainBatch, pids, camids, viewids), the three as int64 tensors"""
    imgs, pids, camids, viewids, keys = zip(*batch)
    return (RawTrainBatch(imgs, [_sample_id(k) for k in keys], augment), torch.tensor(pids, dtype=torch.int64),
            torch.tensor(camids, dtype=torch.int64), torch.tensor(viewids, dtype=torch.int64))


def raw_normal_collate_fn(batch):
    """the same items through val_transforms (the reference's train_set_normal, the stage-1 loader): a RawImageBatch, resized
    with the bilinear filter inside the model call"""
    imgs, pids, camids, viewids, _ = zip(*batch)
    return (RawImageBatch(imgs), torch.tensor(pids, dtype=torch.int64), torch.tensor(camids, dtype=torch.int64),
            torch.tensor(viewids, dtype=torch.int64))


class SyntheticTrainSet:
    """``n_images`` decoded-image stand-ins of ``n_ids`` identities (every identity has at least one): uint8, ragged sizes
    around Market-1501's 128x64, cameras 0..5, view 0.  The number of images per identity is seeded and uneven: when the
    numbers allow it, one identity has fewer than ``num_instance`` images (the sampler then draws with replacement) and one has
    more.  ``train`` is the reference's list of (path, pid, camid, viewid); item i is (image, pid, camid, viewid, i)."""

    def __init__(self, n_images, n_ids, num_instance, seed):
        if not 1 <= n_ids <= n_images:
            raise ValueError(f"SyntheticTrainSet: {n_images} images of {n_ids} identities (DATASETS.SYNTH_TRAIN >= SYNTH_IDS >= 1)")
        self.seed = int(seed)
        rng = np.random.default_rng([self.seed, 20])
        w = rng.random(n_ids) + 0.25
        counts = 1 + rng.multinomial(n_images - n_ids, w / w.sum())
        lo, hi = int(np.argmin(counts)), int(np.argmax(counts))
        if num_instance > 1 and lo != hi and counts[lo] >= num_instance:
            counts[hi] += counts[lo] - (num_instance - 1)
            counts[lo] = num_instance - 1
        pids = rng.permutation(np.repeat(np.arange(n_ids), counts))
        cams = rng.integers(0, 6, size=n_images)
        self.train = [(f"synthetic_train/{i:07d}.jpg", int(pids[i]), int(cams[i]), 0) for i in range(n_images)]
        self.num_train_pids, self.num_train_cams, self.num_train_vids = int(n_ids), 6, 1

    def __len__(self):
        return len(self.train)

    def __getitem__(self, i):
        _, pid, cam, view = self.train[i]
        rng = np.random.default_rng([self.seed, 21, int(i)])
        h, w = int(rng.integers(96, 200)), int(rng.integers(48, 100))
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), pid, cam, view, int(i)


class TrainLoader:
    """A training loader without worker processes: iterates ``sampler`` (e.g. datasets.sampler.RandomIdentitySampler) or, with
    ``shuffle``, a permutation drawn the way torch's RandomSampler draws it (a seed from the global torch generator, then
    ``torch.randperm`` on a generator of that seed), else the dataset's order; cuts the indices into batches of ``batch_size``
    (the last may be short) and hands ``[dataset[i] for i in batch]`` to ``collate``."""

    def __init__(self, dataset, batch_size, sampler=None, shuffle=False, collate=raw_train_collate_fn):
        if sampler is not None and shuffle:
            raise ValueError("TrainLoader: a sampler or shuffle, not both")
        if batch_size < 1:
            raise ValueError("TrainLoader: batch_size >= 1")
        self.dataset, self.batch_size, self.sampler, self.shuffle, self.collate = dataset, int(batch_size), sampler, shuffle, collate

    def _n(self):
        return len(self.sampler) if self.sampler is not None else len(self.dataset)

    def __len__(self):
        return (self._n() + self.batch_size - 1) // self.batch_size

    def _indices(self):
        if self.sampler is not None:
            return [int(i) for i in self.sampler]
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            return torch.randperm(len(self.dataset), generator=g).tolist()
        return list(range(len(self.dataset)))

    def __iter__(self):
        idx = self._indices()
        for s in range(0, len(idx), self.batch_size):
            yield self.collate([self.dataset[i] for i in idx[s:s + self.batch_size]])


def make_train_loaders(cfg):
    """(train_loader_stage2, train_loader_stage1, dataset) over the synthetic training set of DATASETS.SYNTH_TRAIN images: stage 2
    through train_transforms on the GPU with the sampler DATALOADER.SAMPLER names, stage 1 shuffled through val_transforms
    (reference datasets/make_dataloader_uniprompt.py:80-117)"""
    import functools
    from mpreid import ops
    from .sampler import RandomIdentitySampler
    d = cfg.DATASETS
    dataset = SyntheticTrainSet(int(d.SYNTH_TRAIN), int(d.SYNTH_IDS), int(cfg.DATALOADER.NUM_INSTANCE), int(d.SYNTH_SEED))
    augment = ops.TrainAugment(tuple(cfg.INPUT.SIZE_TRAIN), cfg.INPUT.PROB, cfg.INPUT.PADDING, cfg.INPUT.RE_PROB,
                               cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, seed=int(cfg.SOLVER.SEED))
    collate = functools.partial(raw_train_collate_fn, augment=augment)
    batch = int(cfg.SOLVER.STAGE2.IMS_PER_BATCH)
    sampler_name = str(cfg.DATALOADER.SAMPLER)
    if 'triplet' in sampler_name:
        stage2 = TrainLoader(dataset, batch, sampler=RandomIdentitySampler(dataset.train, batch, int(cfg.DATALOADER.NUM_INSTANCE)),
                             collate=collate)
    elif sampler_name == 'softmax':
        stage2 = TrainLoader(dataset, batch, shuffle=True, collate=collate)
    else:
        raise ValueError(f"DATALOADER.SAMPLER {sampler_name!r}: 'softmax' or a name containing 'triplet'")
    stage1 = TrainLoader(dataset, int(cfg.SOLVER.STAGE1.IMS_PER_BATCH), shuffle=True, collate=raw_normal_collate_fn)
    return stage2, stage1, dataset


class SyntheticValLoader:
    def __init__(self, n_query, n_gallery, n_ids, hw, batch, seed, device="cpu", raw=False):
        self.n = n_query + n_gallery
        self.hw, self.batch, self.seed = hw, batch, seed
        rng = np.random.default_rng(seed)
        self.pids = rng.integers(0, n_ids, size=self.n)
        self.camids = rng.integers(0, 6, size=self.n)
        self.device = device
        self.raw = raw

    def _raw_images(self, s, e):
        """decoded-image stand-ins: uint8, heights/widths scattered around Market-1501's 128x64"""
        rng = np.random.default_rng(self.seed * 7919 + s)
        out = []
        for _ in range(s, e):
            h, w = int(rng.integers(96, 200)), int(rng.integers(48, 100))
            out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        return RawImageBatch(out)

    def __len__(self):
        return (self.n + self.batch - 1) // self.batch

    def _batch(self, s, e):
        img = self._raw_images(s, e) if self.raw else \
            torch.from_numpy(synth.synthetic_images(e - s, self.hw[0], self.hw[1], seed=self.seed + s))
        pids = tuple(int(p) for p in self.pids[s:e])
        cams = tuple(int(c) for c in self.camids[s:e])
        return (img, pids, cams, torch.tensor(cams, dtype=torch.int64), torch.zeros(e - s, dtype=torch.int64),
                tuple(f"synthetic/{i:07d}.jpg" for i in range(s, e)))

    def __iter__(self):
        for s in range(0, self.n, self.batch):
            yield self._batch(s, min(self.n, s + self.batch))

    def shard(self, indices):
        """the samples `indices` (ascending global positions) in order: what one rank of a multi-GPU evaluation encodes.
        The images are a function of the unsharded batch they belong to, so the owning batches are generated whole and
        cut; batches without an owned sample are skipped."""
        from processor.processor import select_samples
        want = sorted(indices)
        i = 0
        for s in range(0, self.n, self.batch):
            e = min(self.n, s + self.batch)
            keep = []
            while i < len(want) and want[i] < e:
                keep.append(want[i] - s)
                i += 1
            if keep:
                yield select_samples(self._batch(s, e), keep)


def make_dataloader(cfg):
    if cfg.DATASETS.NAMES != "synthetic":
        raise NotImplementedError(
            f"dataset {cfg.DATASETS.NAMES!r}: directory parsers are out of scope of this build; "
            "use DATASETS.NAMES synthetic or feed R1_mAP_eval / do_inference your own loader")
    d = cfg.DATASETS
    val_loader = SyntheticValLoader(int(d.SYNTH_QUERY), int(d.SYNTH_GALLERY), int(d.SYNTH_IDS),
                                    tuple(cfg.INPUT.SIZE_TEST), int(cfg.TEST.IMS_PER_BATCH), int(d.SYNTH_SEED),
                                    raw=bool(d.get("SYNTH_RAW", False)))
    train_loader_stage2 = train_loader_stage1 = None
    if int(d.get("SYNTH_TRAIN", 0)) > 0:   # the training side: decoded images in, train_transforms on the GPU
        train_loader_stage2, train_loader_stage1, _ = make_train_loaders(cfg)
    return train_loader_stage2, train_loader_stage1, val_loader, int(d.SYNTH_QUERY), int(d.SYNTH_IDS), 6, 1


def vehicleid_trial_splits(pids, trials=10, seed=0):
    """The VehicleID test protocol (reference datasets/vehicleid.py:137-144, looped ten times by test.py:46-63) as DATA:
    a list of `trials` splits (q_idx, g_idx), int64 indices into the pool whose identities are `pids`.  In trial t one
    image of every identity -- drawn with ``np.random.default_rng([seed, t])``, the identities visited in order of first
    appearance in the pool -- is the gallery, all the other images are the queries; both lists ascend in pool order.
    The reference draws with the unseeded global ``random.choice`` while it parses the dataset, so there are no upstream
    bits to match: only the protocol is reproduced, and the same (pids, trials, seed) always gives the same splits."""
    pids = np.asarray(pids)
    if pids.ndim != 1 or pids.size == 0:
        raise ValueError("vehicleid_trial_splits: pids must be a non-empty 1-D sequence")
    if int(trials) < 1:
        raise ValueError("vehicleid_trial_splits: trials must be >= 1")
    _, first, inverse = np.unique(pids, return_index=True, return_inverse=True)
    members = [[] for _ in first]
    for i, u in enumerate(inverse.ravel()):
        members[u].append(i)                                  # ascending pool positions of every identity
    visit = np.argsort(first, kind="stable")                  # identities in order of first appearance
    splits = []
    for t in range(int(trials)):
        rng = np.random.default_rng([int(seed), t])
        in_gallery = np.zeros(pids.size, dtype=bool)
        for u in visit:
            in_gallery[members[u][int(rng.integers(len(members[u])))]] = True
        splits.append((np.nonzero(~in_gallery)[0].astype(np.int64), np.nonzero(in_gallery)[0].astype(np.int64)))
    return splits


def make_trial_dataloader(cfg):
    """(pool_loader, splits, num_classes, cam_num, view_num) for a multi-trial protocol (DATASETS.PROTOCOL): the pool is
    the loader ``make_dataloader`` builds -- the same SYNTH_QUERY + SYNTH_GALLERY images from the same seeds, iterated
    ONCE -- and the trials are index lists into it (TEST.TRIALS of them, from DATASETS.TRIAL_SEED)."""
    protocol = str(cfg.DATASETS.get("PROTOCOL", ""))
    if protocol != "vehicleid":
        raise NotImplementedError(f"DATASETS.PROTOCOL {protocol!r}: only 'vehicleid' has a split generator here; any other "
                                  "protocol hands its own (q_idx, g_idx) lists to do_inference_trials")
    _, _, pool_loader, _, num_classes, cam_num, view_num = make_dataloader(cfg)
    splits = vehicleid_trial_splits(pool_loader.pids, trials=int(cfg.TEST.get("TRIALS", 10)),
                                    seed=int(cfg.DATASETS.get("TRIAL_SEED", 0)))
    return pool_loader, splits, num_classes, cam_num, view_num
