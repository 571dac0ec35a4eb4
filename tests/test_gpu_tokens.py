"""GPU tests of the long-token geometries: 256 x 256 inputs give L = 257 tokens at stride 16 and 442 at stride 12 (the
vehicle re-id configs), above the 256 that one workgroup's LDS holds.  The ViT attention streams K / V through LDS there
(fp16 / split modes: attention_long_kernel; fp32 mode: attention_f32_chunked_kernel above L = 320) and the fp16 RN50 tower's
attention pool passes its score table through the workspace.  Checked against the reference's outputs
(tests/golden/vit_tokens.npz, tests/golden/make_goldens_tokens.py), against the oracle over L = 257 ... 1025, for the rows'
independence of batch and position, for the softmax rescale path, end to end, and above the stated bound."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _close(got, want, rel=4e-3, mx=3e-2):   # the fp16-mode bounds of tests/test_gpu_vit.py
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rl2 = np.linalg.norm(got - want) / np.linalg.norm(want)
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    assert rl2 <= rel and np.abs(got - want).max() <= mx and cos.min() >= 0.99999, (rl2, np.abs(got - want).max(), cos.min())
    return rl2


def _vit_cfgs():
    from mpreid import synth
    return dict(synth.VIT_B16, h_res=16, w_res=16), dict(synth.VIT_B16, h_res=21, w_res=21, stride=12)


@pytest.fixture(scope="module")
def gold():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "vit_tokens.npz"))


# ---- against the reference's outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "split", "fp32"])
def test_vit_b16_256x256_matches_reference(gold, prec):
    from mpreid import ops, synth
    c257, c442 = _vit_cfgs()
    imgs = synth.synthetic_images(4, 256, 256, seed=1257)
    sd = synth.vit_state_dict(c257, seed=7, std=0.02, ln_jitter=0.05)
    enc = ops.VitEncoder(c257, sd, (256, 256), precision=prec)
    f = enc(torch.from_numpy(imgs)).cpu().numpy()
    fcv = enc(torch.from_numpy(imgs), cv_emb=torch.from_numpy(gold["b16_257_cv"])).cpu().numpy()
    sd12 = synth.vit_state_dict(c442, seed=8, std=0.02, ln_jitter=0.05)
    f12 = ops.VitEncoder(c442, sd12, (256, 256), precision=prec)(torch.from_numpy(imgs[:2])).cpu().numpy()
    assert f.shape == (4, 1280) and f12.shape == (2, 1280)
    for got, want in ((f, gold["b16_257_feat"]), (fcv, gold["b16_257_feat_cv"]), (f12, gold["b16_442_feat"])):
        if prec == "fp16":
            _close(got, want)
        else:   # split: max |d| <= 5e-5; fp32: the fp32-mode bound of tests/test_gpu_map_parity.py (2e-5 max |d|)
            assert np.abs(got - want).max() <= (5e-5 if prec == "split" else 2e-5), (prec, np.abs(got - want).max())


@pytest.mark.parametrize("prec", ["fp16", "split", "fp32"])
def test_rn50_256x256_matches_reference(gold, prec):
    from mpreid import ops, synth
    cfg = dict(synth.RN50, h_res=16, w_res=16)
    imgs = synth.synthetic_images(3, 256, 256, seed=1258)
    enc = ops.Rn50Encoder(cfg, synth.rn50_state_dict(cfg, seed=11), (256, 256), precision=prec)
    f = enc(torch.from_numpy(imgs)).cpu().numpy()
    want = gold["rn50_257_feat"]
    rel = np.linalg.norm(f - want) / np.linalg.norm(want)
    assert rel <= (5e-3 if prec == "fp16" else 2e-5), (prec, rel)


# ---- L sweep against the oracle (reduced width) ----------------------------------------------------------------------------
SMALL = dict(patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
# every 16-key tile and 64-key block boundary region of the streaming kernel: 257 (one key in the 5th block), tile edges,
# one short of / at / one past every block boundary 320 ... 1024, the stride-12 geometry and the bound
SWEEP = [257, 258, 273, 289, 319, 320, 321, 383, 385, 442, 447, 449, 511, 513, 575, 577, 639, 641, 703, 705, 767, 769,
         831, 833, 895, 897, 959, 961, 1023, 1024, 1025]


def _grid(L):
    """a (h_res, w_res) patch grid with h_res * w_res = L - 1, as square as the factors allow"""
    P = L - 1
    w = max(d for d in range(1, int(P ** 0.5) + 1) if P % d == 0)
    return P // w, w


@pytest.mark.parametrize("L", SWEEP)
def test_vit_token_sweep_vs_oracle(L):
    from mpreid import ops, synth
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05, ln_jitter=0.1)
    imgs = synth.synthetic_images(3, 16 * h, 16 * w, seed=L)
    want = orc.vit_features(sd, cfg, imgs)
    for prec in ("split", "fp32", "fp16"):
        got = ops.VitEncoder(cfg, sd, (16 * h, 16 * w), precision=prec, ws_tag="sweep")(torch.from_numpy(imgs)).cpu().numpy()
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= (4e-3 if prec == "fp16" else 2e-5), (L, prec, rel)
    ops.release_workspaces("sweep")


# ---- the online softmax's rescale path ------------------------------------------------------------------------------------
def _spiked(L, a_mid, a_end):
    """reduced ViT whose first block's scores jump at chosen keys: the q bias is a fixed vector u for every query, and the
    k projection maps residual channel 1 onto a_mid * u and channel 2 onto a_end * u.  The positional embedding puts
    channel 1 high on two tokens in the middle and channel 2 high on the last (up to three) tokens, all in the LAST key block (LayerNorm turns either into
    about sqrt(width)), so the running max of every row jumps in the last key block, after most of the mass."""
    from mpreid import synth
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    sd = synth.vit_state_dict(cfg, seed=5, std=0.05, ln_jitter=0.0)
    W = cfg["width"]
    pos = sd["positional_embedding"].copy()
    last0 = ((L - 1) // 64) * 64   # first key of the last 64-key block
    mid, end = [L // 2, L // 2 + 1], list(range(max(last0, L - 3), L))
    pos[mid, 1] = 40.0
    pos[end, 2] = 40.0
    sd["positional_embedding"] = pos
    inw = sd["transformer.resblocks.0.attn.in_proj_weight"].copy()
    inb = sd["transformer.resblocks.0.attn.in_proj_bias"].copy()
    u = np.zeros(W, np.float32)
    u[0:W:2] = 1.0                # both heads
    inb[:W] = u                   # q = u + small
    inw[W:2 * W, 1] = a_mid * u
    inw[W:2 * W, 2] = a_end * u
    sd["transformer.resblocks.0.attn.in_proj_weight"] = inw
    sd["transformer.resblocks.0.attn.in_proj_bias"] = inb
    return cfg, sd, (16 * h, 16 * w), mid, end


def _first_block_scores(sd, cfg, imgs):
    """scores q.k / 8 of the first block, head 0, on the host (float64): [B, L, L]"""
    import torch as T
    s = cfg["stride"]
    im = T.from_numpy(imgs).double()
    cw = T.from_numpy(sd["conv1.weight"]).double()
    t = T.nn.functional.conv2d(im, cw, stride=s).flatten(2).transpose(1, 2)
    cls = T.from_numpy(sd["class_embedding"]).double()[None, None].expand(t.shape[0], 1, -1)
    x = T.cat([cls, t], 1) + T.from_numpy(sd["positional_embedding"]).double()[None]
    ln = lambda v, g, b: T.nn.functional.layer_norm(v, (v.shape[-1],), T.from_numpy(sd[g]).double(), T.from_numpy(sd[b]).double())
    x = ln(x, "ln_pre.weight", "ln_pre.bias")
    hN = ln(x, "transformer.resblocks.0.ln_1.weight", "transformer.resblocks.0.ln_1.bias")
    qkv = hN @ T.from_numpy(sd["transformer.resblocks.0.attn.in_proj_weight"]).double().t() + \
        T.from_numpy(sd["transformer.resblocks.0.attn.in_proj_bias"]).double()
    W = cfg["width"]
    q, k = qkv[..., :64], qkv[..., W:W + 64]
    return (q @ k.transpose(1, 2) / 8.0).numpy()


@pytest.mark.parametrize("L,a_mid,a_end", [(257, 0.06, 0.22), (442, 0.06, 0.2), (1025, 0.07, 0.25)])
def test_softmax_rescale_path_vs_oracle(L, a_mid, a_end):
    from mpreid import ops
    cfg, sd, hw, mid, end = _spiked(L, a_mid, a_end)
    imgs = np.random.default_rng(L).standard_normal((3, 3) + hw).astype(np.float32) * 0.5
    sc = _first_block_scores(sd, cfg, imgs)
    # the data forces the branch: for every row the maximum over the keys of the last 64-key block exceeds the maximum over
    # all earlier keys by a wide margin, and the earlier keys still carry a visible share of the mass
    last0 = ((L - 1) // 64) * 64
    early, late = sc[:, :, :last0].max(-1), sc[:, :, last0:].max(-1)
    assert (late - early).min() > 2.0, (late - early).min()
    want = orc.vit_features(sd, cfg, imgs)
    for prec in ("split", "fp32", "fp16"):
        got = ops.VitEncoder(cfg, sd, hw, precision=prec, ws_tag="spike")(torch.from_numpy(imgs)).cpu().numpy()
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= (4e-3 if prec == "fp16" else 2e-5), (L, prec, rel)
    ops.release_workspaces("spike")


# ---- bit-identity guarantees at L = 257 and 442 ------------------------------------------------------------------------
@pytest.mark.parametrize("which", [257, 442])
@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_long_token_rows_are_bit_stable(which, prec):
    """CLS-only last block == full last block; rows do not depend on the batch they sit in (ragged batch of 70, position 10);
    two runs give the same bits; a poisoned, stale workspace changes nothing"""
    from mpreid import ops, synth
    c257, c442 = _vit_cfgs()
    cfg = c257 if which == 257 else c442
    sd = synth.vit_state_dict(cfg, seed=7, std=0.02)
    imgs = torch.from_numpy(synth.synthetic_images(4, 256, 256, seed=which)).cuda()
    tail = ops.VitEncoder(cfg, sd, (256, 256), precision=prec, cls_only_last=True, ws_tag="bits")
    full = ops.VitEncoder(cfg, sd, (256, 256), precision=prec, cls_only_last=False, ws_tag="bits_full")
    a = tail(imgs).clone()
    assert torch.equal(full(imgs), a)
    assert torch.equal(tail(imgs), a)   # run to run
    more = torch.from_numpy(synth.synthetic_images(70, 256, 256, seed=99)).cuda()
    more[10:14] = imgs
    assert torch.equal(tail(more)[10:14], a)
    for pat in (0xFF, 0x7B):
        for key, buf in list(ops._ws_cache.items()):
            if key[1] == "bits":
                buf.fill_(pat)
        assert torch.equal(tail(imgs), a), hex(pat)
    ops.release_workspaces("bits")
    ops.release_workspaces("bits_full")


@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_long_token_uint8_input_matches_float_path(prec):
    """uint8 HWC images + fused ToTensor / Normalize == the fp32 entry point fed with the transformed tensor, at L = 257"""
    from mpreid import ops, synth
    c257, _ = _vit_cfgs()
    sd = synth.vit_state_dict(c257, seed=7, std=0.02)
    enc = ops.VitEncoder(c257, sd, (256, 256), precision=prec)
    u8 = np.random.default_rng(0).integers(0, 256, size=(5, 256, 256, 3), dtype=np.uint8)
    mean, std = (0.5, 0.4, 0.45), (0.5, 0.25, 0.3)
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255.0)
    x = (x - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    want = enc(x).cpu().numpy()
    got = enc.forward_u8(torch.from_numpy(u8), mean, std).cpu().numpy()
    assert np.array_equal(got, want)


def test_rn50_long_pool_rows_are_batch_independent():
    """the fp16 tower's pool with the score table in the workspace: rows do not depend on the batch, nor on stale bytes"""
    from mpreid import ops, synth
    cfg = dict(synth.RN50, h_res=16, w_res=16)
    enc = ops.Rn50Encoder(cfg, synth.rn50_state_dict(cfg, seed=11), (256, 256), precision="fp16", ws_tag="rnbits")
    imgs = torch.from_numpy(synth.synthetic_images(3, 256, 256, seed=5)).cuda()
    a = enc(imgs).clone()
    more = torch.from_numpy(synth.synthetic_images(21, 256, 256, seed=6)).cuda()
    more[7:10] = imgs
    assert torch.equal(enc(more)[7:10], a)
    for key, buf in list(ops._ws_cache.items()):
        if key[1] == "rnbits":
            buf.fill_(0xFF)
    assert torch.equal(enc(imgs), a)
    ops.release_workspaces("rnbits")


# ---- above the bound ----------------------------------------------------------------------------------------------------
def test_above_token_bound_is_refused_and_library_still_works():
    from mpreid import ops, synth
    cfg = dict(SMALL, h_res=41, w_res=25)   # L = 1026
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05)
    imgs = torch.from_numpy(synth.synthetic_images(1, 16 * 41, 16 * 25, seed=1))
    for prec in ("fp16", "split", "fp32"):
        with pytest.raises(RuntimeError, match="1025"):
            ops.VitEncoder(cfg, sd, (16 * 41, 16 * 25), precision=prec)(imgs)
    rcfg = dict(synth.RN50, h_res=34, w_res=32)   # 544 x 512: T = 1089
    with pytest.raises(RuntimeError, match="1025"):
        ops.Rn50Encoder(rcfg, synth.rn50_state_dict(rcfg, seed=11), (544, 512), precision="fp16")(
            torch.from_numpy(synth.synthetic_images(1, 544, 512, seed=2)))
    ok = dict(SMALL, h_res=16, w_res=16)
    sd = synth.vit_state_dict(ok, seed=7, std=0.05, ln_jitter=0.1)
    imgs = synth.synthetic_images(2, 256, 256, seed=3)
    got = ops.VitEncoder(ok, sd, (256, 256), precision="split")(torch.from_numpy(imgs)).cpu().numpy()
    want = orc.vit_features(sd, ok, imgs)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 2e-5


# ---- end to end: make_model -> do_inference -> R1_mAP_eval at 256 x 256 -----------------------------------------------
@pytest.mark.parametrize("name", ["ViT-B-16", "RN50"])
def test_end_to_end_256x256_matches_oracle_pipeline(name):
    from config import cfg_base
    from datasets.make_dataloader import make_dataloader
    from model.make_model import make_model
    from processor.processor import do_inference
    from utils.metrics import R1_mAP_eval
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.NAME", name, "MODEL.ENCODER_PRECISION", "split", "INPUT.SIZE_TRAIN", [256, 256],
                         "INPUT.SIZE_TEST", [256, 256], "DATASETS.NAMES", "synthetic", "DATASETS.SYNTH_QUERY", 64,
                         "DATASETS.SYNTH_GALLERY", 192, "DATASETS.SYNTH_IDS", 40, "TEST.IMS_PER_BATCH", 128])
    cfg.freeze()
    _, _, val_loader, num_query, num_classes, cam_num, view_num = make_dataloader(cfg)
    model = make_model(cfg, num_class=num_classes, camera_num=cam_num, view_num=view_num)
    assert model.encode_group == (256 if name == "RN50" else 255)
    r1, _ = do_inference(cfg, model, val_loader, num_query)
    ev = R1_mAP_eval(num_query, feat_norm=cfg.TEST.FEAT_NORM)
    ev.reset()
    feats, pids = [], []
    sd = {k[len("image_encoder."):]: v.cpu().numpy() for k, v in model.state_dict().items() if k.startswith("image_encoder.")}
    for img, pid, camid, camids, views, paths in val_loader:
        ev.update((model(img.cuda()), pid, camid))
        if name == "RN50":
            feats.append(orc.rn50_features(sd, model.rn_cfg, img.numpy()))
        else:
            feats.append(orc.vit_features(sd, model.vit_cfg, img.numpy()))
        pids.extend(pid)
    cmc, mAP = ev.compute()[:2]
    assert float(cmc[0]) == float(r1)
    feats, pids = np.concatenate(feats), np.asarray(pids)
    fn = orc.l2_normalize(feats)
    cmc_or, map_or = orc.eval_func(orc.euclidean_distance(fn[:num_query], fn[num_query:]), pids[:num_query], pids[num_query:])
    assert abs(mAP - map_or) <= 1e-4 and abs(float(cmc[0]) - float(cmc_or[0])) <= 1e-4, (name, mAP, map_or, cmc[0], cmc_or[0])
