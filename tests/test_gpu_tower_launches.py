"""The launch sequence of the image, MoE and text towers, as the library's own profile records state it, and the sizes of
their workspaces.  One forward per tower with mpreid_profile_enable(1); the assertion is the full set of
(epilogue, m, n, k, launches, flops_total) that mpreid_profile_query returns (total_ms and the time-sorted order are left
out).  bench.py --full and the tools read these records; every literal below is what the library recorded before the block
driver of csrc/vit.hip existed, and is derived from the config in its comment.

Geometry: test_gpu_vit.SMALL (4 x 2 patches of 16 on a 64 x 32 image, width 128, 2 heads, 2 layers) and a text tower of 17
tokens at the same width, 3 images / prompts.  Two layers is the smallest depth at which the CLS-only tail block differs from
a body block; a batch of 3 keeps B, Bpad, M and Mpad distinct."""
import ctypes as C

import pytest
import torch

from mpreid import _lib, ops, synth

pytestmark = pytest.mark.gpu

SMALL = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)   # test_gpu_vit.SMALL
TEXT = dict(tokens=17, width=128, layers=2, heads=2, out_dim=64)
HW = (64, 32)
B = 3
# What the rows below are made of.  Image towers: L = 4 * 2 + 1 = 9 tokens, M = 3 * 9 = 27 rows, the 24 patch rows and the 27
# token rows both padded to Mpad = 256 (the GEMMs' 256-row tile), the 3 CLS rows of the tail block to Bpad = 128; width W = 128,
# patch GEMM k = 3 * 16 * 16 = 768.  Text tower: M = 3 * 17 = 51 rows, Mpad = 256.  pr = halfs per operand element: 1 in fp16,
# 2 in the split mode, where a GEMM's k is 2 * kdim.  Work figures per launch: an fp16 GEMM 2 m n k, a split GEMM 3 m n k
# (three products over kdim = k / 2); LayerNorm M W (4 + 2 pr) bytes;
# attention (k, v of every row + q and the output of the query rows) = (M 2 W + qrows 2 W) 2 pr bytes; the MoE classes 0.
# Epilogue ids: csrc/gemm_f16.h GemmEpi (1 bias -> fp16, 2 bias + residual, 3 bias + QuickGELU, 4 patch embedding; 10 .. 13 the
# split mode's: 10 bias -> fp32, 11 residual, 12 QuickGELU pair, 13 patch) and include/mpreid.h MPREID_PROF_* (100 LayerNorm,
# 101 attention, 110 .. 114 MoE router, dispatch, FC1, FC2, combine).
SPLIT_PATCH = (13, 256, 128, 1536, 1, 150994944)   # GE_S_PATCH: conv1 over Mpad patch rows, k = 2 * 768; 3 * 256 * 128 * 1536
SPLIT_LN1 = (100, 27, 128, 2, 2, 55296)            # ln_1, (100, M, W, pr) x 2 layers; 2 * 27 * 128 * (4 + 4)
SPLIT_IN_PROJ = (10, 256, 384, 256, 2, 150994944)  # in_proj of both blocks on Mpad rows, n = 3 W; 2 * (3 * 256 * 384 * 256)
SPLIT_ATT_BODY = (101, 27, 0, 2, 1, 55296)         # a body block's attention, n = 0 = every row; (27 * 256 + 27 * 256) * 4
SPLIT_ATT_TAIL = (101, 27, 1, 2, 1, 76800)         # the tail's: the CLS tile, 16 query rows per image; (27 * 256 + 48 * 256) * 4
SPLIT_TAIL_MLP = {
    (11, 128, 128, 256, 1, 12582912),              # the tail's out_proj on Bpad rows; 3 * 128 * 128 * 256
    (12, 128, 512, 256, 1, 50331648),              # the tail's c_fc, n = 4 W; 3 * 128 * 512 * 256
    (11, 128, 128, 1024, 1, 50331648),             # the tail's c_proj, k = 2 * 4 W; 3 * 128 * 128 * 1024
}
EXPECTED = {
    # fp16, cls_only_last: block 0 on every row, block 1 the CLS-only tail
    "fp16": {
        (4, 256, 128, 768, 1, 50331648),           # GE_PATCH: conv1 over Mpad patch rows; 2 * 256 * 128 * 768
        (100, 27, 128, 1, 2, 41472),               # ln_1, (100, M, W, pr) x 2 layers; 2 * 27 * 128 * (4 + 2)
        (1, 256, 384, 128, 2, 50331648),           # in_proj of both blocks; 2 * (2 * 256 * 384 * 128)
        (101, 27, 0, 1, 1, 27648),                 # block 0's attention, every row; (27 * 256 + 27 * 256) * 2
        (101, 27, 1, 1, 1, 38400),                 # the tail's, CLS tile only; (27 * 256 + 48 * 256) * 2
        (2, 256, 128, 128, 1, 8388608),            # block 0's out_proj; 2 * 256 * 128 * 128
        (3, 256, 512, 128, 1, 33554432),           # block 0's c_fc; 2 * 256 * 512 * 128
        (2, 256, 128, 512, 1, 33554432),           # block 0's c_proj; 2 * 256 * 128 * 512
        (2, 128, 128, 128, 1, 4194304),            # the tail's out_proj, c_fc and c_proj at m = Bpad
        (3, 128, 512, 128, 1, 16777216),
        (2, 128, 128, 512, 1, 16777216),
    },
    "split_cls": {
        SPLIT_PATCH, SPLIT_LN1, SPLIT_IN_PROJ, SPLIT_ATT_BODY, SPLIT_ATT_TAIL,
        (11, 256, 128, 256, 1, 25165824),          # block 0's out_proj; 3 * 256 * 128 * 256
        (12, 256, 512, 256, 1, 100663296),         # block 0's c_fc; 3 * 256 * 512 * 256
        (11, 256, 128, 1024, 1, 100663296),        # block 0's c_proj; 3 * 256 * 128 * 1024
    } | SPLIT_TAIL_MLP,
    # cls_only_last = False: both blocks on every row, no class at m = Bpad and no CLS-tile attention
    "split_all": {
        SPLIT_PATCH, SPLIT_LN1, SPLIT_IN_PROJ,
        (101, 27, 0, 2, 2, 110592),                # both attentions on every row; 2 * 55296
        (11, 256, 128, 256, 2, 50331648),          # out_proj, c_fc, c_proj of both blocks: twice block 0's figures above
        (12, 256, 512, 256, 2, 201326592),
        (11, 256, 128, 1024, 2, 201326592),
    },
    # E = 2, K = 1, moe_layers = 1: block 0 routed (its out_proj stays a dense GEMM), block 1 the dense CLS-only tail
    "moe": {
        SPLIT_PATCH, SPLIT_LN1, SPLIT_IN_PROJ, SPLIT_ATT_BODY, SPLIT_ATT_TAIL,
        (11, 256, 128, 256, 1, 25165824),          # block 0's out_proj
        (110, 27, 2, 1, 1, 0),                     # router, dispatch, combine: (m, n, k) = (token rows, E, K)
        (111, 27, 2, 1, 1, 0),
        (114, 27, 2, 1, 1, 0),
        (112, 27, 512, 256, 1, 0),                 # grouped FC1: (token rows, N = 4 W, 2 * kseg = 2 W)
        (113, 27, 128, 1024, 1, 0),                # grouped FC2: (token rows, N = W, 2 * kseg = 8 W)
    } | SPLIT_TAIL_MLP,
    # the text tower: split mode, both blocks on all 51 rows, the causal attention filed as "every row" (n = 0)
    "text": {
        (100, 51, 128, 2, 2, 104448),              # ln_1 x 2 layers; 2 * 51 * 128 * 8
        (10, 256, 384, 256, 2, 150994944),         # the GEMM classes of split_all: Mpad is 256 here too
        (101, 51, 0, 2, 2, 208896),                # 2 * (51 * 256 + 51 * 256) * 4
        (11, 256, 128, 256, 2, 50331648),
        (12, 256, 512, 256, 2, 201326592),
        (11, 256, 128, 1024, 2, 201326592),
    },
}


def _forward(name):
    """name -> a callable that runs ONE forward of that tower"""
    if name == "text":
        enc = ops.TextEncoder(TEXT, synth.text_state_dict(TEXT, seed=21), ws_tag="launches_text")
        prompts = (torch.randn((B, TEXT["tokens"], TEXT["width"]), generator=torch.Generator().manual_seed(1)) * 0.02).cuda()
        return lambda: enc.forward(prompts, [16, 3, 9])
    imgs = torch.from_numpy(synth.synthetic_images(B, HW[0], HW[1], seed=3)).cuda()
    if name == "moe":
        cfg = dict(SMALL, num_experts=2, top_k=1, moe_layers=1)
        enc = ops.VitEncoder(cfg, synth.vit_moe_state_dict(cfg, seed=7), HW, ws_tag="launches_moe")
    else:
        enc = ops.VitEncoder(SMALL, synth.vit_state_dict(SMALL, seed=7, std=0.05, ln_jitter=0.1), HW, ws_tag="launches_" + name,
                             precision="fp16" if name == "fp16" else "split", cls_only_last=name != "split_all")
    return lambda: enc(imgs)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_profile_records_of_one_forward(name):
    L = _lib.load()
    run = _forward(name)
    torch.cuda.synchronize()
    ents = (_lib.ProfileEntry * 64)()
    try:
        L.mpreid_profile_reset()
        L.mpreid_profile_enable(1)
        run()
        torch.cuda.synchronize()
        L.mpreid_profile_enable(0)
        n = L.mpreid_profile_query(ents, 64)
    finally:
        L.mpreid_profile_enable(0)
        L.mpreid_profile_reset()
    assert 0 < n <= 64
    got = [(e.epilogue, e.m, e.n, e.k, e.launches, e.flops_total) for e in list(ents)[:n]]
    print(name, sorted(got))
    assert len(set(got)) == n
    assert set(got) == EXPECTED[name], (sorted(set(got) - EXPECTED[name]), sorted(EXPECTED[name] - set(got)))


def _vit_cfg(cfg, hw, precision):
    return _lib.VitCfg(hw[0], hw[1], cfg["patch"], cfg["stride"], cfg["h_res"], cfg["w_res"], cfg["width"], cfg["layers"],
                       cfg["heads"], cfg["out_dim"], 0, 1, precision)


# (vit fp16, vit split, MoE with E = 2 / K = 1 / one MoE block, all-fp32, text) workspace bytes, as the library answered
# before the layouts shared one cursor.  E.g. SMALL fp16 at B = 3, every piece a multiple of 256 already: patches
# 256 * 768 * 2 + x 256 * 128 * 4 + a 256 * 128 * 2 + qkv 256 * 384 * 2 + hidden 256 * 512 * 2 + the tail's x, a, hidden and
# head rows (128 * 128 * 4, 128 * 128 * 2, 128 * 512 * 2, 128 * 128 * 4) = 1343488
WORKSPACE_BYTES = {
    ("small", 3): (1343488, 2424832, 3411968, 199680, 1181184),
    ("full", 1): (6094848, 10616832, 18487808, 3962880, 4720640),
    ("full", 3): (10420224, 18481152, 30289408, 11888640, 4724736),
    ("full", 508): (1113587712, 2022703104, 3034585856, 2013143040, 722984960),
}


@pytest.mark.parametrize("size,batch", sorted(WORKSPACE_BYTES))
def test_workspace_bytes(size, batch):
    L = _lib.load()
    cfg, hw, tcfg = (SMALL, HW, TEXT) if size == "small" else (synth.VIT_B16, (256, 128), synth.CLIP_TEXT)
    f16, split = _vit_cfg(cfg, hw, _lib.VIT_F16), _vit_cfg(cfg, hw, _lib.VIT_SPLIT)
    moe = _lib.VitMoe(2, 1, 1, None)
    text = _lib.TextCfg(*(tcfg[k] for k in ("tokens", "width", "layers", "heads", "out_dim")))
    got = (L.mpreid_vit_workspace_bytes(C.byref(f16), batch), L.mpreid_vit_workspace_bytes(C.byref(split), batch),
           L.mpreid_vit_workspace_bytes_moe(C.byref(split), C.byref(moe), batch),
           L.mpreid_vit_workspace_bytes_f32(C.byref(split), batch), L.mpreid_text_workspace_bytes(C.byref(text), batch))
    assert got == WORKSPACE_BYTES[(size, batch)]
