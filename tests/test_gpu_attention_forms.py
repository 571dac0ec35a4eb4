"""GPU tests of every attention kernel form below 257 tokens.  The encoder picks its attention kernel from the token count L
(attention_dispatch / attention_split_dispatch in csrc/attention.hip), keyed on kt = ceil(L / 16):

    fp16   attention_kernel<2,2,EXACT> L 2..32 | <10,4,MASKALL> 33..128 | <10,4,EXACT> 129..160 | <14,8,MASKALL> 161..192 |
           <14,8,EXACT> 193..224 | <16,8,EXACT> 225..256
    split  attention_split_kernel<2,2> 2..32 | <8,4,XKEY> 129 only | <10,8> 33..160 except 129 | <14,8> 161..224 | <16,8> 225..256
    fp32   attention_f32_kernel 2..320
    L > 256: attention_long_kernel<fp16 | split>

1. a sweep of L over both sides of every edge of that table, on plain random data, against the oracle;
2. the same on data where ONE key carries about a third of every softmax row, so that a key mask that is off by one (the key
   dropped, or counted twice through the clamped copy of row L - 1 that sits behind it in LDS) moves the features by many times
   the fp16 bound -- asserted on the host, in float64, before the GPU is touched;
3. proof (MPREID_TUNE=verbose=1 in a child process) that the chosen L reach the instantiations of the table;
4. the persistent loop of every instantiation wrapped: a batch larger than the largest grid gives the bits of a batch of 8;
5. widths 256 / 512 / 1024 and patch 8 / 32, which vit_check_cfg admits and nothing else runs;
6. the RN50 attention pool on both sides of the switch from the LDS-resident score table to the workspace."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_gpu_tokens import SMALL, _first_block_scores, _grid

pytestmark = pytest.mark.gpu

# the lowest and highest L of every row of the table, both sides of every 16-key tile edge where the instantiation or EXACT
# changes, real geometries (224 x 112: 99, 256 x 128: 129, 224 x 224: 197, 384 x 128: 193, stride 12: 211, 256 x 240: 241)
# and 256, the last resident length
SHORT = [2, 3, 16, 17, 31, 32, 33, 48, 49, 99, 127, 128, 129, 130, 144, 145, 159, 160, 161, 176, 177, 191, 192, 193,
         197, 208, 209, 211, 223, 224, 225, 239, 240, 241, 255, 256]
# one L per row of the table (fp16 row, split row): <2,2>; <10,4,MASKALL>, <10,8>; <10,4,EXACT>, <8,4,XKEY>; <10,4,EXACT>, <10,8>;
# <14,8,MASKALL>, <14,8>; <14,8,EXACT>, <14,8>; <16,8,EXACT>, <16,8>.  None but 129 is of the form 16 n + 1, so the first key of
# the last key tile is not the last key
ROWS = [31, 99, 129, 159, 191, 211, 255]
BOUND = {"fp16": 4e-3, "split": 2e-5, "fp32": 2e-5}   # the bounds of test_vit_token_sweep_vs_oracle


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _check_precisions(tag, cfg, sd, hw, imgs, want):
    """the three precision modes against `want`; every figure is printed before anything is asserted"""
    from mpreid import ops
    rels = {}
    for prec in ("split", "fp32", "fp16"):
        got = ops.VitEncoder(cfg, sd, hw, precision=prec, ws_tag="forms")(torch.from_numpy(imgs)).cpu().numpy()
        assert got.shape == want.shape and np.isfinite(got).all(), (tag, prec)
        rels[prec] = _rel(got, want)
        print("FORMS %s prec=%s rel=%.3e" % (tag, prec, rels[prec]))
    ops.release_workspaces("forms")
    ops.release_workspaces("forms_f32")
    for prec, rel in rels.items():
        assert rel <= BOUND[prec], (tag, prec, rel)


# ---- 1. short-token sweep on plain data ------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SHORT)
def test_short_token_sweep_vs_oracle(L):
    from mpreid import synth
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05, ln_jitter=0.1)
    imgs = synth.synthetic_images(3, 16 * h, 16 * w, seed=L)
    _check_precisions("plain L=%d" % L, cfg, sd, (16 * h, 16 * w), imgs, orc.vit_features(sd, cfg, imgs))


# ---- 2. one spiked key ----------------------------------------------------------------------------------------------------
def _features_f64(sd, cfg, imgs, mutate=None):
    """the encoder's graph in float64 on the host (the graph of oracle.vit_features); `mutate`, if given, maps the scaled scores
    [B, heads, L, L] of block 0 to the ones the softmax sees"""
    F = torch.nn.functional
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).double()  # noqa: E731
    w, heads, p, s = cfg["width"], cfg["heads"], cfg["patch"], cfg["stride"]
    x = T(imgs)
    B = x.shape[0]
    tok = F.unfold(x, kernel_size=p, stride=s).transpose(1, 2) @ T(sd["conv1.weight"]).reshape(w, -1).t()
    x = torch.cat([T(sd["class_embedding"]).expand(B, 1, w), tok], 1) + T(sd["positional_embedding"])
    ln = lambda v, name: F.layer_norm(v, (w,), T(sd[name + ".weight"]), T(sd[name + ".bias"]), 1e-5)  # noqa: E731
    x = ln(x, "ln_pre")
    L = x.shape[1]
    for i in range(cfg["layers"]):
        b = "transformer.resblocks.%d" % i
        qkv = ln(x, b + ".ln_1") @ T(sd[b + ".attn.in_proj_weight"]).t() + T(sd[b + ".attn.in_proj_bias"])
        q, k, v = (t.reshape(B, L, heads, 64).transpose(1, 2) for t in qkv.split(w, dim=2))
        sc = q @ k.transpose(2, 3) / 8.0
        if mutate is not None and i == 0:
            sc = mutate(sc)
        a = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, L, w)
        x = x + a @ T(sd[b + ".attn.out_proj.weight"]).t() + T(sd[b + ".attn.out_proj.bias"])
        hid = ln(x, b + ".ln_2") @ T(sd[b + ".mlp.c_fc.weight"]).t() + T(sd[b + ".mlp.c_fc.bias"])
        x = x + (hid * torch.sigmoid(1.702 * hid)) @ T(sd[b + ".mlp.c_proj.weight"]).t() + T(sd[b + ".mlp.c_proj.bias"])
    x12 = ln(x[:, 0], "ln_post")
    return torch.cat([x12, x12 @ T(sd["proj"])], 1).numpy()


def _one_spike(L, key):
    """the reduced ViT of test_gpu_tokens._spiked with ONE spiked key: every query is u + small (q bias u: every second
    channel 1, both heads), the k projection maps residual channel 2 onto a_end * u, and the positional embedding puts channel
    2 high on token `key` alone (LayerNorm turns that into about sqrt(width)).  The key's score is about 45 a_end above the
    others', so a_end = 1.1 ln(0.67 (L - 1)) / 45 gives it about a third of every row: where dropping the key and counting it
    twice both change the row most."""
    from mpreid import synth
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    sd = synth.vit_state_dict(cfg, seed=5, std=0.05, ln_jitter=0.0)
    W = cfg["width"]
    a_end = 1.1 * math.log(0.67 * (L - 1)) / 45.0
    pos = sd["positional_embedding"].copy()
    pos[key, 2] = 40.0
    sd["positional_embedding"] = pos
    inw = sd["transformer.resblocks.0.attn.in_proj_weight"].copy()
    inb = sd["transformer.resblocks.0.attn.in_proj_bias"].copy()
    u = np.zeros(W, np.float32)
    u[0:W:2] = 1.0
    inb[:W] = u
    inw[W:2 * W, 2] = a_end * u
    sd["transformer.resblocks.0.attn.in_proj_weight"] = inw
    sd["transformer.resblocks.0.attn.in_proj_bias"] = inb
    return cfg, sd, (16 * h, 16 * w)


def _spiked_key_case(L, key):
    cfg, sd, hw = _one_spike(L, key)
    imgs = np.random.default_rng(L).standard_normal((3, 3) + hw).astype(np.float32) * 0.5
    # preconditions, float64 on the host: the spiked key holds a middling share of the rows of head 0 ...
    sc = torch.from_numpy(_first_block_scores(sd, cfg, imgs))
    share = torch.softmax(sc, -1)[:, :, key].numpy()
    med = float(np.median(share))
    # ... and a kernel that drops it, or counts it twice (logit + ln 2), in block 0 moves the FEATURES by at least 2e-2 = five
    # times the loosest bound under test
    want64 = _features_f64(sd, cfg, imgs)

    def drop(s):
        s = s.clone()
        s[..., key] = -float("inf")
        return s

    def twice(s):
        s = s.clone()
        s[..., key] += math.log(2.0)
        return s
    d_drop, d_twice = _rel(_features_f64(sd, cfg, imgs, drop), want64), _rel(_features_f64(sd, cfg, imgs, twice), want64)
    print("FORMS spiked L=%d key=%d share median %.3f min %.3f, mutants drop %.3e twice %.3e" % (L, key, med, share.min(), d_drop,
                                                                                                  d_twice))
    assert 0.2 <= med <= 0.6, (L, key, med)
    assert d_drop >= 2e-2 and d_twice >= 2e-2, (L, key, d_drop, d_twice)
    want = orc.vit_features(sd, cfg, imgs)
    assert _rel(want, want64) <= 2e-6, (L, key, _rel(want, want64))   # the float32 oracle is a sound reference for 2e-5
    _check_precisions("spiked L=%d key=%d" % (L, key), cfg, sd, hw, imgs, want)


# 257 / 258: the first lengths of the streaming kernel, whose fifth 64-key block holds one and two keys
@pytest.mark.parametrize("L", SHORT + [257, 258])
def test_spiked_last_key_vs_oracle(L):
    _spiked_key_case(L, L - 1)


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("which", ["first_of_last_tile", "cls"])
def test_spiked_side_keys_vs_oracle(L, which):
    """the first key of the last key tile (where EXACT starts masking) and key 0, at one L per instantiation"""
    _spiked_key_case(L, 16 * ((L + 15) // 16 - 1) if which == "first_of_last_tile" else 0)


# ---- 3. the sweep runs what the table says -----------------------------------------------------------------------------------
FORMS_WORKER = """
import sys, os
sys.path[:0] = [{root!r}, os.path.join({root!r}, "mp-reid_amd"), os.path.join({root!r}, "tests")]
import torch
from mpreid import ops, synth
from test_gpu_tokens import SMALL, _grid
for L in {lengths!r}:
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05)
    imgs = torch.from_numpy(synth.synthetic_images(2, 16 * h, 16 * w, seed=L))
    for prec in ("fp16", "split"):
        sys.stderr.write("FORMS-CASE %d %s\\n" % (L, prec))
        sys.stderr.flush()
        ops.VitEncoder(cfg, sd, (16 * h, 16 * w), precision=prec)(imgs)
        torch.cuda.synchronize()
print("FORMS OK")
"""
# the first L of this list that reaches an instantiation makes the library name it (once per process and device)
EXPECTED_FORMS = {
    (17, "fp16"): "attention<2,2,EXACT>", (17, "split"): "attention_split<2,2>",
    (99, "fp16"): "attention<10,4,MASKALL>", (99, "split"): "attention_split<10,8>",
    (129, "fp16"): "attention<10,4,EXACT>", (129, "split"): "attention_split<8,4,XKEY>",
    (177, "fp16"): "attention<14,8,MASKALL>", (177, "split"): "attention_split<14,8>",
    (211, "fp16"): "attention<14,8,EXACT>", (211, "split"): None,   # <14,8> again: named at 177
    (241, "fp16"): "attention<16,8,EXACT>", (241, "split"): "attention_split<16,8>",
    (257, "fp16"): "attention_long<fp16>", (257, "split"): "attention_long<split>",
}


def test_every_instantiation_is_reached(tmp_path):
    """MPREID_TUNE=verbose=1 (latched per process: a child) makes every attention launcher name its instantiation on stderr the
    first time it runs.  One L per instantiation: each reaches the one the table says, and together they are the six fp16
    resident forms, the five split resident forms and both streaming forms -- every one the library holds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "forms_worker.py"
    script.write_text(FORMS_WORKER.format(root=root, lengths=sorted({L for L, _ in EXPECTED_FORMS})))
    env = dict(os.environ, MPREID_TUNE="verbose=1")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORMS OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    seen, case = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("FORMS-CASE"):
            case = (int(line.split()[1]), line.split()[2])
            seen[case] = []
        elif line.startswith("[mpreid] attention") and case is not None:
            seen[case].append(line.split()[1])
    print("FORMS instantiations", seen)
    for case, name in EXPECTED_FORMS.items():
        assert seen.get(case) == ([name] if name else []), (case, seen.get(case), name)
    names = {n for v in seen.values() for n in v}
    assert len([n for n in names if n.startswith("attention<")]) == 6
    assert len([n for n in names if n.startswith("attention_split<")]) == 5
    assert len([n for n in names if n.startswith("attention_long<")]) == 2


# ---- 4. the persistent loop at every instantiation -----------------------------------------------------------------------
@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("prec", ["fp16", "split"])
def test_persistent_loop_wraps_with_the_same_bits(L, prec):
    """Rows do not depend on the batch (include/mpreid.h): a batch of 8 distinct images repeated until B * heads exceeds the
    largest persistent grid, so that every workgroup walks more than one (image, head) pair with the next pair's K / V
    prefetched into registers, gives the rows of the batch of 8 bit for bit, twice in a row.  The grid is at most CU count x
    workgroups per CU: the split launcher takes at most 4 per CU; the fp16 launcher asks the occupancy API, which 50 KB of LDS
    (<10,4>) holds to 3 and 74 KB (<14,8>, <16,8>) to 2, but the 12.5 KB of <2,2> only to 160 / 12.5 = 12 -- taken as 16, the
    number of two-wave workgroups a CU has wave slots for."""
    import ctypes as C
    from mpreid import _lib, ops, synth
    cus = C.c_int(0)
    _lib.require_gpu()
    _lib.check(_lib.load().mpreid_device_info(None, 0, C.byref(cus), None), "mpreid_device_info")
    assert cus.value > 0
    per_cu = 16 if L <= 32 else 4
    h, w = _grid(L)
    cfg = dict(SMALL, h_res=h, w_res=w)
    reps = (cus.value * per_cu // cfg["heads"]) // 8 + 1
    B = 8 * reps
    assert B * cfg["heads"] > cus.value * per_cu
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05, ln_jitter=0.1)
    enc = ops.VitEncoder(cfg, sd, (16 * h, 16 * w), precision=prec, ws_tag="wrap")
    imgs = torch.from_numpy(synth.synthetic_images(8, 16 * h, 16 * w, seed=L)).cuda()
    base = enc(imgs).clone()
    assert torch.isfinite(base).all() and not torch.equal(base[0], base[1])
    big = imgs.repeat(reps, 1, 1, 1)
    for run in range(2):
        got = enc(big).view(reps, 8, -1)
        bad = (got != base[None]).any(-1).nonzero()
        assert bad.numel() == 0, (L, prec, run, B, bad[:8].tolist())
    del big
    ops.release_workspaces("wrap")


# ---- 5. supported configs nobody runs --------------------------------------------------------------------------------------
def _cfg_case(tag, cfg, hw, seed):
    from mpreid import synth
    # weights N(0, 0.05^2 * 128 / width): the gain of every linear layer of the width-128 sweeps (CLIP's own init scales the
    # same way, width ** -0.5)
    sd = synth.vit_state_dict(cfg, seed=7, std=0.05 * (128.0 / cfg["width"]) ** 0.5, ln_jitter=0.1)
    imgs = synth.synthetic_images(3, hw[0], hw[1], seed=seed)
    _check_precisions(tag, cfg, sd, hw, imgs, orc.vit_features(sd, cfg, imgs))


@pytest.mark.parametrize("L", [99, 241])
@pytest.mark.parametrize("width", [256, 512, 1024])
def test_wide_encoders_vs_oracle(width, L):
    """heads 4 / 8 / 16: layernorm_kernel's wider rows, head offsets above 2, N = 256 ... GEMMs"""
    h, w = _grid(L)
    cfg = dict(SMALL, width=width, heads=width // 64, h_res=h, w_res=w)
    _cfg_case("width=%d L=%d" % (width, L), cfg, (16 * h, 16 * w), seed=width + L)


@pytest.mark.parametrize("patch", [32, 8])
def test_patch_sizes_vs_oracle(patch):
    """patch 32 at stride 32 (CLIP ViT-B/32's patch, Kp = 3072) and patch 8 at stride 8 (Kp = 192), L = 99"""
    h, w = _grid(99)
    cfg = dict(SMALL, patch=patch, stride=patch, h_res=h, w_res=w)
    _cfg_case("patch=%d L=99" % patch, cfg, (patch * h, patch * w), seed=patch)


# ---- 6. RN50 attention pool on both sides of its switch ------------------------------------------------------------------
# pool_lds_resident(T, E, heads) = H16 * (E + 8) * 2 + H16 * T * 4 bytes with H16 = heads rounded up to 16 (csrc/rn50.hip); the
# score table stays in LDS while that is <= 160 KB.  Full width: E = 2048, heads = 32: 131584 + 128 T <= 163840  <=>  T <= 252.
# T = (H / 16) * (W / 16) + 1 with H, W multiples of 32, so T - 1 is a product of two even numbers: 249 = 4 * 62 + 1 is the
# largest such T on the resident side (250 / 251 / 252 are not reachable), 253 = 14 * 18 + 1 the smallest on the other.
def _pool_lds(T, E=2048, heads=32):
    h16 = (heads + 15) // 16 * 16
    return h16 * (E + 8) * 2 + h16 * T * 4


@pytest.mark.parametrize("grid", [(4, 62), (14, 18)])
def test_rn50_pool_on_both_sides_of_the_lds_switch(grid):
    from mpreid import ops, synth
    T = grid[0] * grid[1] + 1
    reach = [a * b + 1 for a in range(2, 129, 2) for b in range(2, 129, 2)]
    lim = 160 * 1024
    assert max(t for t in reach if _pool_lds(t) <= lim) == 249 and min(t for t in reach if _pool_lds(t) > lim) == 253
    assert (_pool_lds(T) <= lim) == (T == 249)
    cfg = dict(synth.RN50, h_res=grid[0], w_res=grid[1])
    hw = (16 * grid[0], 16 * grid[1])
    sd = synth.rn50_state_dict(cfg, seed=11)
    imgs = synth.synthetic_images(2, hw[0], hw[1], seed=T)
    want = orc.rn50_features(sd, cfg, imgs)
    for prec, bound in (("fp16", 5e-3), ("split", 2e-5)):   # the bounds of test_rn50_256x256_matches_reference
        got = ops.Rn50Encoder(cfg, sd, hw, precision=prec, ws_tag="pool_edge")(torch.from_numpy(imgs)).cpu().numpy()
        rel = _rel(got, want)
        print("FORMS rn50 T=%d prec=%s rel=%.3e" % (T, prec, rel))
        assert rel <= bound, (T, prec, rel)
    ops.release_workspaces("pool_edge")
