#!/usr/bin/env python3
"""Golden vectors of the long-token geometries (256 x 256 inputs: more than 256 tokens), from the REFERENCE.

Run in the build container only (needs the reference, which make_goldens.py imports in place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_tokens.py

Writes tests/golden/vit_tokens.npz: the reference's OUTPUTS only.  Images come from synth.synthetic_images and weights from
synth.vit_state_dict / synth.rn50_state_dict, regenerated from the seeds below by the tests.
  b16_257_feat     ViT-B/16, 256 x 256, stride 16 (16 x 16 grid, L = 257), 4 images (seed 1257), weights seed 7
  b16_257_cv       the camera / view embedding added to the CLS token (seeded, stored: it is an input)
  b16_257_feat_cv  the same with that embedding
  b16_442_feat     ViT-B/16, 256 x 256, stride 12 (21 x 21 grid, L = 442), 2 images (the first two of seed 1257), weights seed 8
  rn50_257_feat    RN50, 256 x 256 (16 x 16 final grid, T = 257), 3 images (seed 1258), weights seed 11
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (imports the reference in place; not edited)
from make_goldens import run_rn50, run_vit, save, synth  # noqa: E402

VIT_257 = dict(synth.VIT_B16, h_res=16, w_res=16)
VIT_442 = dict(synth.VIT_B16, h_res=21, w_res=21, stride=12)
RN50_257 = dict(synth.RN50, h_res=16, w_res=16)


def gen_vit_tokens():
    out = {}
    imgs = synth.synthetic_images(4, 256, 256, seed=1257)
    sd = synth.vit_state_dict(VIT_257, seed=7, std=0.02, ln_jitter=0.05)
    out["b16_257_feat"], _ = run_vit(VIT_257, sd, imgs)
    cv = (np.random.default_rng(18).standard_normal((4, 768)) * 0.02 * 3.0).astype(np.float32)
    out["b16_257_cv"] = cv
    out["b16_257_feat_cv"], _ = run_vit(VIT_257, sd, imgs, cv)
    sd12 = synth.vit_state_dict(VIT_442, seed=8, std=0.02, ln_jitter=0.05)
    out["b16_442_feat"], _ = run_vit(VIT_442, sd12, imgs[:2])
    imgs = synth.synthetic_images(3, 256, 256, seed=1258)
    out["rn50_257_feat"], _, _ = run_rn50(RN50_257, synth.rn50_state_dict(RN50_257, seed=11), imgs)
    save("vit_tokens.npz", **out)


if __name__ == "__main__":
    assert mg.ref_clip is not None
    gen_vit_tokens()
