#!/usr/bin/env python3
"""Golden gradients of the image tower, from the REFERENCE's own VisionTransformer under float64 autograd.

Run in the build container only (needs the reference, which make_goldens.py imports in place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_vit_grad.py

Writes tests/golden/vit_grad.npz for the case vit_grad_cases.GOLDEN_CASE (width 128, 2 heads, 2 layers, a 48 x 32 image, batch 2,
cv_emb given, all three seeds non-zero): the three features at the CLS row and the gradient of
sum(x11[:, 0] o d_f_last) + sum(x12[:, 0] o d_f) + sum(xproj[:, 0] o d_f_proj) in every parameter and in cv_emb.  Tensors of at
most SMALL elements go in whole; of a larger matrix the rows vit_grad_cases.golden_rows picks and its Frobenius norm.  The
weights, images, cv_emb and seeds are regenerated from their seeds by the tests.

The reference's LayerNorm casts its input to float32 ("to handle fp16"), which would cap a float64 run at 1e-7; for this run
its forward is torch.nn.LayerNorm's own, so that the whole graph is float64.  Nothing else of the reference is touched.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402  (imports the reference in place; not edited)
from make_goldens import save  # noqa: E402

import vit_grad_cases as vg  # noqa: E402


def gen():
    name = vg.GOLDEN_CASE
    cfg, img_hw, sd, imgs, cv, _ = vg.tower_case(name)
    mg.ref_clip.LayerNorm.forward = torch.nn.LayerNorm.forward
    m = mg.ref_clip.VisionTransformer(cfg["h_res"], cfg["w_res"], cfg["patch"], cfg["stride"], cfg["width"], cfg["layers"],
                                      cfg["heads"], cfg["out_dim"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.double().train()
    cv_t = torch.from_numpy(cv).double().requires_grad_(True)
    x11, x12, xproj = m(torch.from_numpy(imgs).double(), cv_t)
    feats = (x11[:, 0], x12[:, 0], xproj[:, 0])
    loss = sum((f * torch.from_numpy(d).double()).sum() for f, d in zip(feats, vg.make_seeds(name)))
    loss.backward()
    out = {"f_last": feats[0].detach().numpy(), "f": feats[1].detach().numpy(), "f_proj": feats[2].detach().numpy()}
    grads = {k: p.grad.numpy() for k, p in m.named_parameters()}
    grads["cv_emb"] = cv_t.grad.numpy()
    assert set(grads) == set(sd) | {"cv_emb"}
    for k, g in grads.items():
        assert np.isfinite(g).all() and g.any(), k
        out.update(vg.golden_pack(k, g))
    save("vit_grad.npz", **out)
    mine = vg.tower_grads(name)
    print("largest relative deviation of the restatement:",
          max(vg.golden_deviation(k, mine[k].numpy(), out) for k in grads))


if __name__ == "__main__":
    assert mg.ref_clip is not None
    gen()
