"""The one chunk loop of the encoders (mpreid/ops.py: _forward_images): a batch one image past a tower's chunk size must
equal the two calls on the two sides of the boundary, bit for bit -- a loop that slices the images, cv_emb or out
inconsistently fails here and at no smaller batch."""
import numpy as np
import pytest
import torch

from test_gpu_rn50 import SMALL as RN50_SMALL
from test_gpu_vit import SMALL as VIT_SMALL

pytestmark = pytest.mark.gpu

MEAN, STD = (0.5, 0.4, 0.45), (0.5, 0.25, 0.3)


@pytest.mark.parametrize("tower,precision,step,view", [("vit", "fp32", 64, 1), ("rn50", "fp32", 64, 1), ("rn50", "split", 256, 0)])
def test_batch_across_the_chunk_boundary_equals_its_two_sides(tower, precision, step, view):
    """uint8 input (ToTensor + Normalize in the first kernel), the view of the case, the ViT with a cv_emb row per image;
    64 x 32 images, the reduced configurations of test_gpu_vit.py / test_gpu_rn50.py"""
    from mpreid import ops, synth
    B = step + 1
    rng = np.random.default_rng(step + view)
    u8 = torch.from_numpy(rng.integers(0, 256, (B, 64, 32, 3), dtype=np.uint8))
    if tower == "vit":
        enc = ops.VitEncoder(VIT_SMALL, synth.vit_state_dict(VIT_SMALL, seed=7, std=0.05, ln_jitter=0.1), (64, 32), precision=precision)
        cv = torch.from_numpy(0.1 * rng.standard_normal((B, VIT_SMALL["width"])).astype(np.float32))
    else:
        enc = ops.Rn50Encoder(RN50_SMALL, synth.rn50_state_dict(RN50_SMALL, seed=12), (64, 32), precision=precision)
        cv = None

    def run(lo, hi):
        return enc.forward_view(u8[lo:hi].contiguous(), view, None if cv is None else cv[lo:hi].contiguous(), MEAN, STD).clone()

    whole = run(0, B)
    sides = torch.cat([run(0, step), run(step, B)])
    assert whole.shape == (B, enc.feat_dim) and bool(torch.isfinite(whole).all())
    assert torch.equal(whole, sides)
    assert not torch.equal(whole[step], whole[step - 1])       # (the row past the boundary is its own image's)
