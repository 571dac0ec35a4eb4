#!/usr/bin/env python3
"""Output bits of the transformer towers, for comparing two checkouts: one sha256 per output, one line each.

Builds, from mpreid.synth state dicts with fixed seeds, the reduced towers of tests/test_gpu_tower_launches.py (fp16, split
with and without the CLS-only tail, all-fp32, MoE with E = 2 / K = 1 / one MoE block, text with 17 tokens), the smallest RN50
of tests/test_gpu_rn50.py in its three precisions, plus ViT-B/16 split at B = 16 and CLIP's text tower at B = 8, and runs
one forward each.  The image towers also take the same images as uint8 and every test-time-augmentation view from fp32 and
from uint8 input: every instance of the patch gather, the stems and the head is in the listing.  The library and the Python packer are those of the checkout this file sits in: run it
once in each tree and diff the two listings.  Usage: python tools/tower_bits.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mpreid import ops, synth  # noqa: E402

SMALL = dict(h_res=4, w_res=2, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
TEXT = dict(tokens=17, width=128, layers=2, heads=2, out_dim=64)


def show(name, t):
    torch.cuda.synchronize()
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    print("%-28s %-14s %s" % (name, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


VIEWS = ((ops.VIEW_FLIP, "flip"), (ops.VIEW_PSEUDO_IR, "ir"), (ops.VIEW_PSEUDO_RGB, "rgb"))


def image_inputs(name, enc, batch, hw, views):
    """plain, uint8, then every view of `views` from fp32 and from uint8 input: one line each"""
    imgs = synth.synthetic_images(batch, hw[0], hw[1], seed=3)
    u8 = torch.from_numpy(np.clip(np.rint((imgs * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()).cuda()
    x = torch.from_numpy(imgs).cuda()
    show(name, enc(x))
    show(name + " uint8", enc.forward_u8(u8))
    for v, vname in views:
        show(name + " view " + vname, enc.forward_view(x, v))
        show(name + " uint8 view " + vname, enc.forward_view(u8, v))
    ops.release_workspaces()


def image_tower(name, cfg, sd, hw, batch, views=VIEWS, **kw):
    image_inputs(name, ops.VitEncoder(cfg, sd, hw, ws_tag="bits_" + name, **kw), batch, hw, views)


def rn50_tower(name, precision, views):
    """the smallest RN50 of tests/test_gpu_rn50.py; the fp16 tower has no in-kernel view"""
    cfg = dict(layers=(1, 2, 1, 1), width=16, heads=8, out_dim=64, h_res=4, w_res=2)
    enc = ops.Rn50Encoder(cfg, synth.rn50_state_dict(cfg, seed=12), (64, 32), ws_tag="bits_" + name, precision=precision)
    image_inputs(name, enc, 3, (64, 32), views)


def text_tower(name, cfg, batch):
    enc = ops.TextEncoder(cfg, synth.text_state_dict(cfg, seed=21), ws_tag="bits_" + name)
    prompts = (torch.randn((batch, cfg["tokens"], cfg["width"]), generator=torch.Generator().manual_seed(1)) * 0.02).cuda()
    show(name, enc.forward(prompts, [(5 * i + 3) % cfg["tokens"] for i in range(batch)]))
    del enc
    ops.release_workspaces()


def main():
    sd = synth.vit_state_dict(SMALL, seed=7, std=0.05, ln_jitter=0.1)
    image_tower("small fp16", SMALL, sd, (64, 32), 3, precision="fp16")
    image_tower("small split cls", SMALL, sd, (64, 32), 3)
    image_tower("small split all", SMALL, sd, (64, 32), 3, cls_only_last=False)
    image_tower("small fp32", SMALL, sd, (64, 32), 3, views=VIEWS[:2], precision="fp32")
    moe = dict(SMALL, num_experts=2, top_k=1, moe_layers=1)
    image_tower("small moe", moe, synth.vit_moe_state_dict(moe, seed=7), (64, 32), 3)
    text_tower("small text", TEXT, 3)
    rn50_tower("rn50 fp16", "fp16", ())
    rn50_tower("rn50 fp32", "fp32", VIEWS)
    rn50_tower("rn50 split", "split", VIEWS)
    image_tower("vit_b16 split", synth.VIT_B16, synth.vit_state_dict(synth.VIT_B16, seed=7), (256, 128), 16, views=VIEWS[:1])
    text_tower("clip_text", synth.CLIP_TEXT, 8)


if __name__ == "__main__":
    main()
