#!/usr/bin/env python3
"""Output bits of the transformer towers, for comparing two checkouts: one sha256 per output, one line each.

Builds, from mpreid.synth state dicts with fixed seeds, the reduced towers of tests/test_gpu_tower_launches.py (fp16, split
with and without the CLS-only tail, all-fp32, MoE with E = 2 / K = 1 / one MoE block, text with 17 tokens), the smallest RN50
of tests/test_gpu_rn50.py in its three precisions, plus ViT-B/16 split at B = 16 and CLIP's text tower at B = 8, and runs
one forward each.  The image towers also take the same images as uint8 and every test-time-augmentation view from fp32 and
from uint8 input: every instance of the patch gather, the stems and the head is in the listing.  The library and the Python packer are those of the checkout this file sits in: run it
once in each tree and diff the two listings.
Then the gradients, one line per returned tensor: TextEncoder.backward on the two text towers; VitEncoder.backward on the small
dense tower asking for everything, for the bias and LayerNorm names only (column sums without a weight-gradient GEMM) and for
"tokens" alone (no parameter gradient at all: the path the text sweep shares); on a dense tower of 73 tokens (more than one
64-row block of the attention gradient); on MoE towers with (E, K, MoE blocks) = (2, 1, 1) and (4, 2, 2), aux_coef 0.01 and
the gate's gradient; and on ViT-B/16 split at B = 16 with every parameter.  Usage: python tools/tower_bits.py"""
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


def text_grads(name, cfg, batch):
    enc = ops.TextEncoder(cfg, synth.text_state_dict(cfg, seed=21), ws_tag="bits_" + name)
    gen = torch.Generator().manual_seed(2)
    prompts = (torch.randn((batch, cfg["tokens"], cfg["width"]), generator=gen) * 0.02).cuda()
    grad_out = torch.randn((batch, cfg["out_dim"]), generator=gen).cuda()
    show(name + " d prompts", enc.backward(prompts, [(5 * i + 3) % cfg["tokens"] for i in range(batch)], grad_out))
    del enc
    ops.release_workspaces()


def image_grads(name, cfg, sd, hw, batch, wants=(("", None),), aux_coef=0.0):
    """VitEncoder.backward with all three seeds and a cv_emb; wants: (label, names or None = every parameter + cv_emb + tokens)"""
    enc = ops.VitEncoder(cfg, sd, hw, ws_tag="bits_" + name)
    enc.enable_training()
    gen = torch.Generator().manual_seed(4)
    w, od = cfg["width"], cfg["out_dim"]
    x = torch.from_numpy(synth.synthetic_images(batch, hw[0], hw[1], seed=3)).cuda()
    cv = (torch.randn((batch, w), generator=gen) * 0.02).cuda()
    seeds = [torch.randn((batch, d), generator=gen).cuda() for d in (w, w, od)]
    every = [key for key, _, _ in enc._param_fields()]
    for label, names in wants:
        want = every + ["cv_emb", "tokens"] if names is None else [k for k in every + ["cv_emb", "tokens"] if names(k)]
        got = enc.backward(x, cv, *seeds, want=want, aux_coef=aux_coef)
        assert list(got) == want
        for key in want:
            show(name + label + " d " + key.replace("transformer.resblocks.", ""), got[key])
    del enc
    ops.release_workspaces()


def gradients():
    text_grads("small text", TEXT, 3)
    text_grads("clip_text", synth.CLIP_TEXT, 8)
    sd = synth.vit_state_dict(SMALL, seed=7, std=0.05, ln_jitter=0.1)
    image_grads("small", SMALL, sd, (64, 32), 3, wants=(
        (" all", None), (" bias+ln", lambda k: k.endswith("bias") or "ln_" in k), (" tokens", lambda k: k == "tokens")))
    long = dict(h_res=9, w_res=8, patch=16, stride=16, width=128, layers=2, heads=2, out_dim=64)
    image_grads("73 tokens", long, synth.vit_state_dict(long, seed=7, std=0.05, ln_jitter=0.1), (144, 128), 2)
    for E, K, n_moe in ((2, 1, 1), (4, 2, 2)):
        moe = dict(SMALL, num_experts=E, top_k=K, moe_layers=n_moe)
        image_grads("moe %d/%d/%d" % (E, K, n_moe), moe, synth.vit_moe_state_dict(moe, seed=7), (64, 32), 3, aux_coef=0.01)
    image_grads("vit_b16", synth.VIT_B16, synth.vit_state_dict(synth.VIT_B16, seed=7), (256, 128), 16)


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
    gradients()


if __name__ == "__main__":
    main()
