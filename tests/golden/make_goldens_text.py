#!/usr/bin/env python3
"""Golden vectors of the CLIP text tower, from the REFERENCE's own CLIP.encode_text.

Run in the build container only (needs the reference, which make_goldens.py imports in place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_text.py

Writes tests/golden/text.npz: prompts, end-of-text rows and the reference's outputs only.  The weights come from
synth.text_state_dict(cfg, seed) and are regenerated from the seed by the tests (tests/text_cases.py: GOLDEN_CASES).
  reduced_*   width 128, 2 heads, 2 layers, 21 tokens, out 64; 5 prompts, read out at rows 1, 5, 19, 20, 20
  full_*      CLIP's text tower (512 / 8 / 12 / 77 / 512); 4 prompts, read out at rows 1, 19, 40, 76

encode_text embeds token ids and reads the row of the largest id.  To feed arbitrary prompt embeddings and read-out rows, the
token-embedding table holds the B * L prompt rows, every position has an id of its own, and the id at the chosen row is the
largest of its prompt (it is swapped with the id of the last position).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402  (imports the reference in place; not edited)
from make_goldens import save, synth  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "mp-reid_amd"))
import text_cases as tc  # noqa: E402


def run_text(cfg, sd_np, prompts, eot):
    B, L, W = prompts.shape
    m = mg.ref_clip.CLIP(embed_dim=cfg["out_dim"], image_resolution=16, vision_layers=1, vision_width=64, vision_patch_size=16,
                         vision_stride_size=16, context_length=L, vocab_size=B * L, transformer_width=W,
                         transformer_heads=cfg["heads"], transformer_layers=cfg["layers"], h_resolution=1, w_resolution=1)
    ids = np.arange(B * L, dtype=np.int64).reshape(B, L)
    for b, e in enumerate(eot):
        ids[b, e], ids[b, L - 1] = ids[b, L - 1], ids[b, e]
    table = np.empty((B * L, W), np.float32)
    table[ids.reshape(-1)] = prompts.reshape(B * L, W)
    own = m.state_dict()
    with torch.no_grad():
        for k, v in sd_np.items():
            own[k].copy_(torch.from_numpy(v))
        own["token_embedding.weight"].copy_(torch.from_numpy(table))
    m.eval()
    text = torch.from_numpy(ids)
    assert text.argmax(dim=-1).tolist() == list(eot)
    with torch.no_grad():
        out = m.encode_text(text).numpy()
        # rows behind the read-out row do not reach the result: the reference's mask is causal
        table2 = table.copy()
        for b, e in enumerate(eot):
            table2[ids[b, e + 1:]] += 1.0
        own["token_embedding.weight"].copy_(torch.from_numpy(table2))
        assert np.array_equal(m.encode_text(text).numpy(), out)
    assert out.shape == (B, cfg["out_dim"]) and np.isfinite(out).all()
    return out.astype(np.float32)


def gen_text():
    out = {}
    for name, (cfg, seed, eot) in tc.GOLDEN_CASES.items():
        sd = synth.text_state_dict(cfg, seed=seed)
        prompts = tc.make_prompts(cfg, len(eot), seed + 1000)
        out[name + "_prompts"] = prompts
        out[name + "_eot"] = np.asarray(eot, np.int32)
        out[name + "_out"] = run_text(cfg, sd, prompts, eot)
        print(name, "rel L2 of the float64 restatement:", tc.rel_l2(tc.tower_f64(cfg, sd, prompts, eot), out[name + "_out"]))
    save("text.npz", **out)


if __name__ == "__main__":
    assert mg.ref_clip is not None
    gen_text()
