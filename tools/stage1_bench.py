#!/usr/bin/env python3
"""Stage-1 prompt-learning step benchmark (random-init weights): CLIP's text tower, the 751 identities of Market-1501, batches of
64, stage 1a.  Two paths alternate in one process, each step timed with device events after a warm-up:
  (a) autograd  the path without the fused trainer: prompt assembly and get_text's TextEncoder.forward_grad under autograd, the
                loss in torch operations, backward(), torch.optim.Adam (weight decay 5e-4)
  (b) fused     mpreid.ops.PromptTrainer.step
(a) is measured as two interleaved series a1 / a2 (the order of a round is a1, b, a2): the difference of their medians is the
run-to-run spread a difference between (a) and (b) has to be read against.  Then the parts of the fused step, each alone: text
forward, the loss pair, text backward, the segment sum, the Adam step (medians).  One JSON line, also written to
profiles/stage1_bench.json.  No rate is a gate.
Usage: python tools/stage1_bench.py [--ids 751] [--batch 64] [--rounds 15] [--reps 30]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
from model import make_model_uniprompt as mu  # noqa: E402
from mpreid import ops, synth  # noqa: E402


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(v):
    return sorted(v)[len(v) // 2]


def _learner(ids, seed, stage):
    g = torch.Generator().manual_seed(seed)
    pl = mu.PromptLearner()
    pl.set_tensors({k: torch.randn(*s, generator=g) * 0.02 for k, s in mu.prompt_shapes(ids).items()}, "cuda")
    pl.set_training_stage(stage)
    return pl


def _contrastive(a, b, y):
    logp = torch.log_softmax(a @ b.T, dim=1)
    pos = (y[:, None] == y[None, :]).to(logp.dtype)
    return -((pos * logp).sum(1) / pos.sum(1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=751)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_bench.json"))
    a = ap.parse_args()
    cfg = synth.CLIP_TEXT
    B, eot, lr, wd = a.batch, 19, 3e-4, 5e-4
    enc = ops.TextEncoder(cfg, synth.text_state_dict(cfg, seed=21), ws_tag="stage1_bench")
    g = torch.Generator().manual_seed(2)
    img = (torch.randn((B, cfg["out_dim"]), generator=g) * 0.1).cuda()
    labels = torch.randint(0, a.ids, (B,), generator=g).cuda()
    labels[1] = labels[0]     # at least one repeated identity

    # (a) the autograd path
    pl_a = _learner(a.ids, 3, "1a")
    pl_a.ctx_generic.requires_grad_(True)
    opt = torch.optim.Adam([pl_a.ctx_generic], lr=lr, weight_decay=wd)
    rows = [eot] * B

    def step_autograd():
        opt.zero_grad()
        feats = enc.forward_grad(pl_a.forward(labels), rows)
        loss = _contrastive(img, feats, labels) + _contrastive(feats, img, labels)
        loss.backward()
        opt.step()
        return loss

    # (b) the fused path
    pl_b = _learner(a.ids, 3, "1a")
    trainer = ops.PromptTrainer(enc, pl_b, "1a", eot=eot, lr=lr, weight_decay=wd)

    def step_fused():
        return trainer.step(img, labels)

    for _ in range(3):      # warm-up: workspaces, transposed weights, optimizer state, code objects
        la, lb = step_autograd(), step_fused()
    torch.cuda.synchronize()
    first = {"autograd": float(la.detach()), "fused": float(lb.sum())}
    t_a1, t_a2, t_b = [], [], []
    for _ in range(a.rounds):
        t_a1.append(_ms(step_autograd))
        t_b.append(_ms(step_fused))
        t_a2.append(_ms(step_autograd))
    a1, a2, b = _median(t_a1), _median(t_a2), _median(t_b)

    # the parts of the fused step, each alone
    prompts = pl_b.forward(labels).detach().contiguous()
    bufs = trainer._buffers(B)
    grad = trainer.grads["ctx_generic"]
    p = pl_b.ctx_generic.detach()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    parts = {
        "prompt_assembly": lambda: pl_b.forward(labels, validate=False),
        "text_forward": lambda: enc._forward_into(prompts, bufs["eot"], bufs["feats"]),
        "supcon_pair": lambda: ops.supcon_pair(img, bufs["feats"], labels, loss=bufs["loss"], d_txt=bufs["d_txt"]),
        "text_backward": lambda: enc._backward_into(prompts, bufs["eot"], bufs["d_txt"], bufs["d_prompts"]),
        "rows_segment_sum": lambda: ops.rows_segment_sum(bufs["d_prompts"], labels, 1, 8, a.ids, out=grad, validate=False),
        "adam_step": lambda: ops.adam_step(p, grad, m, v, 1, lr, weight_decay=wd),
    }
    part_ms = {}
    for name, fn in parts.items():
        fn()
        torch.cuda.synchronize()
        part_ms[name] = round(_median([_ms(fn) for _ in range(a.reps)]), 4)
    res = {"tool": "stage1_bench", "device": torch.cuda.get_device_name(0), "ids": a.ids, "batch": B, "rounds": a.rounds,
           "autograd_ms_a1": round(a1, 3), "autograd_ms_a2": round(a2, 3), "autograd_spread_ms": round(abs(a1 - a2), 3),
           "fused_ms": round(b, 3), "fused_minus_autograd_ms": round(b - 0.5 * (a1 + a2), 3),
           "autograd_min_max_ms": [round(min(t_a1 + t_a2), 3), round(max(t_a1 + t_a2), 3)],
           "fused_min_max_ms": [round(min(t_b), 3), round(max(t_b), 3)],
           "fused_parts_ms": part_ms, "fused_parts_sum_ms": round(sum(part_ms.values()), 3),
           "loss_after_warmup": first}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
