#!/usr/bin/env python3
"""Stage-2 training step benchmark (random-init parameters): the Uni-Prompt model at ViT-B/16, 256 x 128 images, batch 64 as 16
identities x 4, 751 identities, SIE off.  One process, every series after a warm-up, medians of `rounds`; compared series
alternate inside a round.  The learning rate is 1e-6 so that a hundred steps on random weights stay finite: the arithmetic and
the traffic of a step do not depend on it.
  step        a whole mpreid.ops.Stage2Trainer.step (host clock around the step and a device synchronise) and its parts, each
              alone: forward_train, Stage2Head.step, VitEncoder.backward, TensorOptimizer.step (device events) and
              sync_weights_batched (host clock: it contains a wait for the device)
  optimizer   TensorOptimizer.step over the trainer's table against a loop of mpreid.ops.adam_step over the same tensors, what the
              library could do before; launches from the library's own count (mpreid_optim_step_launches; one per tensor for
              the loop); achieved bytes per second at 28 bytes per element (4 reads + 3 writes) beside the floor derived from
              a 6.3 TB/s copy
  repack      sync_weights_batched() against sync_weights(), with the number of device synchronisations of each
  paths       the fused step against the autograd path: the model's training-mode forward, make_loss, backward(),
              torch.optim.Adam(foreach=False) -- and the ATen operators that path dispatches (tools/stage2_head_bench.py's count)
One JSON line, also written to profiles/stage2_train_bench.json.  No rate is a gate.
Usage: python tools/stage2_train_bench.py [--rounds 15] [--batch 64] [--ids 751]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
from mpreid import ops  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from stage2_head_bench import _count_launches, _median, _ms  # noqa: E402

COPY_BYTES_PER_S = 6.3e12      # a float4 copy on this chip (the floor's yardstick, not a measurement of this tool)


def _host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ids", type=int, default=751)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_train_bench.json"))
    a = ap.parse_args()
    from config import cfg_base
    from loss.make_loss import make_loss
    from model import make_model_uniprompt as mu
    from solver.make_optimizer_prompt import make_optimizer_2astage
    cfg = cfg_base.clone()
    cfg.defrost()
    cfg.merge_from_list(["DATALOADER.SAMPLER", "softmax_triplet"])
    cfg.SOLVER.STAGE2.update(BASE_LR=1e-6, IMS_PER_BATCH=a.batch)
    m = mu.make_model(cfg, num_class=a.ids, camera_num=6, view_num=1).enable_stage2_training()
    loss_fn, center = make_loss(cfg, a.ids)
    opt, _ = make_optimizer_2astage(cfg, m, center)
    assert isinstance(opt, ops.TensorOptimizer)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(a.batch, 3, 256, 128, generator=g).cuda()
    y = torch.randperm(a.ids, generator=g)[:a.batch // 4].repeat_interleave(4)[torch.randperm(a.batch, generator=g)].cuda()
    with torch.no_grad():
        m.eval()
        text = torch.cat([m(label=torch.arange(lo, min(lo + 64, a.ids)), get_text=True) for lo in range(0, a.ids, 64)]).float().contiguous()
    tr = m.stage2_trainer(cfg, opt, text)
    enc, head = tr.enc, tr.head
    params = dict(m.named_parameters())
    topt = torch.optim.Adam([{"params": [p], "lr": 1e-6, "weight_decay": cfg.SOLVER.STAGE2.WEIGHT_DECAY} for p in params.values()],
                            foreach=False)

    def step_fused():
        return tr.step(img, y).loss

    def step_autograd():
        m.train()
        topt.zero_grad()
        scores, feats, proj = m(x=img, label=y)
        loss = loss_fn(scores[0], feats[1], y, None, proj @ text.t())
        loss.backward()
        topt.step()
        return loss.detach()

    for _ in range(3):
        lf, la = step_fused(), step_autograd()
    torch.cuda.synchronize()
    res = {"tool": "stage2_train_bench", "device": torch.cuda.get_device_name(0), "batch": a.batch, "ids": a.ids, "rounds": a.rounds,
           "loss_after_warmup": {"fused": float(lf), "autograd": float(la)}}

    # ---- the two paths, alternating: a1, b, a2 ----
    t_a1, t_a2, t_b = [], [], []
    for _ in range(a.rounds):
        t_a1.append(_host_ms(step_autograd))
        enc.sync_weights_batched()      # (untimed: the autograd path's optimizer moved the masters after its own re-pack)
        t_b.append(_host_ms(step_fused))
        t_a2.append(_host_ms(step_autograd))
    a1, a2, b = _median(t_a1), _median(t_a2), _median(t_b)
    res["paths"] = {"autograd_ms_a1": round(a1, 3), "autograd_ms_a2": round(a2, 3), "autograd_spread_ms": round(abs(a1 - a2), 3),
                    "fused_ms": round(b, 3), "fused_min_max_ms": [round(min(t_b), 3), round(max(t_b), 3)],
                    "autograd_min_max_ms": [round(min(t_a1 + t_a2), 3), round(max(t_a1 + t_a2), 3)],
                    "autograd_aten_ops": _count_launches(step_autograd)}

    # ---- the parts of the fused step, each alone on the step's own buffers ----
    st = tr.step(img, y)
    want = tr._want
    out = {k: tr.grads[k] for k in want}
    parts = {"forward_train": lambda: enc.forward_train(img),
             "backward": lambda: enc.backward(img, None, None, st.d_f, st.d_f_proj, want, out=out),
             "optimizer": opt.step}
    feats = enc.forward_train(img)
    parts["head"] = lambda: head.step(feats[0], feats[1], feats[2], y, text, form="uniprompt")
    parts = {k: parts[k] for k in ("forward_train", "head", "backward", "optimizer")}
    step_parts = {}
    for name, fn in parts.items():
        fn()
        torch.cuda.synchronize()
        step_parts[name + "_ms"] = round(_median([_ms(fn) for _ in range(a.rounds)]), 4)
    step_parts["repack_ms"] = round(_median([_host_ms(enc.sync_weights_batched) for _ in range(a.rounds)]), 4)
    step_parts["whole_step_ms"] = round(b, 3)
    res["step"] = step_parts

    # ---- the optimizer: one table call against a loop of single-tensor calls over the same tensors ----
    table = opt._table[1][0]
    rows = [(p, gr, s1, s2) for p, gr, s1, s2, _ in table.keep]
    n_elem = sum(p.numel() for p, _, _, _ in rows)
    lr, wd = 1e-6, cfg.SOLVER.STAGE2.WEIGHT_DECAY

    def multi():
        ops.optim_step_multi(table, [(lr, wd)], "Adam", 7)

    def loop():
        for p, gr, s1, s2 in rows:
            ops.adam_step(p, gr, s1, s2, 7, lr, weight_decay=wd)
    table.set_classes([0] * len(table))
    multi(), loop()
    torch.cuda.synchronize()
    t_m, t_l1, t_l2 = [], [], []
    for _ in range(a.rounds):
        t_l1.append(_ms(loop))
        t_m.append(_ms(multi))
        t_l2.append(_ms(loop))
    h_m = _median([_host_ms(multi) for _ in range(a.rounds)])
    h_l = _median([_host_ms(loop) for _ in range(a.rounds)])
    mm, l1, l2 = _median(t_m), _median(t_l1), _median(t_l2)
    bytes_step = 28.0 * n_elem
    res["optimizer"] = {"tensors": len(rows), "elements": n_elem, "bytes_per_step": bytes_step,
                        "multi_ms": round(mm, 4), "multi_min_max_ms": [round(min(t_m), 4), round(max(t_m), 4)],
                        "loop_ms_1": round(l1, 4), "loop_ms_2": round(l2, 4), "loop_spread_ms": round(abs(l1 - l2), 4),
                        "multi_host_ms": round(h_m, 4), "loop_host_ms": round(h_l, 4),
                        "multi_launches": ops.optim_step_launches(len(rows)), "loop_launches": len(rows),
                        "multi_bytes_per_s": round(bytes_step / (mm * 1e-3), 0), "loop_bytes_per_s": round(bytes_step / (0.5 * (l1 + l2) * 1e-3), 0),
                        "floor_ms_at_copy_rate": round(bytes_step / COPY_BYTES_PER_S * 1e3, 4)}

    # ---- the re-pack ----
    t_s1, t_s2, t_bt = [], [], []
    for _ in range(a.rounds):
        t_s1.append(_host_ms(enc.sync_weights))
        t_bt.append(_host_ms(enc.sync_weights_batched))
        t_s2.append(_host_ms(enc.sync_weights))
    n_mats = 1 + 4 * enc.cfg["layers"]
    res["repack"] = {"gemm_weights": n_mats, "sync_weights_ms_1": round(_median(t_s1), 4), "sync_weights_ms_2": round(_median(t_s2), 4),
                     "sync_weights_batched_ms": round(_median(t_bt), 4), "sync_weights_synchronisations": n_mats + 1,
                     "sync_weights_batched_synchronisations": 1}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
