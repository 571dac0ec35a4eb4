#!/usr/bin/env python3
"""Stage-2 head step benchmark (random-init parameters): batch 64 as 16 identities x 4, widths 768 / 512, with the 751 identities
of Market-1501 and the 13 164 of VehicleID; as many text features as identities.  Two paths alternate in one process, each step
timed with device events after a warm-up:
  (a) autograd  the same head in torch operations on the same device: F.batch_norm in training mode, the classifiers, the
                label-smoothed cross-entropy and the batch-hard triplet loss written out, backward() to the three features and
                the six head parameters
  (b) fused     mpreid.ops.Stage2Head.step
(a) is measured as two interleaved series a1 / a2 (the order of a round is a1, b, a2): the difference of their medians is the
run-to-run spread a difference between (a) and (b) has to be read against.  Both forms of the step are measured: the Uni-Prompt
stage-2 form and the list form of make_loss; then the parts of the Uni-Prompt step, each alone (medians of 20).  The launch counts: the fused step's from csrc/stage2_head.hip (the kernels of the
library; plus one increment of num_batches_tracked per bottleneck used); for torch the number of ATen operators the step dispatches,
forward and backward, metadata-only ones left out -- each launches at least one kernel, so a lower bound of its launches.  One JSON line, also written to profiles/stage2_head_bench.json.  No rate is a gate.
Usage: python tools/stage2_head_bench.py [--ids 751 13164] [--batch 64] [--rounds 15]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mpreid import ops  # noqa: E402

WIDTH, WIDTH_PROJ, EPSILON, MARGIN = 768, 512, 0.1, 0.3
FUSED_LAUNCHES = {"uniprompt": 16, "list": 31}     # csrc/stage2_head.hip


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(v):
    return sorted(v)[len(v) // 2]


def _xent(s, y):
    lp = torch.log_softmax(s, 1)
    t = torch.zeros_like(lp).scatter_(1, y.unsqueeze(1), 1) * (1 - EPSILON) + EPSILON / s.shape[1]
    return (-t * lp).sum(1).mean()


def _triplet(x, y):
    d = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist").clamp(min=1e-6)
    pos = y[:, None] == y[None, :]
    inf = torch.full_like(d, float("inf"))
    return torch.relu(torch.where(pos, d, -inf).max(1)[0] - torch.where(pos, inf, d).min(1)[0] + MARGIN).mean()


def _torch_loss(t, y, form):
    def branch(f, name, cls):
        bn = F.batch_norm(f, t[name + ".running_mean"], t[name + ".running_var"], t[name + ".weight"], t[name + ".bias"], True, 0.1, 1e-5)
        return bn @ t[cls + ".weight"].T
    idl = _xent(branch(t["f"], "bottleneck", "classifier"), y)
    tri = _triplet(t["f"], y)
    if form == "list":
        idl = idl + _xent(branch(t["f_proj"], "bottleneck_proj", "classifier_proj"), y)
        tri = tri + _triplet(t["f_last"], y) + _triplet(t["f_proj"], y)
    return _xent(t["f_proj"] @ t["text"].T, y) + (idl + tri)


_NO_KERNEL = ("view", "_unsafe_view", "t", "transpose", "unsqueeze", "squeeze", "expand", "detach", "alias", "permute", "select",
              "slice", "as_strided", "reshape", "_reshape_alias", "stride", "size", "sym_size", "is_same_size")


def _count_launches(fn):
    """the ATen operators one call dispatches, forward and backward, without those that only change a tensor's metadata: each
    of them launches at least one kernel, so this is a lower bound of torch's launches (counted on the host, no profiler)"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket.__name__ not in _NO_KERNEL:
                Count.n += 1
            return func(*args, **(kwargs or {}))
    with Count():
        fn()
    torch.cuda.synchronize()
    return Count.n


def measure(ids, batch, rounds, form):
    g = torch.Generator().manual_seed(ids + (form == "list"))
    dev = "cuda"

    def r(*shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).to(dev)
    y = torch.randperm(ids, generator=g)[:batch // 4].repeat_interleave(4)[torch.randperm(batch, generator=g)].to(dev)
    t = {"f_last": r(batch, WIDTH, scale=0.6), "f": r(batch, WIDTH, scale=0.6), "f_proj": r(batch, WIDTH_PROJ, scale=0.6),
         "text": r(ids, WIDTH_PROJ, scale=0.3), "classifier.weight": r(ids, WIDTH, scale=0.05),
         "classifier_proj.weight": r(ids, WIDTH_PROJ, scale=0.05)}
    for name, n in (("bottleneck", WIDTH), ("bottleneck_proj", WIDTH_PROJ)):
        t[name + ".weight"], t[name + ".bias"] = torch.ones(n, device=dev), torch.zeros(n, device=dev)
        t[name + ".running_mean"], t[name + ".running_var"] = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    leaves = [k for k in t if k != "text" and "running" not in k]
    fused_t = {k: v.clone() for k, v in t.items()}
    for k in leaves:
        t[k].requires_grad_(True)

    def step_autograd():
        for k in leaves:
            t[k].grad = None
        loss = _torch_loss(t, y, form)
        loss.backward()
        return loss

    def bn(name):
        return dict(weight=fused_t[name + ".weight"], bias=fused_t[name + ".bias"], running_mean=fused_t[name + ".running_mean"],
                    running_var=fused_t[name + ".running_var"], num_batches_tracked=torch.tensor(0, dtype=torch.long, device=dev))
    head = ops.Stage2Head(fused_t["classifier.weight"], fused_t["classifier_proj.weight"], bn("bottleneck"), bn("bottleneck_proj"),
                          epsilon=EPSILON, margin=MARGIN)

    def step_fused():
        return head.step(fused_t["f_last"], fused_t["f"], fused_t["f_proj"], y, text_features=fused_t["text"], form=form).loss

    for _ in range(3):      # warm-up: workspaces, buffers, code objects
        la, lb = step_autograd(), step_fused()
    torch.cuda.synchronize()
    first = {"autograd": float(la.detach()), "fused": float(lb[0])}
    t_a1, t_a2, t_b = [], [], []
    for _ in range(rounds):
        t_a1.append(_ms(step_autograd))
        t_b.append(_ms(step_fused))
        t_a2.append(_ms(step_autograd))
    a1, a2, b = _median(t_a1), _median(t_a2), _median(t_b)
    part_ms = None
    if form == "uniprompt":     # the parts of the fused step, each alone on the step's own buffers
        bf, ft = head._buffers(batch, ids, form), fused_t
        W, T = ft["classifier.weight"], ft["text"]
        parts = {
            "bn_forward": lambda: ops.bn1d_train(ft["f"], ft["bottleneck.weight"], ft["bottleneck.bias"], y=bf["y"], mean=bf["mean"],
                                                 invstd=bf["invstd"]),
            "scores": lambda: ops.linear_forward(bf["y"], W, out=bf["S"]),
            "xent": lambda: ops.xent_rows(bf["S"], y, EPSILON, validate=False, loss=bf["terms"][0:1], row_loss=bf["row_loss"],
                                          d_logits=bf["dS"]),
            "d_scores_W": lambda: ops.linear_grad_input(bf["dS"], W, out=bf["dy"]),
            "d_scores_T_y": lambda: ops.linear_grad_weight(bf["dS"], bf["y"], out=bf["grads"]["classifier.weight"]),
            "bn_backward": lambda: ops.bn1d_train_backward(ft["f"], bf["dy"], ft["bottleneck.weight"], bf["mean"], bf["invstd"],
                                                           dx_add=bf["d_tri"], dx=bf["d_f"], dweight=bf["grads"]["bottleneck.weight"],
                                                           dbias=bf["grads"]["bottleneck.bias"]),
            "triplet": lambda: ops.triplet_hard(ft["f"], y, MARGIN, d_feat=bf["d_tri"]),
            "i2t_logits": lambda: ops.linear_forward(ft["f_proj"], T, out=bf["i2t"]),
            "i2t_xent": lambda: ops.xent_rows(bf["i2t"], y, EPSILON, need_argmax=True, validate=False, loss=bf["terms"][2:3],
                                              row_loss=bf["row_loss"], d_logits=bf["d_i2t"], argmax=bf["argmax"]),
            "d_i2t_text": lambda: ops.linear_grad_input(bf["d_i2t"], T, out=bf["d_f_proj"]),
        }
        part_ms = {}
        for name, fn in parts.items():
            fn()
            torch.cuda.synchronize()
            part_ms[name] = round(_median([_ms(fn) for _ in range(20)]), 4)
    return {"ids": ids, "form": form, "fused_parts_ms": part_ms, "autograd_ms_a1": round(a1, 4), "autograd_ms_a2": round(a2, 4),
            "autograd_spread_ms": round(abs(a1 - a2), 4), "fused_ms": round(b, 4),
            "fused_minus_autograd_ms": round(b - 0.5 * (a1 + a2), 4),
            "autograd_min_max_ms": [round(min(t_a1 + t_a2), 4), round(max(t_a1 + t_a2), 4)],
            "fused_min_max_ms": [round(min(t_b), 4), round(max(t_b), 4)],
            "fused_launches": FUSED_LAUNCHES[form], "autograd_aten_ops": _count_launches(step_autograd),
            "loss_after_warmup": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, nargs="+", default=[751, 13164])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_head_bench.json"))
    a = ap.parse_args()
    res = {"tool": "stage2_head_bench", "device": torch.cuda.get_device_name(0), "batch": a.batch, "widths": [WIDTH, WIDTH_PROJ],
           "rounds": a.rounds, "runs": [measure(i, a.batch, a.rounds, f) for i in a.ids for f in ("uniprompt", "list")]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
