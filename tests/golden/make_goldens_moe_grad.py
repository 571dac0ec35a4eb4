#!/usr/bin/env python3
"""Golden features, router logits, load-balancing loss and gradients of the MoE image tower, from the REFERENCE's own
VisionTransformer (MODEL.MOE.ENABLED form) under float64 autograd.

Run in the build container only (needs the reference, which make_goldens.py imports in place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_moe_grad.py

Writes tests/golden/moe_grad.npz, data only, for the cases moe_grad_cases.GOLDEN_CASES (`reduced`: E 4, K 2, 2 of 3 blocks MoE;
`reduced_all`: E 3, K 1, every block MoE), each with cv_emb given and all three seeds non-zero: x11[:, 0], x12[:, 0] and
xproj[:, 0]; the router logits exactly as returned (fourth return value, flat index l * B + b); the reference's
load_balancing_loss_func of them; and two sets of gradients, each in every parameter that autograd reaches and in cv_emb, packed
by vit_grad_cases.golden_pack (small tensors whole, of a larger matrix fixed rows and the Frobenius norm):
    of sum(x11[:, 0] o d1) + sum(x12[:, 0] o d2) + sum(xproj[:, 0] o d3)
    of load_balancing_loss_func(logits, top_k) alone, under the prefix aux_
(apart, because beside seeds of unit size the second is a thousandth of the first and would be checked to three digits less).  `<case>_nograd` lists the parameters whose .grad autograd leaves at None (the gates
of blocks 1 ..).  Of the experts the bias gradients are kept and the matrices' left out: they are frozen in stage 2, nothing in
the project computes them, their biases see the same du and dy, and with them the file would pass the 1 MiB a committed file may
have.  The case's seed is stored: weights, images, cv_emb and seeds are regenerated from it by the tests.

Three float32 casts of the reference would cap a float64 run at 1e-7, and are lifted for this run: its LayerNorm casts its input
("to handle fp16"), so its forward is torch.nn.LayerNorm's own, as in make_goldens_vit_grad.py; and its MoE block asks for the
router's softmax in torch.float (model/clip/model.py:208), so the module's `F` is a view of torch.nn.functional whose softmax
drops that request when the logits are float64; and load_balancing_loss_func takes the expert shares as a float32 mean of the
0/1 mask (:368, `expert_mask.float()`), whose 2^-24 the gradient magnifies by the shares' size over their spread (the gradient
sees only their differences), so Tensor.float answers in float64 while that function runs (`l_aux_f64` and the aux_ set).
`l_aux` is the function's value as the reference returns it, with nothing lifted inside it.  Nothing else is touched.
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

sys.path.insert(0, os.path.join(mg.ROOT, "mp-reid_amd"))
import moe_grad_cases as gc  # noqa: E402
import vit_grad_cases as vg  # noqa: E402


class _FunctionalF64:
    """torch.nn.functional, except that softmax keeps float64 logits in float64"""

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    @staticmethod
    def softmax(x, dim=None, dtype=None):
        return torch.nn.functional.softmax(x, dim=dim, dtype=None if x.dtype == torch.float64 else dtype)


def gen():
    mg.ref_clip.LayerNorm.forward = torch.nn.LayerNorm.forward
    mg.ref_clip.F = _FunctionalF64()
    out = {}
    for name in gc.GOLDEN_CASES:
        c = gc.tower_case(name)
        cfg = c["cfg"]
        m = mg.ref_clip.VisionTransformer(cfg["h_res"], cfg["w_res"], cfg["patch"], cfg["stride"], cfg["width"], cfg["layers"],
                                          cfg["heads"], cfg["out_dim"], num_experts=cfg["num_experts"], top_k=cfg["top_k"],
                                          moe_layers=cfg["moe_layers"], dropout=0.0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
        m.double().train()
        cv_t = torch.from_numpy(c["cv"]).double().requires_grad_(True)
        x11, x12, xproj, logits = m(torch.from_numpy(c["imgs"]).double(), cv_t)
        feats = (x11[:, 0], x12[:, 0], xproj[:, 0])
        l_aux_as_is = float(mg.ref_clip.load_balancing_loss_func(logits.detach(), cfg["top_k"]))
        keep_float = torch.Tensor.float
        torch.Tensor.float = torch.Tensor.double
        try:
            l_aux = mg.ref_clip.load_balancing_loss_func(logits, cfg["top_k"])
        finally:
            torch.Tensor.float = keep_float
        loss = sum((f * torch.from_numpy(d).double()).sum() for f, d in zip(feats, c["seeds"]))
        loss.backward(retain_graph=True)
        p = name + "_"
        out[p + "seed"] = np.int64(c["seed"])
        out[p + "f_last"], out[p + "f"], out[p + "f_proj"] = (f.detach().numpy() for f in feats)
        out[p + "logits"] = logits.detach().numpy()
        out[p + "l_aux"] = np.float64(l_aux_as_is)
        out[p + "l_aux_f64"] = np.float64(float(l_aux))
        grads = {k: q.grad.numpy() for k, q in m.named_parameters() if q.grad is not None}
        nograd = sorted(k for k, q in m.named_parameters() if q.grad is None)
        grads["cv_emb"] = cv_t.grad.numpy()
        assert set(grads) | set(nograd) == set(c["sd"]) | {"cv_emb"}
        out[p + "nograd"] = np.array(nograd)
        for k, g in grads.items():
            assert np.isfinite(g).all(), k
            if ".experts." in k and k.endswith(".weight"):
                continue   # (the file's size: see the module's text)
            out.update({p + kk: v for kk, v in vg.golden_pack(k, g).items()})
        m.zero_grad(set_to_none=True)
        cv_t.grad = None
        l_aux.backward()
        aux = {k: q.grad.numpy() for k, q in m.named_parameters() if q.grad is not None and ".experts." not in k}
        aux["cv_emb"] = cv_t.grad.numpy()
        assert "transformer.resblocks.0.gate.weight" in aux and not any(k.startswith(("ln_post", "proj")) for k in aux)
        out[p + "aux_keys"] = np.array(sorted(aux))
        for k, g in aux.items():
            out.update({p + "aux_" + kk: v for kk, v in vg.golden_pack(k, g).items()})
        print(name, "seed", c["seed"], "l_aux", float(l_aux), "no .grad:", nograd)
        dev = gc.golden_deviations(name, out)
        worst = max(dev, key=dev.get)
        print("  largest deviation of the restatement: %.2e (%s); l_aux %.2e" % (dev[worst], worst, dev["l_aux"]))
    save("moe_grad.npz", **out)


if __name__ == "__main__":
    assert mg.ref_clip is not None
    gen()
