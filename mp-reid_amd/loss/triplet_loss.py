"""Drop-in for the reference's ``loss/triplet_loss.py``: ``TripletLoss(margin=None, hard_factor=0.0)``, called as
``triplet(global_feat, labels)`` -> ``(loss, dist_ap, dist_an)`` -- batch-hard mining over the Euclidean distance matrix (the
hardest positive of an anchor is the farthest row of its label, itself included; the hardest negative the nearest other row),
then MarginRankingLoss(margin) or, without a margin, SoftMarginLoss of ``dist_an - dist_ap``.

On fp32 CUDA features [B, dim] with B <= 1024 the loss is an autograd function over the library's kernels
(``mpreid.ops.triplet_hard``: mpreid_triplet_hard_f32): value and gradient come from one call.  Anything else (host tensors,
another dtype, a larger batch) runs the same formula in torch on the tensors' device.  Both compute the distance as a sum of
squared differences, the exact-arithmetic value of the reference's |x|^2 + |y|^2 - 2 x.y, which in fp32 loses the digits of
close pairs; and both answer label groups of unequal sizes, where the reference's ``view(N, -1)`` raises.  The gradient flows
through the loss; ``dist_ap`` and ``dist_an`` are returned for logging, detached on the kernel path.
``normalize_feature=True`` raises NotImplementedError: make_loss never passes it.
"""
import torch

from mpreid import _lib
from mpreid import ops as _ops


class _TripletHard(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, labels, margin, hard_factor):
        loss, ap, an, _, _, d_feat = _ops.triplet_hard(feat.detach(), labels, margin, hard_factor)
        ctx.save_for_backward(d_feat)
        ctx.mark_non_differentiable(ap, an)
        return loss[0].clone(), ap, an

    @staticmethod
    def backward(ctx, grad, _ap, _an):
        (d_feat,) = ctx.saved_tensors
        return grad * d_feat, None, None, None


def euclidean_dist(x, y):
    """sqrt(max(sum_e (x_ae - y_be)^2, 1e-12)), [m, d] and [n, d] -> [m, n]"""
    return torch.cdist(x, y, p=2.0, compute_mode="donot_use_mm_for_euclid_dist").clamp(min=1e-6)


def hard_example_mining(dist_mat, labels):
    """(dist_ap, dist_an): per row the largest entry among the same-label columns and the smallest among the others (+inf
    where there is none); any group sizes"""
    labels = labels.to(dist_mat.device)
    pos = labels.unsqueeze(0) == labels.unsqueeze(1)
    inf = torch.full_like(dist_mat, float("inf"))
    return torch.where(pos, dist_mat, -inf).max(1)[0], torch.where(pos, inf, dist_mat).min(1)[0]


class TripletLoss(object):
    def __init__(self, margin=None, hard_factor=0.0):
        self.margin = margin
        self.hard_factor = hard_factor

    def __call__(self, global_feat, labels, normalize_feature=False):
        if normalize_feature:
            raise NotImplementedError("TripletLoss: normalize_feature=True is not built (make_loss never passes it)")
        x = global_feat
        if (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= 1
                and 1 <= x.shape[0] <= _lib.TRIPLET_MAX_BATCH and torch.is_tensor(labels) and labels.dim() == 1
                and not labels.is_floating_point() and labels.shape[0] == x.shape[0]):
            return _TripletHard.apply(x, labels, None if self.margin is None else float(self.margin), float(self.hard_factor))
        dist_ap, dist_an = hard_example_mining(euclidean_dist(x, x), labels)
        dist_ap = dist_ap * (1.0 + self.hard_factor)
        dist_an = dist_an * (1.0 - self.hard_factor)
        if self.margin is not None:
            loss = torch.relu(dist_ap - dist_an + self.margin).mean()
        else:
            loss = torch.nn.functional.softplus(dist_ap - dist_an).mean()
        return loss, dist_ap, dist_an
