"""Drop-in for the reference's ``loss/make_loss.py``: ``make_loss(cfg, num_classes)`` -> ``(loss_func, center_criterion)``.

DATALOADER.SAMPLER 'softmax': ``loss_func(score, feat, target)`` is the plain cross-entropy of the score.
DATALOADER.SAMPLER 'softmax_triplet' with MODEL.METRIC_LOSS_TYPE 'triplet': ``loss_func(score, feat, target, target_cam,
i2tscore=None)`` is  ID_LOSS_WEIGHT * identity loss + TRIPLET_LOSS_WEIGHT * triplet loss [+ I2T_LOSS_WEIGHT * image-to-text
loss] , where score and feat are tensors or lists of tensors (the losses of a list are added), the identity and the
image-to-text loss are label-smoothed with MODEL.IF_LABELSMOOTH 'on' and plain cross-entropy otherwise, and the triplet loss
has the margin SOLVER.MARGIN or, with MODEL.NO_MARGIN, the soft-margin form.  On fp32 CUDA tensors every term is an autograd
function over the library's kernels (loss/softmax_loss.py, loss/triplet_loss.py); a whole head step without autograd is
``mpreid.ops.Stage2Head``.  A configuration the reference only prints a complaint about (and then fails on) raises ValueError.

``center_criterion`` is a plain torch CenterLoss with the reference's constructor: loss_func never calls it, and it is not
accelerated.
"""
import torch
import torch.nn as nn

from .softmax_loss import CrossEntropyLabelSmooth, cross_entropy
from .triplet_loss import TripletLoss


class CenterLoss(nn.Module):
    """mean over the batch of the squared distance of a feature to the centre of its class, clamped to [1e-12, 1e12]"""

    def __init__(self, num_classes=751, feat_dim=2048, use_gpu=True):
        super().__init__()
        self.num_classes, self.feat_dim, self.use_gpu = num_classes, feat_dim, use_gpu
        device = "cuda" if use_gpu and torch.cuda.is_available() else "cpu"
        self.centers = nn.Parameter(torch.randn(num_classes, feat_dim, device=device))

    def forward(self, x, labels):
        assert x.size(0) == labels.size(0), "features.size(0) is not equal to labels.size(0)"
        d = (x - self.centers[labels.to(self.centers.device)].to(x.device)).pow(2).sum(1)
        return d.clamp(min=1e-12, max=1e+12).mean()


def _sum_over(fn, x):
    return sum(fn(t) for t in x) if isinstance(x, list) else fn(x)


def make_loss(cfg, num_classes):
    sampler = cfg.DATALOADER.SAMPLER
    center_criterion = CenterLoss(num_classes=num_classes, feat_dim=2048, use_gpu=True)
    if sampler == 'softmax':
        def loss_func(score, feat, target):
            return cross_entropy(score, target)
        return loss_func, center_criterion
    if sampler != 'softmax_triplet':
        raise ValueError("expected sampler should be softmax or softmax_triplet but got {}".format(sampler))
    if cfg.MODEL.METRIC_LOSS_TYPE != 'triplet':
        raise ValueError("expected METRIC_LOSS_TYPE should be triplet but got {}".format(cfg.MODEL.METRIC_LOSS_TYPE))
    triplet = TripletLoss() if cfg.MODEL.NO_MARGIN else TripletLoss(cfg.SOLVER.MARGIN)
    xent = CrossEntropyLabelSmooth(num_classes=num_classes) if cfg.MODEL.IF_LABELSMOOTH == 'on' else cross_entropy
    w_id, w_tri, w_i2t = cfg.MODEL.ID_LOSS_WEIGHT, cfg.MODEL.TRIPLET_LOSS_WEIGHT, cfg.MODEL.I2T_LOSS_WEIGHT

    def loss_func(score, feat, target, target_cam, i2tscore=None):
        id_loss = _sum_over(lambda s: xent(s, target), score)
        tri_loss = _sum_over(lambda f: triplet(f, target)[0], feat)
        loss = w_id * id_loss + w_tri * tri_loss
        if i2tscore is not None:
            loss = w_i2t * xent(i2tscore, target) + loss
        return loss
    return loss_func, center_criterion
