"""Drop-in for the reference's ``loss/supcontrast.py``: ``SupConLoss(device)`` with
``forward(text_features, image_features, t_label, i_targets)`` -- the supervised contrastive loss at temperature 1.0 on
unnormalised features: the mean over the rows of ``text_features`` of minus the mean log-softmax probability (over the rows
of ``image_features``) of the entries that carry the row's label.  (The argument names are the reference's; the stage-1 loop
passes the image features first for ``loss_i2t`` and the text features first for ``loss_t2i``.)

The square same-label case -- both feature sets [B, dim] on the device, one label vector, B <= 1024 -- is an autograd function
over the library's kernels (``mpreid.ops.supcon_pair`` with one direction: mpreid_supcon_f32): value and both gradients come
from HIP, stabilised with the row maxima.  Anything else (two different label vectors, a non-square batch, more than 1024 rows,
host tensors, another dtype than fp32) runs the same formula in torch on the tensors' device.  A stage-1 step that needs both
directions and the update at once is ``mpreid.ops.PromptTrainer.step``, which calls the pair form directly.
"""
import torch
import torch.nn as nn

from mpreid import _lib
from mpreid import ops as _ops


class _SupConRows(torch.autograd.Function):
    """loss of the rows of a against the rows of b (the row-softmax direction of S = a b^T), gradients from the kernel"""

    @staticmethod
    def forward(ctx, a, b, labels):
        loss, d_b, d_a = _ops.supcon_pair(a.detach(), b.detach(), labels, need_d_img=True, directions=1)
        ctx.save_for_backward(d_a, d_b)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad):
        d_a, d_b = ctx.saved_tensors
        return grad * d_a, grad * d_b, None


def _same_labels(t_label, i_targets):
    return t_label is i_targets or (t_label.shape == i_targets.shape and t_label.device == i_targets.device
                                    and bool(torch.equal(t_label, i_targets)))


class SupConLoss(nn.Module):
    def __init__(self, device):
        super().__init__()
        self.device = device
        self.temperature = 1.0

    def forward(self, text_features, image_features, t_label, i_targets):
        a, b = text_features, image_features
        if (a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float32 and a.dim() == 2 and a.shape == b.shape
                and 1 <= a.shape[0] <= _lib.SUPCON_MAX_BATCH and torch.is_tensor(t_label) and torch.is_tensor(i_targets)
                and t_label.dim() == 1 and not t_label.is_floating_point() and _same_labels(t_label, i_targets)):
            return _SupConRows.apply(a, b, t_label)
        mask = (t_label.unsqueeze(1) == i_targets.unsqueeze(0)).to(device=a.device, dtype=a.dtype)
        log_prob = torch.log_softmax((a @ b.T) / self.temperature, dim=1)
        return -((mask * log_prob).sum(1) / mask.sum(1)).mean()
