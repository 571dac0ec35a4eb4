"""Drop-in for the reference's ``loss/softmax_loss.py``: ``CrossEntropyLabelSmooth(num_classes, epsilon=0.1, use_gpu=True)`` with
``forward(inputs, targets)`` -- the mean over the rows of minus the sum over the classes of
``((1 - epsilon) [c == y] + epsilon / num_classes) * log_softmax(inputs)``.

On fp32 CUDA logits [rows, num_classes] the loss is an autograd function over the library's kernel (``mpreid.ops.xent_rows``:
mpreid_xent_rows_f32): value and gradient come from one call, stabilised with the row maximum.  Anything else (host tensors,
another dtype, a logit matrix whose width is not num_classes) runs the same formula in torch on the tensors' device.
``cross_entropy(inputs, targets)`` is the epsilon = 0 case, what make_loss uses where the reference calls F.cross_entropy.
"""
import torch
import torch.nn as nn

from mpreid import ops as _ops


class _XentRows(torch.autograd.Function):
    """the label-smoothed cross-entropy of the rows, gradient from the kernel"""

    @staticmethod
    def forward(ctx, logits, targets, epsilon):
        loss, d_logits, _ = _ops.xent_rows(logits.detach(), targets, epsilon)
        ctx.save_for_backward(d_logits)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad):
        (d_logits,) = ctx.saved_tensors
        return grad * d_logits, None, None


def _on_kernel(inputs, targets):
    return (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == 2
            and inputs.shape[0] >= 1 and inputs.shape[1] >= 1 and torch.is_tensor(targets) and targets.dim() == 1
            and not targets.is_floating_point() and targets.dtype != torch.bool and targets.shape[0] == inputs.shape[0])


def smoothed_cross_entropy(inputs, targets, epsilon, num_classes):
    """the formula in torch, on the tensors' device and in their dtype"""
    log_probs = torch.log_softmax(inputs, dim=1)
    hot = torch.zeros_like(log_probs).scatter_(1, targets.to(log_probs.device).unsqueeze(1), 1)
    t = (1 - epsilon) * hot + epsilon / num_classes
    return (-t * log_probs).mean(0).sum()


def cross_entropy(inputs, targets):
    """F.cross_entropy(inputs, targets) with mean reduction: the kernel at epsilon = 0 on fp32 CUDA logits"""
    if _on_kernel(inputs, targets):
        return _XentRows.apply(inputs, targets, 0.0)
    return torch.nn.functional.cross_entropy(inputs, targets.to(inputs.device))


class CrossEntropyLabelSmooth(nn.Module):
    def __init__(self, num_classes, epsilon=0.1, use_gpu=True):
        super().__init__()
        self.num_classes = num_classes
        self.epsilon = epsilon
        self.use_gpu = use_gpu

    def forward(self, inputs, targets):
        if _on_kernel(inputs, targets) and inputs.shape[1] == self.num_classes:
            return _XentRows.apply(inputs, targets, float(self.epsilon))
        return smoothed_cross_entropy(inputs, targets, self.epsilon, self.num_classes)
