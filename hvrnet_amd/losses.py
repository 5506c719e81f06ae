"""Loss modules built from config dicts (registry.LOSSES / registry.build_loss).

Mirror of mmdet/models/losses/focal_loss.py with losses/utils.py `weight_reduce_loss`: the sigmoid focal loss over the HIP kernels of
csrc/focal.hip (the rule, the reduction order and the one deviation from the reference are stated in include/hvr_hip.h).  There is
no PyTorch form of the loss here: CPU tensors raise, as every other op of the package does.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import native
from .ops import sigmoid_focal_loss
from .registry import LOSSES


class FocalLossReducedFunction(Function):
    """loss_weight / avg * sum_n w[n] sum_c l[n][c] in one pass over the logits (native.focal_loss): the forward writes the gradient too,
    the backward scales it by the incoming scalar.  -> a 0-dim f32 tensor."""

    @staticmethod
    def forward(ctx, pred, target, weight, gamma, alpha, loss_weight, avg):
        x = pred if pred.stride(-1) == 1 else pred.contiguous()
        out1, d_logits = native.focal_loss(x, target.contiguous(), weight, gamma, alpha, loss_weight, avg)
        ctx.save_for_backward(d_logits)
        ctx.C = pred.shape[1]
        return out1[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d_logits, = ctx.saved_tensors
        return (d_logits[:, :ctx.C] * g,) + (None,) * 6


@LOSSES.register_module
class FocalLoss(nn.Module):

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0):
        super(FocalLoss, self).__init__()
        assert use_sigmoid is True, 'Only sigmoid focal loss supported now.'
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = use_sigmoid, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        """focal_loss.py:62-82.  pred [N, C] logits, target int64 [N], weight [N] per row.  'none' -> [N, C]; 'mean' / 'sum' -> 0-dim."""
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError('reduction %r is none of "none", "mean", "sum"' % (reduction,))
        if avg_factor is not None and reduction == 'sum':
            raise ValueError('avg_factor can not be used with reduction="sum"')     # losses/utils.py:50-51
        if not pred.is_cuda:
            raise NotImplementedError('FocalLoss runs on the GPU only (no CPU fallback); got a %s tensor' % pred.device)
        assert pred.dim() == 2 and target.dim() == 1 and target.shape[0] == pred.shape[0]
        if weight is not None:
            assert weight.dim() == 1 and weight.shape[0] == pred.shape[0], 'one weight per row (focal_loss.py:39-41)'
            weight = weight.float().contiguous()
        if reduction == 'none':
            loss = sigmoid_focal_loss(pred, target, self.gamma, self.alpha)
            if weight is not None:
                loss = loss * weight.view(-1, 1)
            return self.loss_weight * loss
        if pred.dtype != torch.float32:      # the reduced kernel reads f32 logits
            pred = pred.float()
        avg = float(pred.shape[0] * pred.shape[1]) if reduction == 'mean' and avg_factor is None else (1.0 if reduction == 'sum' else float(avg_factor))
        return FocalLossReducedFunction.apply(pred, target, weight, float(self.gamma), float(self.alpha), float(self.loss_weight), avg)
