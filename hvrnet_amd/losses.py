"""Loss modules built from config dicts (registry.LOSSES / registry.build_loss).

FocalLoss below; SmoothL1Loss, BalancedL1Loss, MSELoss, IoULoss, BoundedIoULoss (mmdet/models/losses/smooth_l1_loss.py,
balanced_l1_loss.py, mse_loss.py, iou_loss.py) over csrc/reg_loss.hip and GHMC, GHMR (ghm_loss.py) over csrc/ghm.hip further down.

Mirror of mmdet/models/losses/focal_loss.py with losses/utils.py `weight_reduce_loss`: the sigmoid focal loss over the HIP kernels of
csrc/focal.hip (the rule, the reduction order and the one deviation from the reference are stated in include/hvr_hip.h).  There is
no PyTorch form of the loss here: CPU tensors raise, as every other op of the package does.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import native
from . import ops
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


# ---------------------------------------------------------------------------------------------- regression and IoU losses
class ReducedLossFunction(Function):
    """loss_weight / avg * sum w l in one pass (native.reg_loss / native.box_loss): the forward writes the gradient too, the backward
    scales it by the incoming scalar.  avg: a float, or an int32 device tensor whose first element, clamped to 1, divides.  -> 0-dim."""

    @staticmethod
    def forward(ctx, pred, target, weight, family, rule, params, loss_weight, avg):
        counts = avg if torch.is_tensor(avg) else None
        host = 1.0 if counts is not None else float(avg)
        fn = native.reg_loss if family == 'reg' else native.box_loss
        p = ops._rows(pred) if family == 'reg' else pred.float().contiguous()
        out1, d_pred = fn(rule, p, target.float().contiguous(), weight, loss_weight=loss_weight, avg=host, counts=counts, **params)
        ctx.save_for_backward(d_pred)
        return out1[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d_pred, = ctx.saved_tensors
        return (d_pred * g,) + (None,) * 7


class _WeightedLoss(nn.Module):
    """weighted_loss + the module's forward (losses/utils.py:36-98): 'none' takes the elementwise kernel, 'mean' / 'sum' the reduced one."""
    family, rule = 'reg', None

    def _params(self):
        return dict()

    def _weight(self, weight, loss_shape):
        if weight is None:
            return None
        assert tuple(weight.shape) == tuple(loss_shape), '%s: weight %s for a loss of shape %s' % (type(self).__name__, tuple(weight.shape), tuple(loss_shape))
        return weight.float().contiguous()

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        """-> [N, D] ('none'; IoULoss: [n]) or a 0-dim tensor.  avg_factor: a number, or an int32 device tensor (its first element, at
        least 1, divides: no host read)."""
        name = type(self).__name__
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError('reduction %r is none of "none", "mean", "sum"' % (reduction,))
        if avg_factor is not None and reduction == 'sum':
            raise ValueError('avg_factor can not be used with reduction="sum"')     # losses/utils.py:50-51
        if not pred.is_cuda:
            raise NotImplementedError('%s runs on the GPU only (no CPU fallback); got a %s tensor' % (name, pred.device))
        assert pred.dim() == 2 and pred.shape == target.shape and pred.numel() > 0, '%s: pred and target [N, D] of one shape' % name
        loss_shape = (pred.shape[0],) if self.rule == 'iou' else tuple(pred.shape)
        weight = self._weight(weight, loss_shape)
        if reduction == 'none':
            if self.family == 'reg':
                p = self._params()
                loss = ops.RegLossFunction.apply(pred, target, self.rule, p.get('beta', 0.0), p.get('alpha', 0.0), p.get('gamma', 0.0))
            else:
                p = self._params()
                loss = ops.BoxLossFunction.apply(pred, target, self.rule, p.get('beta', 0.0), p['eps'])
            if weight is not None:
                loss = loss * weight
            return self.loss_weight * loss
        if reduction == 'sum':
            avg = 1.0
        elif avg_factor is None:
            n = 1
            for k in loss_shape:
                n *= k
            avg = float(n)
        else:
            avg = avg_factor if torch.is_tensor(avg_factor) else float(avg_factor)
        return ReducedLossFunction.apply(pred, target, weight, self.family, self.rule, self._params(), float(self.loss_weight), avg)


@LOSSES.register_module
class SmoothL1Loss(_WeightedLoss):
    rule = 'smooth_l1'

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super(SmoothL1Loss, self).__init__()
        assert beta > 0
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def _params(self):
        return dict(beta=float(self.beta))


@LOSSES.register_module
class BalancedL1Loss(_WeightedLoss):
    """Balanced L1 Loss, arXiv 1904.02701."""
    rule = 'balanced_l1'

    def __init__(self, alpha=0.5, gamma=1.5, beta=1.0, reduction='mean', loss_weight=1.0):
        super(BalancedL1Loss, self).__init__()
        assert beta > 0 and alpha > 0 and gamma > 0
        self.alpha, self.gamma, self.beta, self.reduction, self.loss_weight = alpha, gamma, beta, reduction, loss_weight

    def _params(self):
        return dict(beta=float(self.beta), alpha=float(self.alpha), gamma=float(self.gamma))


@LOSSES.register_module
class MSELoss(_WeightedLoss):
    rule = 'mse'

    def __init__(self, reduction='mean', loss_weight=1.0):
        super(MSELoss, self).__init__()
        self.reduction, self.loss_weight = reduction, loss_weight


@LOSSES.register_module
class IoULoss(_WeightedLoss):
    family, rule = 'box', 'iou'

    def __init__(self, eps=1e-6, reduction='mean', loss_weight=1.0):
        super(IoULoss, self).__init__()
        assert eps > 0
        self.eps, self.reduction, self.loss_weight = eps, reduction, loss_weight

    def _params(self):
        return dict(eps=float(self.eps))


@LOSSES.register_module
class BoundedIoULoss(_WeightedLoss):
    family, rule = 'box', 'bounded_iou'

    def __init__(self, beta=0.2, eps=1e-3, reduction='mean', loss_weight=1.0):
        super(BoundedIoULoss, self).__init__()
        assert beta > 0 and eps > 0
        self.beta, self.eps, self.reduction, self.loss_weight = beta, eps, reduction, loss_weight

    def _params(self):
        return dict(beta=float(self.beta), eps=float(self.eps))


# ---------------------------------------------------------------------------------------------- GHM
class GHMFunction(Function):
    """One call of native.ghmc_loss / native.ghmr_loss: the loss (0-dim) with the gradient the same call wrote.  The module's acc_sum
    buffer is advanced in place by the kernel; `ws` keeps counts, bin weights, tot and n for the caller (module.last_ws)."""

    @staticmethod
    def forward(ctx, pred, target, weight, module):
        p = pred.float().contiguous()
        acc = module.acc_sum if module.momentum > 0 else None
        if isinstance(module, GHMC):
            t = target.contiguous() if target.dtype == torch.long and target.dim() == 1 else target.float().contiguous()
            out1, d, ws = native.ghmc_loss(p, t, weight.float().contiguous(), module.edges, module.momentum, acc, module.loss_weight)
        else:
            out1, d, ws = native.ghmr_loss(p, target.float().contiguous(), weight.float().contiguous(), module.edges, module.mu, module.momentum, acc,
                                           module.loss_weight)
        module.last_ws = ws
        ctx.save_for_backward(d)
        return out1[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d, = ctx.saved_tensors
        return d * g, None, None, None


def _ghm_edges(bins, last):
    assert 1 <= int(bins) <= 64, 'GHM: bins=%r (1 .. 64 on the HIP path)' % (bins,)
    edges = torch.arange(bins + 1).float() / bins
    if last is None:
        edges[-1] += 1e-6
    else:
        edges[-1] = last
    return edges


@LOSSES.register_module
class GHMC(nn.Module):
    """GHM classification loss, arXiv 1811.05181 (ghm_loss.py:18-93).  edges / acc_sum are buffers under the reference's names."""

    def __init__(self, bins=10, momentum=0, use_sigmoid=True, loss_weight=1.0):
        super(GHMC, self).__init__()
        self.bins, self.momentum = bins, momentum
        self.register_buffer('edges', _ghm_edges(bins, None))
        if momentum > 0:
            self.register_buffer('acc_sum', torch.zeros(bins))
        self.use_sigmoid = use_sigmoid
        if not self.use_sigmoid:
            raise NotImplementedError
        self.loss_weight = loss_weight
        self.last_ws = None

    def forward(self, pred, target, label_weight, *args, **kwargs):
        """pred [N, C] logits; target [N, C] binary with label_weight [N, C], or int64 labels [N] with label_weight [N] -> 0-dim."""
        if not pred.is_cuda:
            raise NotImplementedError('GHMC runs on the GPU only (no CPU fallback); got a %s tensor' % pred.device)
        assert pred.dim() == 2
        if pred.dim() != target.dim():
            assert target.dtype == torch.long and target.shape[0] == pred.shape[0] and label_weight.shape == target.shape
        else:
            assert target.shape == pred.shape and label_weight.shape == pred.shape
        return GHMFunction.apply(pred, target, label_weight, self)


@LOSSES.register_module
class GHMR(nn.Module):
    """GHM regression loss (ghm_loss.py:96-171)."""

    def __init__(self, mu=0.02, bins=10, momentum=0, loss_weight=1.0):
        super(GHMR, self).__init__()
        assert mu > 0
        self.mu, self.bins, self.momentum = mu, bins, momentum
        self.register_buffer('edges', _ghm_edges(bins, 1e3))
        if momentum > 0:
            self.register_buffer('acc_sum', torch.zeros(bins))
        self.loss_weight = loss_weight
        self.last_ws = None

    def forward(self, pred, target, label_weight, avg_factor=None):
        """pred, target, label_weight [N, 4 (* classes)] -> 0-dim.  avg_factor is accepted and ignored, as in the reference."""
        if not pred.is_cuda:
            raise NotImplementedError('GHMR runs on the GPU only (no CPU fallback); got a %s tensor' % pred.device)
        assert pred.dim() == 2 and target.shape == pred.shape and label_weight.shape == pred.shape
        return GHMFunction.apply(pred, target, label_weight, self)
