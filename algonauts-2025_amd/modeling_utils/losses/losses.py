"""HIP-backed losses of the TRIBE path.

`PearsonLoss` mirrors /root/reference/modeling_utils/modeling_utils/losses/losses.py:11-42
(1 - per-column Pearson with eps 1e-8, mean | sum over columns).  `MSELoss` is the HIP
counterpart of `torch.nn.MSELoss()` selected by defaults.py:125; `L1Loss`, `SmoothL1Loss` and
`HuberLoss` are those of the torch modules of the same name (grids/run_ensemble.py draws the last
two), and `hip_loss_for` maps a stock torch module to its counterpart.

All accept what the reference passes -- two [N, V] matrices, columns = voxels -- and, as the
fast path used by BrainModule, the un-flattened [B, V, T'] pair via `forward_bvt` (the '(b t) d'
flatten of pl_module.py:54-55 is a pure re-indexing of the same sums and is never materialised).
All are differentiable (HIP backward kernels, modeling_utils/autograd.py).
"""

from __future__ import annotations

import torch
from torch import nn

from tribe_hip import ops


def _as_bvt(x: torch.Tensor, dim: int) -> torch.Tensor:
    """[N, V] (voxels along `dim`) -> strided [1, V, N] view, no copy."""
    if x.ndim != 2:
        x = x.transpose(0, dim).reshape(x.shape[dim], -1).t()  # reference semantics for >2-D inputs (copying)
        dim = 1
    v = x if dim == 1 else x.t()
    return v.t().unsqueeze(0)  # [1, V, N]


class PearsonLoss(nn.Module):
    """1 - Pearson r per column (eps 1e-8 in the denominator), mean | sum over columns.

    A column whose one-pass variance is within rounding of 0 counts as constant: its covariance is 0 too.  For a constant
    prediction column the gradient is the finite term -k / den * (y - mean y) (den = 1e-8): the reference's autograd gives NaN
    there, because the derivative of sqrt at 0 is infinite and multiplies 0."""

    def __init__(self, reduction: str = "mean", dim: int = 1):
        super().__init__()
        self.reduction = reduction
        self.dim = dim

    def forward_bvt(self, pred: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
        if self.reduction not in ("mean", "sum"):
            raise ValueError(f"Invalid reduction: {self.reduction}")
        if torch.is_grad_enabled() and pred.requires_grad:
            from ..autograd import PearsonLossFn

            return PearsonLossFn.apply(pred.float(), true.float(), self.reduction)
        return ops.pearson_loss(pred.float(), true.float(), self.reduction)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self.forward_bvt(_as_bvt(x.float(), self.dim), _as_bvt(y.float(), self.dim))


def _check_reduction(name: str, reduction: str) -> None:
    if reduction == "none":
        raise NotImplementedError(f"the HIP {name} implements reduction='mean' and 'sum' (what the reference's grids configure), not 'none'")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"{reduction} is not a valid value for reduction")


class _ElemLoss(nn.Module):
    """An element-wise loss reduced over all elements: one HIP forward (ops.elem_loss) and one backward (autograd.ElemLoss).  The
    reduction does not depend on the element order, so [N, V] matrices and the un-flattened [B, V, T'] pair take the same path."""

    kind: str

    def __init__(self, reduction: str = "mean"):
        super().__init__()
        _check_reduction(type(self).__name__, reduction)
        self.reduction = reduction

    def _param(self) -> float:
        return 0.0

    def forward(self, pred: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
        name = type(self).__name__
        if pred.shape != true.shape:
            raise ValueError(f"{name}: shape mismatch {tuple(pred.shape)} vs {tuple(true.shape)}")
        _check_reduction(name, self.reduction)
        if torch.is_grad_enabled() and pred.requires_grad:
            from ..autograd import ElemLoss

            return ElemLoss.apply(pred.float(), true.float(), self.kind, self._param(), self.reduction)
        return ops.elem_loss(pred.float().contiguous(), true.float().contiguous(), self.kind, self._param(), self.reduction)

    forward_bvt = forward


class L1Loss(_ElemLoss):
    """mean | sum of |pred - true| (torch.nn.L1Loss); the gradient is sign(pred - true), 0 where they are equal."""

    kind = "l1"


class SmoothL1Loss(_ElemLoss):
    """torch.nn.SmoothL1Loss: 0.5 d^2 / beta for |d| < beta, |d| - 0.5 beta otherwise; beta == 0 is L1Loss.  A negative beta raises here, at
    construction, with the words torch uses at call time."""

    kind = "smooth_l1"

    def __init__(self, reduction: str = "mean", beta: float = 1.0):
        super().__init__(reduction)
        if beta < 0:
            raise ValueError("smooth_l1_loss does not support negative values for beta.")
        self.beta = beta

    def _param(self) -> float:
        return float(self.beta)


class HuberLoss(_ElemLoss):
    """torch.nn.HuberLoss: 0.5 d^2 for |d| <= delta, delta (|d| - 0.5 delta) otherwise.  Unlike torch, whose module constructs with any delta
    and fails at the first call, delta <= 0 raises here at construction (with torch's call-time words)."""

    kind = "huber"

    def __init__(self, reduction: str = "mean", delta: float = 1.0):
        super().__init__(reduction)
        if delta <= 0:
            raise ValueError("huber_loss does not support non-positive values for delta.")
        self.delta = delta

    def _param(self) -> float:
        return float(self.delta)


class MSELoss(_ElemLoss):
    """mean | sum of (pred - true)^2 over all elements (torch.nn.MSELoss); 'mean' is the reference's default loss."""

    kind = "mse"


def hip_loss_for(module: nn.Module) -> nn.Module | None:
    """The HIP counterpart, with the same hyper-parameters, of a stock torch.nn.MSELoss / L1Loss / SmoothL1Loss / HuberLoss whose reduction
    is 'mean' or 'sum'; None for everything else (subclasses, reduction='none', other losses, modules that already have forward_bvt)."""
    if getattr(module, "reduction", None) not in ("mean", "sum"):
        return None
    kind = type(module)
    if kind is nn.MSELoss:
        return MSELoss(reduction=module.reduction)
    if kind is nn.L1Loss:
        return L1Loss(reduction=module.reduction)
    if kind is nn.SmoothL1Loss and module.beta >= 0:
        return SmoothL1Loss(reduction=module.reduction, beta=module.beta)
    if kind is nn.HuberLoss and module.delta > 0:
        return HuberLoss(reduction=module.reduction, delta=module.delta)
    return None   # an invalid beta / delta is left to torch, which reports it at the call
