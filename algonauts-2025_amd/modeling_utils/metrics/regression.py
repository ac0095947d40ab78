"""Streaming regression metrics `MeanSquaredError`, `MeanAbsoluteError`, `R2Score` and `ExplainedVariance`, HIP-backed.

The reference builds any torchmetrics metric by name (`TorchMetricConfig`, metrics/base.py:116-127) and wraps any of them per
subject (`GroupedMetric`, :39-91).  torchmetrics is absent here, so the four regression metrics a brain-encoding run reports next to
Pearson are restated with torchmetrics' constructor arguments and `update(preds, target)` / `compute()` / `reset()`.

One kernel (tribe_regression_stats_update) accumulates f64 {sum d, sum d^2, sum |d|, sum t, sum t^2, n} per (group, output), with
d = target - preds formed in f64: the residual sums are direct, not derived from moments (sum d^2 = Sxx - 2 Sxy + Syy cancels when the
prediction follows the target on an offset, and sum |d| has no moment form).  The scores follow scikit-learn's documented
`force_finite=True` conventions, which the tests pin against `sklearn.metrics`:

  mse = sum d^2 / n, rmse = sqrt(mse), mae = sum |d| / n,
  r2 = 1 - rss / tss, explained_variance = 1 - var(d) / var(t);  tss == 0 -> 1 when the numerator is 0, else 0;
  n == 0 -> NaN;  r2 with n < 2 -> NaN.

`multioutput` is "raw_values", "uniform_average" or "variance_weighted" (weights tss; the uniform average when every tss is 0).
`MeanSquaredError` / `MeanAbsoluteError` with `num_outputs=1` pool every element, as torchmetrics' flattening does.
`sync()` all-reduces the statistics over the process group for multi-GPU evaluation.
"""

from __future__ import annotations

import torch

from tribe_hip import ops

from ._state import _BvtStatsState

_MULTIOUTPUT = ("raw_values", "uniform_average", "variance_weighted")


class _RegressionState(_BvtStatsState):
    """The width follows the data: the first update sets it, and subclasses with a declared number of outputs override `_check_width`."""

    _ops_update = "regression_stats_update"

    def _ensure(self, device: torch.device, width: int, n_groups: int) -> None:
        if self.stats is not None and self.stats.device == device and self.stats.shape[1] != width:
            raise ValueError(f"expected {self.stats.shape[1]} outputs as in the earlier updates, got {width}")
        super()._ensure(device, width, n_groups)

    @staticmethod
    def _as_bvt(x: torch.Tensor) -> torch.Tensor:
        x = x.detach().float()
        if x.ndim == 3:
            return x
        if x.ndim == 1:
            x = x.unsqueeze(1)   # [N]: one output
        if x.ndim != 2:
            raise ValueError(f"expected [N], [N, V] or [B, V, T], got {tuple(x.shape)}")
        return x.t().unsqueeze(0)  # [1, V, N] strided view of the flattened matrix


class _RegressionMetric(_RegressionState):
    """`scores()` is one value per group, [G], or per group and output, [G, V]; `compute()` is group 0 of it."""

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update_bvt(preds, target)

    def scores(self) -> torch.Tensor:
        raise NotImplementedError

    def compute(self) -> torch.Tensor:
        return self.scores()[0]

    def _reduced(self, kind: str, mode: str) -> torch.Tensor:
        """f32 [G, V] for "raw_values", else f32 [G] (reduced in f64, rounded once)."""
        stats = self._require_stats()
        if mode == "raw_values":
            return ops.regression_from_stats(stats, kind)
        return ops.regression_reduce(stats, kind, mode).float()


class _PerOutputOrPooled(_RegressionMetric):
    """torchmetrics' `num_outputs` rule: 1 flattens everything into one pooled score, V gives one score per output."""

    kind: str

    def __init__(self, num_outputs: int = 1):
        super().__init__()
        if not (isinstance(num_outputs, int) and num_outputs > 0):
            raise ValueError(f"Expected num_outputs to be a positive integer but got {num_outputs}")
        self.num_outputs = num_outputs

    def _check_width(self, width: int) -> None:
        if self.num_outputs != 1 and self.num_outputs != width:
            raise ValueError(f"expected {self.num_outputs} outputs, got {width}")

    def scores(self) -> torch.Tensor:
        return self._reduced(self.kind, "pooled" if self.num_outputs == 1 else "raw_values")


class MeanSquaredError(_PerOutputOrPooled):
    def __init__(self, squared: bool = True, num_outputs: int = 1):
        super().__init__(num_outputs)
        self.squared = squared

    @property
    def kind(self) -> str:  # type: ignore[override]
        return "mse" if self.squared else "rmse"


class MeanAbsoluteError(_PerOutputOrPooled):
    kind = "mae"


class _Multioutput(_RegressionMetric):
    kind: str

    def __init__(self, multioutput: str = "uniform_average"):
        super().__init__()
        if multioutput not in _MULTIOUTPUT:
            raise ValueError(f"Invalid input to argument `multioutput`. Choose one of the following: {_MULTIOUTPUT}")
        self.multioutput = multioutput

    def scores(self) -> torch.Tensor:
        return self._reduced(self.kind, self.multioutput)


class ExplainedVariance(_Multioutput):
    kind = "explained_variance"


class R2Score(_Multioutput):
    """`adjusted` = k > 0 applies 1 - (1 - r2) (n - 1) / (n - k - 1) to the reduced score and leaves it as is when k >= n - 1.  This rule
    is restated from torchmetrics' documentation, not checked against the library: parity unpinned.  `num_outputs` (a constructor
    argument of older torchmetrics) is accepted and ignored: the width follows the data."""

    kind = "r2"

    def __init__(self, adjusted: int = 0, multioutput: str = "uniform_average", num_outputs: int | None = None):
        super().__init__(multioutput)
        if not isinstance(adjusted, int) or isinstance(adjusted, bool) or adjusted < 0:
            raise ValueError("`adjusted` parameter should be an integer larger or equal to 0.")
        self.adjusted = adjusted

    def scores(self) -> torch.Tensor:
        r2 = super().scores()
        if self.adjusted == 0:
            return r2
        n = self._require_stats()[:, 0, 5]                                  # every output of a group holds the same count
        n = n.reshape(-1, *([1] * (r2.ndim - 1)))
        k = float(self.adjusted)
        adj = 1.0 - (1.0 - r2.double()) * (n - 1.0) / (n - k - 1.0)
        return torch.where(n - 1.0 > k, adj, r2.double()).float()


REGRESSION_METRICS: dict[str, type[_RegressionMetric]] = {
    "MeanSquaredError": MeanSquaredError, "MeanAbsoluteError": MeanAbsoluteError, "R2Score": R2Score,
    "ExplainedVariance": ExplainedVariance,
}
