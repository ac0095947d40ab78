"""Streaming per-voxel Pearson metrics, HIP-backed.

Mirror of /root/reference/modeling_utils/modeling_utils/metrics/base.py:
  * `MultidimPearsonCorrCoef(num_outputs)` (base.py:26-29): `update(preds[N, V], target[N, V])`,
    `compute()` -> mean over outputs of the per-output Pearson r, `reset()`;
  * `GroupedMetric(metric_name, kwargs)` (base.py:39-91): one sub-metric per group id,
    `update(preds, target, groups)`, `compute()` -> {group_id: value}.
The reference inherits the running mean/var/cov update of `torchmetrics.PearsonCorrCoef`
(third-party, absent here -> "parity unpinned" for the streaming form); this build accumulates the
f64 sufficient statistics {Sx, Sy, Sxx, Syy, Sxy, n} per (group, voxel) on the GPU in one kernel
(tribe_pearson_stats_update) -- algebraically the same r, pinned against scipy.stats.pearsonr,
which is what the reference's own evaluation uses (main.py:459-477).  The pandas groupby of
base.py:67-78 is replaced by passing the group index of every batch row to the kernel.
`sync()` all-reduces the statistics over the process group (RCCL) for multi-GPU evaluation.

`TorchMetricConfig` / `GroupedMetric` also take the regression metrics of metrics/regression.py (MeanSquaredError,
MeanAbsoluteError, R2Score, ExplainedVariance), which keep a [G, V, 6] state of their own.
"""

from __future__ import annotations

import inspect
import typing as tp

import pydantic
import torch
from torch import nn

from tribe_hip import ops

from ._state import _BvtStatsState
from .regression import REGRESSION_METRICS


class _PearsonState(_BvtStatsState):
    _ops_update = "pearson_stats_update"

    def __init__(self, num_outputs: int, n_groups: int = 1):
        super().__init__(n_groups)
        self.num_outputs = num_outputs

    @staticmethod
    def _as_bvt(x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 3:
            return x.float()
        if x.ndim != 2:
            raise ValueError(f"expected [N, V] or [B, V, T], got {tuple(x.shape)}")
        return x.float().t().unsqueeze(0)  # [1, V, N] strided view of the flattened matrix

    def _check_width(self, width: int) -> None:
        if width != self.num_outputs:
            raise ValueError(f"expected {self.num_outputs} outputs, got {width}")

    def per_output(self) -> torch.Tensor:
        return ops.pearson_from_stats(self._require_stats())  # [G, V]


class MultidimPearsonCorrCoef(_PearsonState):
    def __init__(self, num_outputs: int = 1, **_: tp.Any):
        super().__init__(num_outputs, 1)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update_bvt(preds, target)

    def compute(self) -> torch.Tensor:
        return self.per_output()[0].mean()


class OnlinePearsonCorr(MultidimPearsonCorrCoef):
    """metrics.py:16-63: same statistic with `dim` / `reduction` options."""

    def __init__(self, dim: int = 0, reduction: str | None = "mean"):
        super().__init__(1)
        self.dim, self.reduction, self._initialized = dim, reduction, False

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if self.dim == 1:
            preds, target = preds.T, target.T
        if not self._initialized:
            self.num_outputs, self._initialized = preds.shape[1], True
        super().update(preds, target)

    def compute(self) -> torch.Tensor:
        r = self.per_output()[0]
        return r.mean() if self.reduction == "mean" else r.sum() if self.reduction == "sum" else r

    def reset(self) -> None:
        self._initialized = False
        super().reset()


# metrics/rank_corr.py adds "MultidimSpearmanCorrCoef" and metrics/bootstrap.py "BootstrapPearsonCorrCoef" (they import this module, so
# the entries are made there)
_BASE_METRICS = {"MultidimPearsonCorrCoef": MultidimPearsonCorrCoef, "OnlinePearsonCorr": OnlinePearsonCorr}


class GroupedMetric(nn.Module):
    def __init__(self, metric_name: str, kwargs: dict[str, tp.Any] | None = None) -> None:
        super().__init__()
        assert metric_name in _BASE_METRICS or metric_name in REGRESSION_METRICS, f"Metric {metric_name} not found"
        self.base_metric_cls = _BASE_METRICS.get(metric_name) or REGRESSION_METRICS[metric_name]
        self.metric_kwargs = kwargs or {}
        # Pearson: one [G, V, 6] state made on the first update; regression: the sub-metric itself holds the [G, V, 6] state
        self._regression = metric_name in REGRESSION_METRICS
        self._state: tp.Any = self.base_metric_cls(**self.metric_kwargs) if self._regression else None
        self._ids: list[str] = []  # group keys in first-seen order (groupby(sort=False), base.py:67)
        self._index: dict[str, int] = {}

    def update(self, preds: torch.Tensor, target: torch.Tensor, groups: tp.Optional[torch.Tensor] = None) -> None:
        """preds/target [N, V] with groups [N], or (fast path) [B, V, T] with groups [B] / [B, 1]."""
        n_rows = preds.shape[0]
        if groups is None:
            groups = torch.zeros(n_rows, dtype=torch.int64)
        groups = groups.flatten()
        assert len(groups) == n_rows, f"Groups must be the same shape as preds/target, got {groups.shape} and {preds.shape}"
        labels = groups.tolist()
        for lab in labels:
            key = str(lab)
            if key not in self._index:
                self._index[key] = len(self._ids)
                self._ids.append(key)
        slot = torch.tensor([self._index[str(lab)] for lab in labels], dtype=torch.int64, device=preds.device)
        if self._state is None:
            # a class that keeps the groups apart itself (rank_corr.py: it holds samples, not moments) is its own state
            if getattr(self.base_metric_cls, "grouped_state", False):
                self._state = self.base_metric_cls(**{"num_outputs": preds.shape[1], **self.metric_kwargs})
            else:
                self._state = _PearsonState(preds.shape[1])
        if preds.ndim == 1 and self._regression:  # [N]: one output
            preds, target = preds.unsqueeze(-1), target.unsqueeze(-1)
        if preds.ndim == 2:  # [N, V]: every row is its own "batch row" of length T = 1
            preds, target = preds.float().unsqueeze(-1), target.float().unsqueeze(-1)
        self._state.update_bvt(preds, target, slot, len(self._ids))

    def compute(self) -> dict[str, float]:
        if self._state is None or not self._ids:
            return {}
        if self._regression:
            scores = self._state.scores()  # [G], or [G, V] for a sub-metric that reports every output
            if scores.ndim != 1:
                raise ValueError(f"GroupedMetric needs one value per group, {self.base_metric_cls.__name__}({self.metric_kwargs}) gives "
                                 f"{scores.shape[1]} (multioutput='raw_values' or num_outputs > 1)")
            values = scores.tolist()
            return {gid: values[self._index[gid]] for gid in self._ids}
        r = self._state.per_output()  # [G, V]
        means = r.mean(dim=1).tolist()
        return {gid: means[self._index[gid]] for gid in self._ids}

    def intervals(self) -> dict[str, tp.Any]:
        """{group_id: result} of a sub-metric that resamples (metrics/bootstrap.py): every group from its own blocks."""
        if not hasattr(self.base_metric_cls, "intervals"):
            raise TypeError(f"{self.base_metric_cls.__name__} has no intervals()")
        if self._state is None or not self._ids:
            return {}
        return {gid: self._state.intervals(group=self._index[gid]) for gid in self._ids}

    def sync(self, group: tp.Any = None) -> None:
        if self._state is not None:
            self._state.sync(group)

    def reset(self) -> None:
        if self._state is not None:
            self._state.reset()

    def __repr__(self) -> str:
        return f"GroupedMetric({self.base_metric_cls.__name__})"


class BaseMetricConfig(pydantic.BaseModel):
    model_config = pydantic.ConfigDict(extra="forbid")
    log_name: str
    name: str

    def build(self) -> nn.Module:
        raise NotImplementedError


class MultidimPearsonCorrCoefConfig(BaseMetricConfig):
    """TorchMetricConfig shape of the reference (base.py:112-127): {log_name, name, kwargs}."""

    name: tp.Literal["MultidimPearsonCorrCoef"] = "MultidimPearsonCorrCoef"
    kwargs: dict[str, tp.Any] = {}

    def build(self) -> nn.Module:
        return MultidimPearsonCorrCoef(**self.kwargs)


class TorchMetricConfig(BaseMetricConfig):
    """The reference's TorchMetricConfig (base.py:116-127) for the torchmetrics regression metrics restated in metrics/regression.py;
    `kwargs` are checked against the constructor of the class (its validate_kwargs)."""

    name: tp.Literal["MeanSquaredError", "MeanAbsoluteError", "R2Score", "ExplainedVariance"]
    kwargs: dict[str, tp.Any] = {}

    def model_post_init(self, __context: tp.Any) -> None:
        accepted = set(inspect.signature(REGRESSION_METRICS[self.name].__init__).parameters) - {"self"}
        unknown = sorted(set(self.kwargs) - accepted)
        if unknown:   # pydantic reports a ValueError raised here as a ValidationError
            raise ValueError(f"{self.name}: unknown kwargs {unknown}; accepted: {sorted(accepted)}")

    def build(self) -> nn.Module:
        return REGRESSION_METRICS[self.name](**self.kwargs)


class GroupedMetricConfig(BaseMetricConfig):
    name: tp.Literal["GroupedMetric"] = "GroupedMetric"
    metric_name: str
    kwargs: dict[str, tp.Any] | None = None

    def build(self) -> nn.Module:
        return GroupedMetric(metric_name=self.metric_name, kwargs=self.kwargs)
