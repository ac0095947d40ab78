"""Retrieval metrics `Rank` and `TopkAcc`, HIP-backed.

Mirror of /root/reference/modeling_utils/modeling_utils/metrics/metrics.py:66-218 (the reference's default experiment logs
`retrieval_top1` = TopkAcc(topk=1), grids/defaults.py:107-124).  For one `update(x [N, V], y [M, V], x_labels, y_labels)`:

  * s[n, m] = dot(x_n, y_m) / (1e-15 + ||y_m||)                         (`_compute_sim`, norm_kind "y")
  * t(n) = n without labels (N == M), else `y_labels.index(x_labels[n])`  (first occurrence; ValueError when absent)
  * rank = (#{s > s_true} + #{s >= s_true} - 1) / 2, comparisons with NaN false; rank < 0 (NaN true score) -> N // 2; then
    `relative` divides by M
  * the state is the concatenation of every call's ranks (torchmetrics' dist_reduce_fx="cat"); `Rank.compute()` is its mean,
    lower median or unbiased std, `TopkAcc.compute()` the fraction of ranks < topk.

The ranks come from csrc/metrics.hip without forming the [N, M] score matrix; `update_bvt(pred, target)` additionally fuses the
time-means of the retrieval branch of `_run_step` (pl_module.py:98-99).  The state is a device buffer that grows by doubling plus
a host-side count, so `update` neither synchronises with the host nor concatenates.  `sync(group)` all-gathers the rank buffers
of a process group (the reference drops TopkAcc under DDP, main.py:255-258; here it works).
"""

from __future__ import annotations

import typing as tp
from collections import defaultdict

import numpy as np
import torch
from torch import nn

from tribe_hip import ops

from .base import BaseMetricConfig, OnlinePearsonCorr  # noqa: F401  (re-exported: the reference defines it in this module)

_REDUCE_SLOT = {"mean": 0, "std": 1, "median": 2}


class Rank(nn.Module):
    is_differentiable: bool = False
    higher_is_better: bool = False
    full_state_update: bool = True

    def __init__(self, reduction: tp.Literal["mean", "median", "std"] = "median", relative: bool = False):
        super().__init__()
        self.reduction = reduction
        self.relative = relative
        self._buf: torch.Tensor | None = None   # f32 [capacity] on the device of the data
        self._count = 0

    # -- state ---------------------------------------------------------------------------------------------------------------
    @property
    def ranks(self) -> torch.Tensor:
        """The ranks of every update so far (a view of the state buffer)."""
        if self._buf is None:
            return torch.empty(0)
        return self._buf[: self._count]

    def _reserve(self, n: int, device: torch.device) -> torch.Tensor:
        """Room for n more ranks; returns the slice they go to."""
        if self._buf is not None and self._buf.device != device:
            self._buf = self._buf[: self._count].to(device)
        cap = 0 if self._buf is None else self._buf.numel()
        need = self._count + n
        if need > cap:
            grown = torch.empty(max(64, 2 * cap, need), dtype=torch.float32, device=device)
            if self._count:
                grown[: self._count].copy_(self._buf[: self._count])
            self._buf = grown
        return self._buf[self._count: need]

    def reset(self) -> None:
        self._count = 0   # the buffer is kept for the next epoch

    # -- similarity and ranks ------------------------------------------------------------------------------------------------
    @classmethod
    def _compute_sim(cls, x: torch.Tensor, y: torch.Tensor, norm_kind: str | None = "y", eps: float = 1e-15) -> torch.Tensor:
        if eps != 1e-15:
            raise ValueError(f"_compute_sim: the kernel uses eps = 1e-15, got {eps}")
        return ops.retrieval_scores(_matrix(x, "x"), _matrix(y, "y"), norm_kind)

    @staticmethod
    def _true_indices(n: int, m: int, x_labels: list | None, y_labels: list | None, device: torch.device) -> torch.Tensor | None:
        if x_labels is not None and y_labels is not None:
            if len(x_labels) != n or len(y_labels) != m:
                raise ValueError(f"labels: {len(x_labels)} / {len(y_labels)} for {n} queries and {m} gallery rows")
            idx = [y_labels.index(lab) for lab in x_labels]   # first occurrence; ValueError when absent (as the reference)
            return torch.tensor(idx, dtype=torch.int64).to(device, non_blocking=True)
        if x_labels is not None or y_labels is not None:
            raise ValueError("give both x_labels and y_labels or neither")
        if n != m:
            raise ValueError(f"without labels queries and gallery must have the same length, got {n} and {m}")
        return None

    def _compute_ranks(self, x: torch.Tensor, y: torch.Tensor, x_labels: list | None = None, y_labels: list | None = None,
                       out: torch.Tensor | None = None) -> torch.Tensor:
        x, y = _matrix(x, "x"), _matrix(y, "y")
        true_idx = self._true_indices(x.shape[0], y.shape[0], x_labels, y_labels, x.device)
        y_norm = ops.retrieval_prep(y, mean=False, norm_x=True)[2]
        return ops.retrieval_ranks(x, y, y_norm, true_idx, self.relative, out=out)

    @torch.no_grad()
    def update(self, x: torch.Tensor, y: torch.Tensor, x_labels: list | None = None, y_labels: list | None = None) -> None:
        self._compute_ranks(x, y, x_labels, y_labels, out=self._reserve(x.shape[0], x.device))
        self._count += x.shape[0]

    @torch.no_grad()
    def update_bvt(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        """update(pred.mean(-1), target.mean(-1)) for [B, V, T'] tensors (any common strides), means and norms fused: two launches."""
        pred, target = pred.detach(), target.detach()
        if target.dtype != torch.float32:
            target = target.float()
        if pred.dtype != torch.float32:
            pred = pred.float()
        if target.stride() != pred.stride():   # the kernel reads both with one set of strides
            pred, target = pred.contiguous(), target.contiguous()
        x, y, _, y_norm = ops.retrieval_prep(pred, target, mean=True, norm_y=True)
        ops.retrieval_ranks(x, y, y_norm, None, self.relative, out=self._reserve(x.shape[0], x.device))
        self._count += x.shape[0]

    # -- results -------------------------------------------------------------------------------------------------------------
    def _reduced(self, topk: float = 1.0) -> torch.Tensor | None:
        if self._count == 0:
            return None
        return ops.rank_reduce(self.ranks, topk)

    def compute(self) -> torch.Tensor:
        if self.reduction not in _REDUCE_SLOT:
            raise ValueError(f'Unknown aggregation {self.reduction} for computing metric. Available aggregations are: "mean", '
                             '"median" or "std".')
        out = self._reduced()
        return torch.tensor(float("nan")) if out is None else out[_REDUCE_SLOT[self.reduction]]

    def sync(self, group: tp.Any = None) -> None:
        """Concatenate the rank buffers of every process of `group` in rank order (lengths first, then padded data)."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        world = dist.get_world_size(group)
        mine = self.ranks.float()
        dev = mine.device
        n = torch.tensor([self._count], dtype=torch.int64, device=dev)
        lens = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(lens, n, group=group)
        lens_host = [int(v.item()) for v in lens]
        longest = max(lens_host)
        padded = torch.zeros(longest, dtype=torch.float32, device=dev)
        padded[: self._count] = mine
        parts = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded, group=group)
        self._buf = torch.cat([p[:k] for p, k in zip(parts, lens_host)])
        self._count = sum(lens_host)

    def _compute_macro_average(self, ranks: torch.Tensor, labels: list[str]) -> dict[str, float]:
        assert len(ranks) == len(labels)
        groups: dict[str, list] = defaultdict(list)
        agg_func = np.mean if self.reduction == "mean" else np.median
        for r, label in zip(_host(ranks), labels):
            groups[label].append(r)
        return {label: agg_func(values) for label, values in groups.items()}

    @classmethod
    def _compute_topk_scores(cls, x: torch.Tensor, y: torch.Tensor, y_labels: list[str], k: int = 5
                             ) -> tuple[list[list[str]], list[list[float]]]:
        scores = cls._compute_sim(x, y).cpu()
        topk_inds = torch.argsort(scores, dim=1, descending=True)[:, :k]
        topk_labels = [[y_labels[int(i)] for i in inds] for inds in topk_inds]
        return topk_labels, [[float(scores[n, int(i)]) for i in inds] for n, inds in enumerate(topk_inds)]


class TopkAcc(Rank):
    is_differentiable: bool = False
    higher_is_better: bool = True
    full_state_update: bool = True

    def __init__(self, topk: int = 5):
        super().__init__(relative=False)
        self.topk = topk

    def _compute_macro_average(self, ranks: torch.Tensor, labels: list[str]) -> dict[str, float]:
        groups: dict[str, list] = defaultdict(list)
        for r, label in zip(_host(ranks), labels):
            groups[label].append(r)
        return {label: float(np.mean([r < self.topk for r in values])) for label, values in groups.items()}

    def compute(self) -> torch.Tensor:
        out = self._reduced(self.topk)
        return torch.tensor(float("nan")) if out is None else out[3]


def _matrix(x: torch.Tensor, name: str) -> torch.Tensor:
    if x.ndim != 2:
        raise ValueError(f"{name}: expected [rows, V], got {tuple(x.shape)}")
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def _host(ranks: torch.Tensor) -> list[float]:
    return ranks.detach().cpu().tolist() if isinstance(ranks, torch.Tensor) else list(ranks)


# -- configs (the reference derives one per custom metric from its __init__ signature, metrics/base.py:105-113) -----------------
class RankConfig(BaseMetricConfig):
    name: tp.Literal["Rank"] = "Rank"
    reduction: tp.Literal["mean", "median", "std"] = "median"
    relative: bool = False

    def build(self) -> nn.Module:
        return Rank(reduction=self.reduction, relative=self.relative)


class TopkAccConfig(BaseMetricConfig):
    name: tp.Literal["TopkAcc"] = "TopkAcc"
    topk: int = 5

    def build(self) -> nn.Module:
        return TopkAcc(topk=self.topk)


class OnlinePearsonCorrConfig(BaseMetricConfig):
    name: tp.Literal["OnlinePearsonCorr"] = "OnlinePearsonCorr"
    dim: int
    reduction: tp.Literal["mean", "sum", "none"] | None = "mean"

    def build(self) -> nn.Module:
        return OnlinePearsonCorr(dim=self.dim, reduction=self.reduction)

