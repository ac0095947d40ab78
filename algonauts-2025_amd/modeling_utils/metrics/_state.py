"""The f64 [G, V, 6] streaming state shared by the Pearson metrics (base.py) and the regression metrics (regression.py)."""

from __future__ import annotations

import typing as tp

import torch
from torch import nn

from tribe_hip import ops


class _BvtStatsState(nn.Module):
    """f64 [G, V, 6] statistics, created on the first update (device follows the data).  A subclass names its `ops` update function
    in `_ops_update` and gives `_as_bvt` (input -> f32 [B, V, T] view) and `_check_width`."""

    def __init__(self, n_groups: int = 1):
        super().__init__()
        self.n_groups = n_groups
        self.stats: torch.Tensor | None = None

    def _check_width(self, width: int) -> None:
        """Refuse data whose number of outputs is not the state's."""

    def _ensure(self, device: torch.device, width: int, n_groups: int) -> None:
        if self.stats is None or self.stats.device != device:
            self.stats = torch.zeros(max(n_groups, self.n_groups), width, 6, dtype=torch.float64, device=device)
        elif self.stats.shape[0] < n_groups:
            grown = torch.zeros(n_groups, width, 6, dtype=torch.float64, device=device)
            grown[: self.stats.shape[0]] = self.stats
            self.stats = grown
        self.n_groups = self.stats.shape[0]

    def update_bvt(self, preds: torch.Tensor, target: torch.Tensor, group: torch.Tensor | None = None, n_groups: int = 1) -> None:
        p, t = self._as_bvt(preds), self._as_bvt(target)
        self._check_width(p.shape[1])
        self._ensure(p.device, p.shape[1], n_groups)
        getattr(ops, self._ops_update)(self.stats, p, t, group)

    def sync(self, group: tp.Any = None) -> None:
        import torch.distributed as dist

        if self.stats is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)

    def _require_stats(self) -> torch.Tensor:
        if self.stats is None:
            raise RuntimeError("compute() called before update()")
        return self.stats

    def reset(self) -> None:
        self.stats = None
