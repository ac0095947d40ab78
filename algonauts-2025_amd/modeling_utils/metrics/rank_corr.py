"""Spearman rank correlation per output, HIP-backed: `MultidimSpearmanCorrCoef`.

The companion of `MultidimPearsonCorrCoef` for heavy-tailed, outlier-ridden targets: Pearson's r of the average ranks of
predictions and targets, per output column, `compute()` = the mean over outputs.  The reference has no such class (its
`TorchMetricConfig` would hand the name `SpearmanCorrCoef` to torchmetrics, which is absent here and stays rejected); the name
follows its `MultidimPearsonCorrCoef`, and the semantics are scipy's: `scipy.stats.spearmanr(x, y)` per column with average ranks for
ties and `nan_policy="propagate"`; a constant column or fewer than two samples give NaN.  torchmetrics' `eps` in the denominator and
its 0 for a constant column are not reproduced ("parity unpinned" against torchmetrics).

Ranks need every sample, so the state is not a streaming moment: f32 `[G, V, capacity]` buffers of predictions and targets, one
contiguous run of samples per (group, output), that grow by doubling (copied on the device), plus the int64 sample counts `[G]`,
which live on the device: `update` appends through `ops.rank_append` without synchronising with the host.  The host only knows how
many samples it has appended since the last reset -- an upper bound of every group's count, which is what the capacity is kept
above.  `per_output()` reads the counts (the one host synchronisation, where a result is wanted anyway) and runs the sort-and-rank
kernels of csrc/rank_corr.hip once per group, so ranks are taken within each group's own rows (the reference's groupby semantics).
Memory: 2 * 4 * n * V bytes for n samples of one group; with G groups fed through `GroupedMetric` up to G times that, because every
group's run is sized for the bound.

`sync(group)` concatenates, per group id, the samples of every process of a process group in rank order (lengths first, then
padded data, as `Rank.sync`).
"""

from __future__ import annotations

import inspect
import typing as tp

import torch
from torch import nn

from tribe_hip import ops

from .base import _BASE_METRICS, BaseMetricConfig

MAX_SAMPLES = ops.SPEARMAN_MAX_SAMPLES   # per group: the int64 rank sums are exact up to 2^20 samples


class MultidimSpearmanCorrCoef(nn.Module):
    is_differentiable: bool = False
    higher_is_better: bool = True
    full_state_update: bool = True
    grouped_state: bool = True   # GroupedMetric builds this class as its state (it keeps the groups' samples apart itself)

    def __init__(self, num_outputs: int = 1):
        super().__init__()
        if isinstance(num_outputs, bool) or not isinstance(num_outputs, int) or num_outputs < 1:
            raise ValueError(f"num_outputs must be a positive integer, got {num_outputs!r}")
        self.num_outputs = num_outputs
        self._pred: torch.Tensor | None = None     # f32 [G, V, capacity] on the device of the data
        self._true: torch.Tensor | None = None
        self._counts: torch.Tensor | None = None   # int64 [G], same device: samples held per group
        self._total = 0                            # samples appended since the last reset: >= every entry of _counts

    # -- state ---------------------------------------------------------------------------------------------------------------
    @property
    def n_groups(self) -> int:
        return 0 if self._counts is None else self._counts.numel()

    def _reserve(self, n_new: int, n_groups: int, device: torch.device) -> None:
        """Room for n_new more samples in each of at least n_groups groups; growing copies on the device."""
        V = self.num_outputs
        if self._pred is not None and self._pred.device != device:
            self._pred, self._true, self._counts = self._pred.to(device), self._true.to(device), self._counts.to(device)
        G = max(n_groups, self.n_groups)
        cap = 0 if self._pred is None else self._pred.shape[2]
        need = self._total + n_new
        if need <= cap and G == self.n_groups:
            return
        new_cap = cap if need <= cap else max(64, 2 * cap, need)
        pred = torch.empty(G, V, new_cap, dtype=torch.float32, device=device)
        true = torch.empty(G, V, new_cap, dtype=torch.float32, device=device)
        counts = torch.zeros(G, dtype=torch.int64, device=device)
        if self._pred is not None:
            g, k = self.n_groups, self._total
            pred[:g, :, :k].copy_(self._pred[:, :, :k])
            true[:g, :, :k].copy_(self._true[:, :, :k])
            counts[:g].copy_(self._counts)
        self._pred, self._true, self._counts = pred, true, counts

    def reset(self) -> None:
        self._total = 0   # the buffers are kept for the next epoch
        if self._counts is not None:
            self._counts.zero_()

    # -- updates -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _as_bvt(x: torch.Tensor) -> torch.Tensor:
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.ndim == 3:
            return x
        if x.ndim != 2:
            raise ValueError(f"expected [N, V] or [B, V, T], got {tuple(x.shape)}")
        return x.t().unsqueeze(0)   # [1, V, N] strided view of the matrix

    @torch.no_grad()
    def update_bvt(self, preds: torch.Tensor, target: torch.Tensor, group: torch.Tensor | None = None, n_groups: int = 1) -> None:
        """Append [B, V, T] (or [N, V]) samples; group int64 [B] on the device gives the group of every batch row."""
        p, t = self._as_bvt(preds), self._as_bvt(target)
        if p.shape[1] != self.num_outputs:
            raise ValueError(f"expected {self.num_outputs} outputs, got {p.shape[1]}")
        if p.shape != t.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} differ")
        n_new = p.shape[0] * p.shape[2]
        if n_new == 0:
            return
        if group is None and self._total + n_new > MAX_SAMPLES:
            raise ValueError(f"MultidimSpearmanCorrCoef: {self._total + n_new} samples exceed 2^20")
        if p.stride() != t.stride():   # the kernel reads both with one set of strides
            p, t = p.contiguous(), t.contiguous()
        self._reserve(n_new, n_groups, p.device)
        ops.rank_append(self._pred, self._true, self._counts, p, t, group)
        self._total += n_new

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update_bvt(preds, target)

    # -- results -------------------------------------------------------------------------------------------------------------
    def per_output(self) -> torch.Tensor:
        """rho f32 [G, V]; a group without samples is NaN."""
        if self._counts is None or self._total == 0:
            raise RuntimeError("compute() called before update()")
        counts = self._counts.tolist()
        if max(counts) > MAX_SAMPLES:
            raise ValueError(f"MultidimSpearmanCorrCoef: {max(counts)} samples in one group exceed 2^20")
        out = torch.full((len(counts), self.num_outputs), float("nan"), dtype=torch.float32, device=self._pred.device)
        for g, n in enumerate(counts):
            if n > 0:
                out[g] = ops.spearman_from_state(self._pred[g], self._true[g], n)[0]
        return out

    def compute(self) -> torch.Tensor:
        return self.per_output()[0].double().mean().float()   # f64 mean: one more rounding, not V of them

    def sync(self, group: tp.Any = None) -> None:
        """Per group id, concatenate the samples of every process of `group` in rank order (lengths first, then padded data).
        Every process calls it, with or without samples of its own."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        if self._counts is None:
            raise RuntimeError("sync() called before update()")
        world, V, dev = dist.get_world_size(group), self.num_outputs, self._counts.device
        n_mine = torch.tensor([self.n_groups], dtype=torch.int64, device=dev)
        n_all = [torch.zeros_like(n_mine) for _ in range(world)]
        dist.all_gather(n_all, n_mine, group=group)
        G = max(int(v.item()) for v in n_all)
        mine = torch.zeros(G, dtype=torch.int64, device=dev)
        mine[: self.n_groups] = self._counts
        lens = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(lens, mine, group=group)
        lens_host = [v.tolist() for v in lens]
        own, longest = mine.tolist(), max(max(row) for row in lens_host)
        totals = [sum(row[g] for row in lens_host) for g in range(G)]
        gathered = []
        for state in (self._pred, self._true):
            padded = torch.zeros(G, V, longest, dtype=torch.float32, device=dev)
            for g in range(self.n_groups):
                padded[g, :, : own[g]] = state[g, :, : own[g]]
            parts = [torch.empty_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded, group=group)
            merged = torch.zeros(G, V, max(totals), dtype=torch.float32, device=dev)
            for g in range(G):
                at = 0
                for part, row in zip(parts, lens_host):
                    merged[g, :, at: at + row[g]] = part[g, :, : row[g]]
                    at += row[g]
            gathered.append(merged)
        self._pred, self._true = gathered
        self._counts = torch.tensor(totals, dtype=torch.int64, device=dev)
        self._total = max(totals)


_BASE_METRICS["MultidimSpearmanCorrCoef"] = MultidimSpearmanCorrCoef


class MultidimSpearmanCorrCoefConfig(BaseMetricConfig):
    """{log_name, name, kwargs}, the shape of the reference's TorchMetricConfig; `kwargs` are checked against the constructor."""

    name: tp.Literal["MultidimSpearmanCorrCoef"] = "MultidimSpearmanCorrCoef"
    kwargs: dict[str, tp.Any] = {}

    def model_post_init(self, __context: tp.Any) -> None:
        accepted = set(inspect.signature(MultidimSpearmanCorrCoef.__init__).parameters) - {"self"}
        unknown = sorted(set(self.kwargs) - accepted)
        if unknown:   # pydantic reports a ValueError raised here as a ValidationError
            raise ValueError(f"{self.name}: unknown kwargs {unknown}; accepted: {sorted(accepted)}")

    def build(self) -> nn.Module:
        return MultidimSpearmanCorrCoef(**self.kwargs)
