"""Block-bootstrap intervals and p-values for the per-parcel Pearson r, HIP-backed: `BootstrapPearsonCorrCoef`.

`MultidimPearsonCorrCoef` gives a point estimate.  This class answers the two questions that follow it: which parcels are predicted
above chance and how wide is the interval around the mean r (`intervals`), and is one model's r really above another's
(`paired_difference`).  The resampling unit is a block -- one batch row of the `[B, V, T']` view, i.e. one stimulus segment: samples
inside a segment are autocorrelated, so segments, not samples, are drawn with replacement.  Segments are treated as exchangeable;
correlation that reaches across adjacent segments is not modelled (the intervals are then somewhat narrow).

State: the f64 `{Sx, Sy, Sxx, Syy, Sxy, n}` statistics of every block, `[capacity, V, 6]`, and the int64 group id of every block,
`[capacity]`, both on the device of the data and grown by doubling; the host keeps the block count only.  `update` writes the rows of
a batch into the slice `stats[n : n + B]` with the existing `ops.pearson_stats_update` and `group = arange(B)`: every (block, parcel)
cell receives exactly one flush onto zero, so the statistics are bit-reproducible.  A replicate is a count-weighted sum of block
statistics followed by the finaliser of `ops.pearson_from_stats` (csrc/bootstrap.hip); the observed r comes from the same kernel
with every count 1.  The draw depends on (seed, replicate, draw index, number of blocks) alone, so two metrics with equal seeds fed
the same segments are resampled identically and their replicate tables can be subtracted pairwise.  With groups (`GroupedMetric`:
subjects) only the blocks of the requested group are drawn: the bootstrap is stratified by subject.

Memory: 48 * blocks * V bytes of state (49 MB for 1024 blocks x 1000 parcels), 4 * num_bootstraps * blocks for the counts and
4 * num_bootstraps * V for the replicates while `intervals` runs.
"""

from __future__ import annotations

import dataclasses
import inspect
import typing as tp

import torch
from torch import nn

from tribe_hip import ops

from .base import _BASE_METRICS, BaseMetricConfig

MAX_BLOCKS = ops.BOOTSTRAP_MAX_BLOCKS
MAX_BOOTSTRAPS = ops.BOOTSTRAP_MAX_REPLICATES


@dataclasses.dataclass
class BootstrapResult:
    """Per parcel `[V]`: observed value, the first and last requested quantile of the replicates, their standard deviation (the
    bootstrap standard error), the p-value and the number of non-NaN replicates; the same for the mean over parcels (scalars).
    `quantile_values` `[n_q, V]` / `mean_quantile_values` `[n_q]` hold every requested quantile.  `p_value`: `intervals` gives
    (1 + #{r* <= 0}) / (m + 1), the one-sided test of H0: r <= 0; `paired_difference` the two-sided one."""

    observed: torch.Tensor
    lower: torch.Tensor
    upper: torch.Tensor
    std: torch.Tensor
    p_value: torch.Tensor
    n_valid: torch.Tensor
    mean_observed: torch.Tensor
    mean_lower: torch.Tensor
    mean_upper: torch.Tensor
    mean_std: torch.Tensor
    mean_p_value: torch.Tensor
    mean_n_valid: torch.Tensor
    quantile_values: torch.Tensor
    mean_quantile_values: torch.Tensor
    replicates: torch.Tensor | None = None        # [num_bootstraps, V], raw=True only
    mean_replicates: torch.Tensor | None = None   # [num_bootstraps]


def _is_int(x: tp.Any) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class BootstrapPearsonCorrCoef(nn.Module):
    is_differentiable: bool = False
    higher_is_better: bool = True
    full_state_update: bool = True
    grouped_state: bool = True   # GroupedMetric builds this class as its state (it keeps the group id of every block itself)

    def __init__(self, num_outputs: int = 1, num_bootstraps: int = 1000, quantiles: tp.Sequence[float] = (0.025, 0.975), seed: int = 0):
        super().__init__()
        if not _is_int(num_outputs) or num_outputs < 1:
            raise ValueError(f"num_outputs must be a positive integer, got {num_outputs!r}")
        if not _is_int(num_bootstraps) or not 1 <= num_bootstraps <= MAX_BOOTSTRAPS:
            raise ValueError(f"num_bootstraps must be an integer in [1, {MAX_BOOTSTRAPS}], got {num_bootstraps!r}")
        try:
            qs = tuple(float(q) for q in quantiles)
        except (TypeError, ValueError):
            raise ValueError(f"quantiles must be a sequence of numbers in [0, 1], got {quantiles!r}") from None
        if not qs or not all(0.0 <= q <= 1.0 for q in qs):
            raise ValueError(f"quantiles must be a non-empty sequence of numbers in [0, 1], got {quantiles!r}")
        if not _is_int(seed) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        self.num_outputs, self.num_bootstraps, self.quantiles, self.seed = num_outputs, num_bootstraps, qs, seed
        self._stats: torch.Tensor | None = None    # f64 [capacity, V, 6] on the device of the data; rows >= _n are zero
        self._groups: torch.Tensor | None = None   # int64 [capacity], same device: the group of every block
        self._n = 0                                # blocks held
        self.n_groups = 0

    # -- state ---------------------------------------------------------------------------------------------------------------
    def _reserve(self, n_new: int, device: torch.device) -> None:
        """Room for n_new more blocks; growing doubles the capacity and copies on the device."""
        if self._stats is not None and self._stats.device != device:
            self._stats, self._groups = self._stats.to(device), self._groups.to(device)
        cap = 0 if self._stats is None else self._stats.shape[0]
        need = self._n + n_new
        if need <= cap:
            return
        new_cap = max(64, 2 * cap, need)
        stats = torch.zeros(new_cap, self.num_outputs, 6, dtype=torch.float64, device=device)
        groups = torch.zeros(new_cap, dtype=torch.int64, device=device)
        if self._stats is not None and self._n:
            stats[: self._n].copy_(self._stats[: self._n])
            groups[: self._n].copy_(self._groups[: self._n])
        self._stats, self._groups = stats, groups

    def reset(self) -> None:
        if self._stats is not None and self._n:
            self._stats[: self._n].zero_()   # the buffers are kept for the next epoch; an update adds onto zero
        self._n = 0
        self.n_groups = 0

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
        return x.t().unsqueeze(0)   # [1, V, N] strided view of the matrix: one block

    @torch.no_grad()
    def update_bvt(self, preds: torch.Tensor, target: torch.Tensor, group: torch.Tensor | None = None, n_groups: int = 1) -> None:
        """Every batch row of [B, V, T] (or the whole of [N, V]) becomes one block; group int64 [B] gives the group of every row."""
        p, t = self._as_bvt(preds), self._as_bvt(target)
        if p.shape[1] != self.num_outputs:
            raise ValueError(f"expected {self.num_outputs} outputs, got {p.shape[1]}")
        if p.shape != t.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} differ")
        B = p.shape[0]
        if B == 0 or p.shape[2] == 0:
            return
        if self._n + B > MAX_BLOCKS:
            raise ValueError(f"BootstrapPearsonCorrCoef: {self._n + B} blocks exceed {MAX_BLOCKS}.  A block is one batch row: pass "
                             "[B, V, T'] predictions and targets (one block per segment, the 3-D form BrainModule passes) rather than "
                             "[N, V] rows through GroupedMetric, whose 2-D path makes every row a block of its own")
        if p.stride() != t.stride():   # the kernel reads both with one set of strides
            p, t = p.contiguous(), t.contiguous()
        self._reserve(B, p.device)
        n = self._n
        ops.pearson_stats_update(self._stats[n: n + B], p, t, torch.arange(B, dtype=torch.int64, device=p.device))
        if group is None:
            self._groups[n: n + B] = 0
        else:
            self._groups[n: n + B] = group.to(device=p.device, dtype=torch.int64).flatten()
        self._n = n + B
        self.n_groups = max(self.n_groups, int(n_groups), 1)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update_bvt(preds, target)

    # -- results -------------------------------------------------------------------------------------------------------------
    def _require(self) -> torch.Tensor:
        if self._stats is None or self._n == 0:
            raise RuntimeError("compute() called before update()")
        return self._stats[: self._n]

    def _blocks_of(self, group: int) -> torch.Tensor:
        """int64 [n_sel]: the blocks of `group`, ascending (one host synchronisation, where a result is wanted anyway)."""
        return torch.nonzero(self._groups[: self._n] == group).flatten()

    def per_output(self) -> torch.Tensor:
        """observed r f32 [G, V]; a group without blocks is NaN."""
        stats = self._require()
        out = torch.full((self.n_groups, self.num_outputs), float("nan"), dtype=torch.float32, device=stats.device)
        for g in range(self.n_groups):
            blocks = self._blocks_of(g)
            if blocks.numel():
                out[g] = ops.bootstrap_pearson(stats, blocks, None)[0]
        return out

    def compute(self) -> torch.Tensor:
        stats = self._require()
        blocks = self._blocks_of(0)
        if not blocks.numel():
            return torch.full((), float("nan"), dtype=torch.float32, device=stats.device)
        return ops.bootstrap_pearson(stats, blocks, None)[2].clone()

    def _replicates(self, group: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        stats = self._require()
        blocks = self._blocks_of(group)
        if not blocks.numel():
            raise ValueError(f"BootstrapPearsonCorrCoef: group {group} holds no block")
        counts = ops.bootstrap_counts(self.seed, self.num_bootstraps, blocks.numel(), stats.device)
        return ops.bootstrap_pearson(stats, blocks, counts)

    def _summarise(self, observed: torch.Tensor, replicates: torch.Tensor, mean_observed: torch.Tensor, mean_replicates: torch.Tensor,
                   two_sided: bool, raw: bool) -> BootstrapResult:
        V = self.num_outputs
        table = torch.cat([replicates, mean_replicates.unsqueeze(1)], 1)   # [n, V + 1]: the parcels, then the mean over parcels
        qv, sd, n_le, n_ge, n_valid = ops.bootstrap_summary(table, self.quantiles)
        p_le, _, p_two = ops.bootstrap_p_values(n_le, n_ge, n_valid)
        p = p_two if two_sided else p_le
        return BootstrapResult(observed, qv[0, :V], qv[-1, :V], sd[:V], p[:V], n_valid[:V],
                               mean_observed, qv[0, V], qv[-1, V], sd[V], p[V], n_valid[V], qv[:, :V], qv[:, V],
                               replicates if raw else None, mean_replicates if raw else None)

    def intervals(self, group: int = 0, raw: bool = False) -> BootstrapResult:
        """Percentile intervals (the first and last of `quantiles`), bootstrap standard error and the one-sided p-value of H0: r <= 0,
        per parcel and for the mean over parcels, from `num_bootstraps` resamplings of the blocks of `group`."""
        return self._summarise(*self._replicates(group), two_sided=False, raw=raw)

    def paired_difference(self, other: "BootstrapPearsonCorrCoef", group: int = 0) -> BootstrapResult:
        """The same summary for r_self - r_other under one shared resampling; `p_value` is two-sided.  Both metrics must have been fed
        the same blocks in the same order (equal seed, num_bootstraps, num_outputs, block count and block groups)."""
        if not isinstance(other, BootstrapPearsonCorrCoef):
            raise TypeError(f"paired_difference: expected a BootstrapPearsonCorrCoef, got {type(other)}")
        for name in ("seed", "num_bootstraps", "num_outputs"):
            if getattr(self, name) != getattr(other, name):
                raise ValueError(f"paired_difference: {name} differs ({getattr(self, name)} vs {getattr(other, name)}): the two resamplings "
                                 "would not be the same")
        if self._n != other._n:
            raise ValueError(f"paired_difference: block counts differ ({self._n} vs {other._n})")
        self._require()
        if not torch.equal(self._groups[: self._n], other._groups[: other._n].to(self._groups.device)):
            raise ValueError("paired_difference: the blocks' groups differ: the two metrics were not fed the same segments")
        mine, theirs = self._replicates(group), other._replicates(group)
        return self._summarise(*(a - b.to(a.device) for a, b in zip(mine, theirs)), two_sided=True, raw=True)

    def sync(self, group: tp.Any = None) -> None:
        """Concatenate the blocks of every process of `group` in rank order (lengths first, then padded statistics and group ids).
        Every process calls it, with or without blocks of its own."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        if self._stats is None:
            raise RuntimeError("sync() called before update()")
        world, V, dev = dist.get_world_size(group), self.num_outputs, self._stats.device
        mine = torch.tensor([self._n, self.n_groups], dtype=torch.int64, device=dev)
        lens = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(lens, mine, group=group)
        lens_host = [v.tolist() for v in lens]
        longest, total = max(row[0] for row in lens_host), sum(row[0] for row in lens_host)
        if total > MAX_BLOCKS:
            raise ValueError(f"BootstrapPearsonCorrCoef: {total} blocks over all processes exceed {MAX_BLOCKS}")
        merged = []
        for state, shape in ((self._stats, (longest, V, 6)), (self._groups, (longest,))):
            padded = torch.zeros(shape, dtype=state.dtype, device=dev)
            padded[: self._n] = state[: self._n]
            parts = [torch.empty_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded, group=group)
            out = torch.zeros((max(total, 1),) + tuple(shape[1:]), dtype=state.dtype, device=dev)
            at = 0
            for part, (n, _) in zip(parts, lens_host):
                out[at: at + n] = part[:n]
                at += n
            merged.append(out)
        self._stats, self._groups = merged
        self._n, self.n_groups = total, max(row[1] for row in lens_host)


_BASE_METRICS["BootstrapPearsonCorrCoef"] = BootstrapPearsonCorrCoef


class BootstrapPearsonCorrCoefConfig(BaseMetricConfig):
    """{log_name, name, kwargs}, the shape of the reference's TorchMetricConfig; `kwargs` are checked against the constructor."""

    name: tp.Literal["BootstrapPearsonCorrCoef"] = "BootstrapPearsonCorrCoef"
    kwargs: dict[str, tp.Any] = {}

    def model_post_init(self, __context: tp.Any) -> None:
        accepted = set(inspect.signature(BootstrapPearsonCorrCoef.__init__).parameters) - {"self"}
        unknown = sorted(set(self.kwargs) - accepted)
        if unknown:   # pydantic reports a ValueError raised here as a ValidationError
            raise ValueError(f"{self.name}: unknown kwargs {unknown}; accepted: {sorted(accepted)}")

    def build(self) -> nn.Module:
        return BootstrapPearsonCorrCoef(**self.kwargs)
