"""GPU: csrc/bootstrap.hip and BootstrapPearsonCorrCoef against the numpy restatement of tests/test_bootstrap_host.py.

Bounds (derived, none tuned):
  * counts, n_le / n_ge / n_valid and the p-values are integers or f32 roundings of f64 ratios of integers: `==`.
  * a replicate or observed r: 2^-24 = 2^-25 for the one rounding to f32 of a value in [-1, 1] + 2^-25 of slack over the f64
    accumulation error, which is <= N 2^-53 (1 + mean^2 / var) times a small constant: < 1e-9 for N <= 1e6 samples when every column's
    |mean| <= its standard deviation (signal_data: N(0, 1) noise + 0.3 signal).  The reference is the restatement applied to the block
    statistics downloaded from the device with the same counts, so only the resampling and the finaliser are compared.
  * a quantile: 2^-24 (two f64 evaluations 1e-16 apart may round to adjacent f32 values; one ulp is <= 2^-24 below 1); the standard
    deviation: relative 2^-23.
  * the mean over parcels against the f64 mean of the device's own f32 values: 2^-24 (again one rounding, two evaluations)."""

import dataclasses

import numpy as np
import pydantic
import pytest
import torch

from oracle import tribe_ref
from tests.test_bootstrap_host import counts_of, draws, mean_over_parcels, resample, signal_data, summary

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R_TOL = 2.0**-24
QUANTILES = (0.0, 0.025, 0.5, 0.975, 1.0)


def _gpu(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def _results_bit_equal(a, b) -> bool:
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if (x is None) != (y is None) or (x is not None and not _bits_equal(x, y)):
            return False
    return True


def _close(got: np.ndarray, want: np.ndarray, tol: float) -> bool:
    """equal NaN pattern and |got - want| <= tol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or (np.isnan(got) != np.isnan(want)).any():
        return False
    ok = ~np.isnan(want)
    return bool((np.abs(got[ok] - want[ok]) <= tol).all())


def _metric(V, **kwargs):
    from modeling_utils.metrics import BootstrapPearsonCorrCoef

    return BootstrapPearsonCorrCoef(V, **{"num_bootstraps": 33, "seed": 5, **kwargs})


# ------------------------------------------------------------------------------------------------
# counts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boot", [1, 7, 256])
def test_counts_equal_the_restatement(n_boot):
    from tribe_hip import ops

    for seed in (0, (1 << 32) + 5):
        for n_sel in (1, 2, 3, 4, 5, 63, 64, 65, 1000):
            got = ops.bootstrap_counts(seed, n_boot, n_sel, DEV)
            assert got.dtype == torch.int32 and got.shape == (n_boot, n_sel)
            assert (got.cpu().numpy() == counts_of(seed, n_boot, n_sel)).all(), (seed, n_sel)


def test_counts_with_a_histogram_above_64_kib():
    """n_sel = 20000: 80 KB of LDS, the launch that raises the kernel's dynamic LDS limit; and the limit itself, 32768."""
    from tribe_hip import ops

    for n_sel in (20000, 32768):
        got = ops.bootstrap_counts(9, 2, n_sel, DEV).cpu().numpy()
        assert (got == counts_of(9, 2, n_sel)).all()


# ------------------------------------------------------------------------------------------------
# replicates and observed r
# ------------------------------------------------------------------------------------------------
def _check_against_restatement(metric, n_blocks):
    from tribe_hip import ops

    stats = metric._stats[: metric._n]
    assert metric._n == n_blocks
    blocks = torch.arange(n_blocks, device=DEV)
    counts = ops.bootstrap_counts(metric.seed, metric.num_bootstraps, n_blocks, DEV)
    obs, rep, m_obs, m_rep = ops.bootstrap_pearson(stats, blocks, counts)
    w_obs, w_rep, _, _ = resample(stats.cpu().numpy(), np.arange(n_blocks), counts.cpu().numpy())
    obs, rep = obs.cpu().numpy(), rep.cpu().numpy()
    diff = np.abs(np.concatenate([rep, obs[None]]).astype(np.float64) - np.concatenate([w_rep, w_obs[None]]))
    worst = diff[np.isfinite(diff)].max() if np.isfinite(diff).any() else 0.0
    print(f"blocks {n_blocks} V {rep.shape[1]}: worst |r - restatement| = {worst:.3e}")
    assert _close(rep, w_rep, R_TOL) and _close(obs, w_obs, R_TOL)
    assert _close(m_rep.cpu().numpy(), mean_over_parcels(rep), R_TOL)
    assert _close(m_obs.cpu().numpy().reshape(1), mean_over_parcels(obs[None]), R_TOL)
    return obs, rep


@pytest.mark.parametrize("V", [1, 3, 65, 130])
@pytest.mark.parametrize("n_blocks", [1, 2, 7, 37, 300])
def test_replicates_equal_the_restatement(n_blocks, V):
    """T' = 4, 12: the float4 rows branch of the statistics kernel; 1, 13: its strided branch."""
    for T in (1, 4, 12, 13):
        x, y = signal_data(n_blocks, V, T, seed=n_blocks + 10 * V + T)
        metric = _metric(V)
        metric.update(_gpu(x), _gpu(y))
        _check_against_restatement(metric, n_blocks)


def test_two_dimensional_input_is_one_block_per_call():
    """[N, V] takes the transposed (strided) view: one block per update."""
    V = 5
    metric = _metric(V)
    for i, N in enumerate((9, 14, 30, 7)):
        x, y = signal_data(1, V, N, seed=70 + i)
        metric.update(_gpu(x[0].T), _gpu(y[0].T))
    assert metric._n == 4
    _check_against_restatement(metric, 4)


def test_degenerate_blocks():
    """Two one-sample blocks: NaN exactly where both draws coincide (28 of 64 replicates at seed 5), r = -1 elsewhere (the two points
    fall on a descending line).  A constant column is NaN in every replicate and in `observed`."""
    metric = _metric(1, num_bootstraps=64, seed=5)
    metric.update(torch.tensor([[[1.0]], [[2.0]]], device=DEV), torch.tensor([[[3.0]], [[1.0]]], device=DEV))
    res = metric.intervals(raw=True)
    d = draws(5, 64, 2)
    same = d[:, 0] == d[:, 1]
    rep = res.replicates.cpu().numpy()[:, 0]
    assert same.sum() == 28 and (np.isnan(rep) == same).all() and (rep[~same] == -1.0).all()
    assert float(res.observed[0]) == -1.0 and int(res.n_valid[0]) == 36
    assert float(res.lower[0]) == -1.0 and float(res.upper[0]) == -1.0 and float(res.std[0]) == 0.0
    assert float(res.p_value[0]) == np.float32(37 / 37)
    assert np.isnan(res.mean_replicates.cpu().numpy()[same]).all()

    x, y = signal_data(5, 2, 8, seed=3)
    x[:, 1, :] = 1.25
    metric = _metric(2)
    metric.update(_gpu(x), _gpu(y))
    res = metric.intervals(raw=True)
    assert torch.isnan(res.replicates[:, 1]).all() and torch.isnan(res.observed[1]) and not torch.isnan(res.replicates[:, 0]).any()
    assert int(res.n_valid[1]) == 0 and torch.isnan(res.lower[1]) and torch.isnan(res.std[1]) and torch.isnan(res.p_value[1])
    assert torch.isnan(res.mean_observed) and int(res.mean_n_valid) == 0 and torch.isnan(metric.compute())


def test_observed_r_against_the_existing_metrics():
    from modeling_utils.metrics import MultidimPearsonCorrCoef
    from tribe_hip import ops

    V = 65
    metric, plain = _metric(V), MultidimPearsonCorrCoef(V)
    for i, (B, T) in enumerate(((6, 12), (3, 12), (5, 13))):
        x, y = signal_data(B, V, T, seed=90 + i)
        metric.update(_gpu(x), _gpu(y))
        plain.update(_gpu(x), _gpu(y))
    observed = metric.per_output()
    assert observed.shape == (1, V)
    pooled = ops.pearson_from_stats(metric._stats[: metric._n].sum(0, keepdim=True))
    assert _close(observed.cpu().numpy(), pooled.cpu().numpy(), R_TOL)
    assert _close(observed.cpu().numpy(), plain.per_output().cpu().numpy(), R_TOL)
    assert abs(float(metric.compute()) - float(plain.compute())) <= 2.0**-23
    assert _bits_equal(metric.intervals().observed, observed[0])


# ------------------------------------------------------------------------------------------------
# summary
# ------------------------------------------------------------------------------------------------
def _table(n: int, seed: int) -> np.ndarray:
    """f32 [n, 6]: no NaN; about half NaN; all NaN; exact ties at +0.0 / -0.0 among a few values; all negative; about half NaN with ties."""
    rng = np.random.default_rng(seed)
    t = np.clip(rng.standard_normal((n, 6)) * 0.3, -1, 1).astype(np.float32)
    t[rng.random(n) < 0.5, 1] = np.nan
    t[:, 2] = np.nan
    t[:, 3] = np.array([0.0, -0.0, 0.25, -0.5, 0.0], dtype=np.float32)[rng.integers(0, 5, n)]
    t[:, 4] = -np.abs(t[:, 4]) - 0.01
    t[:, 5] = np.array([0.0, -0.0, 0.125, -0.125], dtype=np.float32)[rng.integers(0, 4, n)]
    t[rng.random(n) < 0.5, 5] = np.nan
    return t


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1025, 16384])
def test_summary_equals_numpy(n):
    from tribe_hip import ops

    t = _table(n, seed=n)
    qv, sd, n_le, n_ge, n_valid = ops.bootstrap_summary(_gpu(t), QUANTILES)
    want = summary(t, QUANTILES)
    assert qv.shape == (len(QUANTILES), 6) and _close(qv.cpu().numpy(), want["q"], 2.0**-24)
    got_sd = sd.cpu().numpy().astype(np.float64)
    assert (np.isnan(got_sd) == np.isnan(want["std"])).all()
    ok = ~np.isnan(want["std"])
    assert (np.abs(got_sd[ok] - want["std"][ok]) <= 2.0**-23 * want["std"][ok]).all()
    for got, key in ((n_le, "n_le"), (n_ge, "n_ge"), (n_valid, "n_valid")):
        assert got.dtype == torch.int32 and (got.cpu().numpy() == want[key]).all(), key
    for got, key in zip(ops.bootstrap_p_values(n_le, n_ge, n_valid), ("p_le", "p_ge", "p_two")):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and (np.isnan(got) == np.isnan(want[key])).all()
        assert (got[~np.isnan(got)] == want[key][~np.isnan(got)]).all(), key
    # a strided view (the replicate table's layout: rows of V + 1 values) gives the same bits
    wide = torch.full((n, 9), 7.0, device=DEV)
    wide[:, :6] = _gpu(t)
    again = ops.bootstrap_summary(wide[:, :6], QUANTILES)
    assert all(_bits_equal(a, b) for a, b in zip(again, (qv, sd, n_le, n_ge, n_valid)))


def test_intervals_equal_the_restatement():
    """The whole chain on one metric: counts, replicates, the summary of the parcels and of the mean column."""
    V, nb = 7, 37
    x, y = signal_data(nb, V, 12, seed=21)
    metric = _metric(V, num_bootstraps=200, quantiles=QUANTILES, seed=(1 << 40) + 3)
    metric.update(_gpu(x), _gpu(y))
    res = metric.intervals(raw=True)
    obs, rep, m_obs, m_rep = resample(metric._stats[:nb].cpu().numpy(), np.arange(nb), counts_of(metric.seed, 200, nb))
    assert _close(res.replicates.cpu().numpy(), rep, R_TOL) and _close(res.observed.cpu().numpy(), obs, R_TOL)
    for table, values, lower, upper, std, p, m in (
            (res.replicates, res.quantile_values, res.lower, res.upper, res.std, res.p_value, res.n_valid),
            (res.mean_replicates[:, None], res.mean_quantile_values[:, None], res.mean_lower[None], res.mean_upper[None], res.mean_std[None],
             res.mean_p_value[None], res.mean_n_valid[None])):
        want = summary(table.cpu().numpy(), QUANTILES)                     # of the device's own replicates
        assert _close(values.cpu().numpy(), want["q"], 2.0**-24)
        assert _bits_equal(lower, values[0]) and _bits_equal(upper, values[-1])
        assert (np.abs(std.cpu().numpy() - want["std"]) <= 2.0**-23 * want["std"]).all()
        assert (p.cpu().numpy() == want["p_le"]).all() and (m.cpu().numpy() == 200).all()
    assert (res.lower <= res.upper).all()
    assert metric.intervals().replicates is None


# ------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_or_on_how_blocks_arrive():
    V = 65
    x, y = signal_data(130, V, 12, seed=31)
    xg, yg = _gpu(x), _gpu(y)

    a = _metric(V)
    a.update(xg[:6], yg[:6])
    first, second = a.intervals(raw=True), a.intervals(raw=True)
    assert _results_bit_equal(first, second)
    b = _metric(V)
    b.update(xg[:3], yg[:3])
    b.update(xg[3:6], yg[3:6])
    assert _bits_equal(a._stats[:6], b._stats[:6]) and _results_bit_equal(first, b.intervals(raw=True))

    whole, parts = _metric(V), _metric(V)
    whole.update(xg, yg)
    for i in range(0, 130, 26):                                            # capacity 64 -> 128 -> 256
        parts.update(xg[i: i + 26], yg[i: i + 26])
    assert parts._stats.shape[0] == 256 and parts._n == whole._n == 130
    assert _results_bit_equal(whole.intervals(raw=True), parts.intervals(raw=True))
    # reset keeps the buffers and leaves them zero: the next epoch gives the same bits
    parts.reset()
    assert parts._n == 0 and parts._stats.shape[0] == 256 and not parts._stats.any()
    parts.update(xg[:6], yg[:6])
    assert _results_bit_equal(first, parts.intervals(raw=True))


# ------------------------------------------------------------------------------------------------
# pairing
# ------------------------------------------------------------------------------------------------
def test_paired_difference():
    V, nb = 9, 37
    xa, y = signal_data(nb, V, 12, seed=41, noise=1.0)
    xb, y2 = signal_data(nb, V, 12, seed=41, noise=2.0)
    assert (y == y2).all()
    a, a2, b = (_metric(V, num_bootstraps=200, seed=8) for _ in range(3))
    a.update(_gpu(xa), _gpu(y))
    a2.update(_gpu(xa), _gpu(y))
    b.update(_gpu(xb), _gpu(y))

    same = a.paired_difference(a2)
    assert not same.replicates.any() and not same.observed.any() and not same.mean_replicates.any()
    assert (same.p_value == 1.0).all() and float(same.mean_p_value) == 1.0 and (same.lower == 0).all() and (same.upper == 0).all()

    diff = a.paired_difference(b)
    counts = counts_of(8, 200, nb)
    ra, rb = (resample(m._stats[:nb].cpu().numpy(), np.arange(nb), counts) for m in (a, b))
    want = summary(ra[1] - rb[1], a.quantiles)
    want_mean = summary((ra[3] - rb[3])[:, None], a.quantiles)
    tol = 2.0**-23
    assert _close(diff.observed.cpu().numpy(), ra[0] - rb[0], tol)
    assert _close(diff.lower.cpu().numpy(), want["q"][0], tol) and _close(diff.upper.cpu().numpy(), want["q"][-1], tol)
    assert _close(diff.mean_lower.cpu().numpy(), want_mean["q"][0, 0], tol) and _close(diff.mean_upper.cpu().numpy(), want_mean["q"][-1, 0], tol)
    own = summary(diff.replicates.cpu().numpy(), a.quantiles)              # the two-sided p-value of the device's own difference table
    own_mean = summary(diff.mean_replicates.cpu().numpy()[:, None], a.quantiles)
    assert (diff.p_value.cpu().numpy() == own["p_two"]).all()
    assert float(diff.mean_p_value) == own_mean["p_two"][0]
    with pytest.raises(ValueError, match="seed"):
        a.paired_difference(_metric(V, num_bootstraps=200, seed=9))


# ------------------------------------------------------------------------------------------------
# grouping
# ------------------------------------------------------------------------------------------------
def test_grouped_metric_resamples_every_subject_from_its_own_blocks():
    from modeling_utils.metrics import GroupedMetric

    V, T = 5, 12
    x, y = signal_data(24, V, T, seed=51)
    subjects = np.array([3, 1, 3, 7, 1, 3, 7, 7, 1, 3, 3, 1] * 2)
    grouped = GroupedMetric("BootstrapPearsonCorrCoef", {"num_bootstraps": 33, "seed": 5})
    for lo in (0, 8, 16):
        grouped.update(_gpu(x[lo: lo + 8]), _gpu(y[lo: lo + 8]), groups=torch.from_numpy(subjects[lo: lo + 8]).view(-1, 1))
    results, means = grouped.intervals(), grouped.compute()
    assert list(results) == list(means) == ["3", "1", "7"]                 # first-seen order
    for sid in (3, 1, 7):
        alone = _metric(V)
        alone.update(_gpu(x[subjects == sid]), _gpu(y[subjects == sid]))
        want = alone.intervals()
        assert _results_bit_equal(results[str(sid)], want), sid
        r = want.observed.cpu().numpy().astype(np.float64)
        # GroupedMetric.compute() takes the f32 mean of V values: a rounding per add of partial sums no larger than sum |r|
        assert abs(means[str(sid)] - r.mean()) <= 2.0**-25 + V * 2.0**-24 * np.abs(r).mean(), sid


def test_grouped_metric_two_dimensional_rows_are_blocks():
    """[N, V] rows through GroupedMetric: every row a block of one sample, resampled within its group."""
    from modeling_utils.metrics import GroupedMetric

    V, N = 3, 40
    x, y = signal_data(1, V, N, seed=61)
    x, y = x[0].T.copy(), y[0].T.copy()
    groups = np.arange(N) % 2
    grouped = GroupedMetric("BootstrapPearsonCorrCoef", {"num_bootstraps": 33, "seed": 5})
    grouped.update(_gpu(x), _gpu(y), groups=torch.from_numpy(groups))
    state = grouped._state
    assert state._n == N and state.n_groups == 2
    res = grouped.intervals()
    for g in (0, 1):
        blocks = np.nonzero(groups == g)[0]
        obs, rep, _, _ = resample(state._stats[:N].cpu().numpy(), blocks, counts_of(5, 33, len(blocks)))
        assert _close(res[str(g)].observed.cpu().numpy(), obs, R_TOL)
        lower = summary(rep, state.quantiles)["q"][0]
        assert _close(res[str(g)].lower.cpu().numpy(), lower, 2.0**-23)


# ------------------------------------------------------------------------------------------------
# BrainModule
# ------------------------------------------------------------------------------------------------
def test_brain_module_validation_step_feeds_the_metric():
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig
    from modeling_utils.metrics import MetricConfig
    from tests.test_gpu_model import _cuda_batch, _small_pair

    fdims = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
    V, Tout, S = 50, 10, 4
    ref, m = _small_pair(fdims, V, Tout, S)
    adapter = pydantic.TypeAdapter(MetricConfig)
    cfgs = [{"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": V}},
            {"log_name": "pearson_ci", "name": "BootstrapPearsonCorrCoef", "kwargs": {"num_outputs": V, "num_bootstraps": 64}},
            {"log_name": "subj_pearson_ci", "name": "GroupedMetric", "metric_name": "BootstrapPearsonCorrCoef", "kwargs": {"num_bootstraps": 64}}]
    metrics = {f"val/{c['log_name']}": adapter.validate_python(c).build() for c in cfgs}
    bm = BrainModule(m, TorchLossConfig(name="MSELoss").build(), None, metrics)
    for i, subj in enumerate((torch.tensor([[2], [0], [2]]), torch.tensor([[3], [2], [0]]))):
        data = tribe_ref.synthetic_batch(3, 31, fdims, S, seed=40 + i)
        data["subject_id"] = subj
        with torch.no_grad():
            yr = ref(data)
        data["fmri"] = 0.3 * yr + torch.randn(yr.shape, generator=torch.Generator().manual_seed(50 + i))
        bm.validation_step(_cuda_batch(data), i)
    bm.on_validation_epoch_end()
    boot = metrics["val/pearson_ci"]
    assert bm.logged["val/pearson_ci"] is boot and boot._n == 6
    value = float(boot.compute())
    assert np.isfinite(value) and abs(value - float(metrics["val/pearson"].compute())) <= 2.0**-23
    res = boot.intervals()
    assert res.observed.shape == (V,) and bool(torch.isfinite(res.lower).all()) and bool((res.lower <= res.upper).all())
    assert float(res.mean_lower) <= float(res.mean_upper) and int(res.mean_n_valid) == 64
    keys = [k for k in bm.logged if k.startswith("val/subj_pearson_ci/")]
    assert keys == [f"val/subj_pearson_ci/{s}" for s in ("2", "0", "3")] and all(np.isfinite(bm.logged[k]) for k in keys)
    assert set(metrics["val/subj_pearson_ci"].intervals()) == {"2", "0", "3"}
