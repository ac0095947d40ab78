"""GPU: the regression-metric kernels (csrc/regression_metrics.hip), the metric classes on top of them and their use in
BrainModule, against the float64 restatement of tests/test_regression_metrics_host.py (which scikit-learn pins there).

Launch branches of the kernel pair that csrc/bvt_stats.h shares with the Pearson statistics: `rows` ([B, V, 100] contiguous ->
bvt_stats_rows_kernel<RegressionAcc>), `t99` ([B, V, 99]) and `nv` (the '(b t) v' matrix viewed as [B, V, 100], strides (100 V, 1, V))
-> bvt_stats_strided_kernel<RegressionAcc>; T = 1028 runs the rows kernel's four-deep loop and its remainder.  Rows are split over up to three updates that accumulate; group ids change inside one wave's rows and across row
chunks, ids -1 / G / G + 3 are skipped and group G - 1 receives nothing.

Bounds (u = 2^-53, k = n + 2 for the n adds behind a sum plus the roundings of d and d^2, on either side; no empirical tolerance):
  * counts: exactly equal;  each of the five sums: k u sum |term|.
  * mse, rmse, mae (a quotient of one positive sum): k u |want|, + 2^-23 |want| for the f32 result.
  * r2 = 1 - rss / tss, explained_variance = 1 - vres / tss:  d(num) / tss + num d(tss) / tss^2 (+ 2^-23 |want|), with
    d(rss) = k u rss, and d(tss) = 2 k u sum t^2, d(vres) = 2 k u sum d^2 for the centred sums S2 - S1^2 / n (the error of S2 and as
    much again for S1^2 / n).  The bound also covers a centred sum that one side rounds to 0 under the n-ulp rule: that changes it by
    at most n 2^-52 S2.  tss == 0 (the constant-target columns): exactly 0 or 1.
  * NaN (n == 0; n < 2 for r2): the same pattern.
  * reductions over V outputs: pooled as mse with V more adds; uniform_average the mean of the per-output bounds; variance_weighted
    sum_v tss_v score_v / sum_v tss_v: [sum_v (d(tss_v) |score_v| + tss_v bound_v) + |R| sum_v d(tss_v)] / sum_v tss_v; each + (V + 2) u
    of the summed magnitudes.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tribe_ref  # noqa: E402
from tests.test_regression_metrics_host import KINDS, centred_ss, flatten_bt, raw_scores, reduced_score, regression_data, sums64  # noqa: E402

U53 = 2.0**-53
F32 = 2.0**-23
G = 4                 # metric groups: rows go to 0 .. G - 2; group G - 1 receives none (n = 0)
LAYOUTS = ["rows", "t99", "nv"]
POOLED_KINDS = ("mse", "rmse", "mae")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    return _ops


# ------------------------------------------------------------------------------------------------
# inputs and the reference
# ------------------------------------------------------------------------------------------------
def _device_view(x: torch.Tensor, layout: str) -> torch.Tensor:
    """Host [B, V, T] -> a fresh device allocation in the layout under test (no offset views)."""
    if layout == "nv":
        B, V, T = x.shape
        return tribe_ref.flatten_bt(x).contiguous().cuda().view(B, T, V).transpose(1, 2)
    return x.contiguous().cuda()


def _groups(B: int) -> torch.Tensor:
    """Runs of three rows per group cycling through 0 .. G - 2, so a group changes inside one wave's rows (b, b + 4, ...) and across
    row-chunk boundaries; ids -1, G and G + 3 (to be skipped) sprinkled in."""
    gid = (torch.arange(B) // 3) % (G - 1)
    gid[5::7] = -1
    gid[3::11] = G
    gid[10::13] = G + 3
    return gid


def _pieces(B: int):
    """The rows split over up to three update calls that accumulate into one state."""
    cuts = sorted({0, B // 3, (2 * B) // 3, B})
    return [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]


def _reference(pred: torch.Tensor, true: torch.Tensor, gid: torch.Tensor, n_groups: int):
    """float64 statistics [n_groups, V, 6] and the magnitudes [n_groups, V, 5] behind the five sums, per group of rows."""
    V = pred.shape[1]
    stats, mags = np.zeros((n_groups, V, 6)), np.zeros((n_groups, V, 5))
    for grp in range(n_groups):
        sel = gid == grp
        if sel.any():
            stats[grp], mags[grp] = sums64(flatten_bt(pred[sel]), flatten_bt(true[sel]))
    return stats, mags


@functools.lru_cache(maxsize=None)
def _case(B: int, V: int, T: int):
    """Data and reference of one shape, computed once and shared by the layouts that use it (read only)."""
    pred, true = regression_data(B, V, T, seed=B * 7919 + V + T)
    gid = _groups(B)
    return pred, true, gid, *_reference(pred, true, gid, G)


# ------------------------------------------------------------------------------------------------
# bounds (derivations in the module docstring)
# ------------------------------------------------------------------------------------------------
def _score_bound(stats: np.ndarray, kind: str) -> np.ndarray:
    """Bound of the f64 score of every output; 0 where the score is an exact 0 / 1 or NaN."""
    k = (stats[..., 5] + 2) * U53
    want = raw_scores(stats, kind)
    if kind in POOLED_KINDS:
        return np.nan_to_num(k * np.abs(want))
    rss, stt = stats[..., 1], stats[..., 4]
    tss = centred_ss(stats[..., 3], stt, stats[..., 5])
    num, dnum = (rss, k * rss) if kind == "r2" else (centred_ss(stats[..., 0], rss, stats[..., 5]), 2 * k * rss)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = dnum / tss + num * (2 * k * stt) / tss**2
    return np.where(tss > 0, b, 0.0)


def _reduced_bound(stats: np.ndarray, kind: str, mode: str) -> float:
    """stats [V, 6] of one group with n > 0."""
    V = stats.shape[0]
    raw, bound = raw_scores(stats, kind), _score_bound(stats, kind)
    if mode == "pooled":
        return float((stats[0, 5] + 2 + V + 2) * U53 * abs(reduced_score(stats, kind, mode)))
    tss = centred_ss(stats[:, 3], stats[:, 4], stats[:, 5])
    if mode == "uniform_average" or tss.sum() == 0:
        return float(bound.mean() + (V + 2) * U53 * np.abs(raw).mean())
    dtss = 2 * (stats[:, 5] + 2) * U53 * stats[:, 4]
    R = reduced_score(stats, kind, mode)
    return float(((dtss * np.abs(raw) + tss * bound).sum() + abs(R) * dtss.sum() + (V + 2) * U53 * (tss * np.abs(raw)).sum()) / tss.sum())


def _assert_close(got: np.ndarray, want: np.ndarray, bound: np.ndarray, what: str):
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs (n == 0, or n < 2 for r2, and nothing else)"
    err = np.abs(got - want)[~nan]
    excess = err - np.broadcast_to(bound, want.shape)[~nan]
    assert excess.size == 0 or excess.max() <= 0, f"{what}: off by {err.max():.3e}, {excess.max():.3e} beyond the bound"


def _check_state(ops, stats: torch.Tensor, want_stats: np.ndarray, mags: np.ndarray, what: str):
    """The device statistics against the float64 sums, then every score and reduction computed from the device statistics."""
    got_stats = stats.cpu().numpy()
    assert np.array_equal(got_stats[..., 5], want_stats[..., 5]), f"{what}: sample counts differ (a row dropped, repeated or misplaced)"
    k = (want_stats[..., 5:6] + 2) * U53
    err = np.abs(got_stats[..., :5] - want_stats[..., :5])
    assert (err <= k * mags).all(), f"{what}: sums off by up to {(err / np.maximum(mags, 1e-300)).max():.3e} relative"
    for kind in KINDS:
        want, bound = raw_scores(want_stats, kind), _score_bound(want_stats, kind)
        print(f"{what} {kind}: largest bound {bound.max():.3e}")
        raw = ops.regression_from_stats(stats, kind)
        assert raw.dtype == torch.float32 and raw.shape == stats.shape[:2]
        _assert_close(raw.cpu().numpy(), want, bound + F32 * np.nan_to_num(np.abs(want)), f"{what} {kind} raw")
        for mode in ("pooled", "uniform_average", "variance_weighted"):
            if mode == "pooled" and kind not in POOLED_KINDS:
                continue
            got = ops.regression_reduce(stats, kind, mode).cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (stats.shape[0],)
            for g in range(stats.shape[0]):
                want_g = reduced_score(want_stats[g], kind, mode)
                bound_g = 0.0 if np.isnan(want_g) else _reduced_bound(want_stats[g], kind, mode)
                _assert_close(got[g], want_g, bound_g, f"{what} {kind} {mode} group {g}")
    # the force-finite values of the constant-target columns, the perfect column and explained variance on the offset column
    r2, ev = (ops.regression_from_stats(stats, kind).cpu().numpy() for kind in ("r2", "explained_variance"))
    seen = want_stats[:, 0, 5] > 0
    assert seen.any() and not seen[G - 1:].any()
    for got, col, value in ((r2, 0, 0.0), (ev, 0, 0.0), (r2, 1, 1.0), (ev, 1, 1.0), (r2, 4, 1.0), (ev, 4, 1.0), (ev, 2, 1.0)):
        assert (got[seen, col] == value).all(), f"{what}: column {col} must give exactly {value}, got {got[seen, col]}"
    assert (r2[seen, 2] < 1.0).all()
    assert np.isnan(r2[~seen]).all() and np.isnan(ev[~seen]).all()


def _run_case(ops, B: int, V: int, T: int, layout: str):
    pred, true, gid, want_stats, mags = _case(B, V, T)
    stats = torch.zeros(G, V, 6, dtype=torch.float64, device="cuda")
    for b0, b1 in _pieces(B):
        ops.regression_stats_update(stats, _device_view(pred[b0:b1], layout), _device_view(true[b0:b1], layout), gid[b0:b1].cuda())
    _check_state(ops, stats, want_stats, mags, f"B={B} V={V} T={T} {layout}")
    return stats


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V", [33, 1000])
@pytest.mark.parametrize("B", [1, 5, 16, 67])
def test_stats_scores_and_reductions(ops, B, V, layout):
    _run_case(ops, B, V, 99 if layout == "t99" else 100, layout)


def test_rows_long(ops):
    """T > 768: the rows kernel's four-deep float4 loop (i + 192 < T / 4) runs before its remainder loop."""
    _run_case(ops, 5, 33, 1028, "rows")


def test_cancellation_column_keeps_its_mse(ops):
    """true = 1e3 + N(0, 1), pred = true + 1e-3 N(0, 1): the direct residual sum meets the bound of every other column.  A residual
    sum derived from the moments, Sxx - 2 Sxy + Syy, of the same data is several orders outside it."""
    B, V, T = 67, 33, 100
    pred, true, _, _, _ = _case(B, V, T)
    stats = torch.zeros(1, V, 6, dtype=torch.float64, device="cuda")
    ops.regression_stats_update(stats, pred.cuda(), true.cuda(), None)
    want_stats, _ = sums64(flatten_bt(pred), flatten_bt(true))
    want = raw_scores(want_stats, "mse")[3]
    got = float(ops.regression_from_stats(stats, "mse")[0, 3])
    bound = ((B * T + 2) * U53 + F32) * want
    assert abs(got - want) <= bound, f"mse of the cancellation column {got!r} vs {want!r} (bound {bound:.3e})"
    # the moment form at its best: float64 pairwise sums of the exact products (what the Pearson state holds)
    p, t = flatten_bt(pred)[:, 3], flatten_bt(true)[:, 3]
    moment = ((p * p).sum() - 2 * (p * t).sum() + (t * t).sum()) / (B * T)
    assert abs(moment - want) > 100 * bound


def test_one_sample_and_no_group(ops):
    """n == 1 (one row of T = 1): r2 NaN, explained variance 1, mse = d^2; group == None sends every row to group 0."""
    V = 33
    pred, true = regression_data(1, V, 1, seed=3)
    stats = torch.zeros(2, V, 6, dtype=torch.float64, device="cuda")
    ops.regression_stats_update(stats, pred.cuda(), true.cuda(), None)
    want_stats, _ = sums64(flatten_bt(pred), flatten_bt(true))
    assert np.array_equal(stats[0].cpu().numpy(), want_stats) and not stats[1].any()
    assert torch.isnan(ops.regression_from_stats(stats, "r2")).all()
    ev = ops.regression_from_stats(stats, "explained_variance").cpu()
    assert (ev[0] == 1.0).all() and torch.isnan(ev[1]).all()
    mse = ops.regression_from_stats(stats, "mse").cpu().numpy()
    assert np.array_equal(mse[0], raw_scores(want_stats, "mse").astype(np.float32)) and np.isnan(mse[1]).all()
    for kind in KINDS:
        for mode in ("uniform_average", "variance_weighted"):
            got = ops.regression_reduce(stats, kind, mode).cpu().numpy()
            assert np.isnan(got[1]) and (np.isnan(got[0]) if kind == "r2" else np.isfinite(got[0]))
    with pytest.raises(ValueError):
        ops.regression_reduce(stats, "r2", "pooled")
    with pytest.raises(ValueError):
        ops.regression_from_stats(stats, "spearman")


@pytest.mark.parametrize("B,T,layout", [(3, 99, "t99"), (3, 100, "nv"), (1, 100, "rows"), (1, 1028, "rows")])
def test_pearson_and_regression_states_walk_the_data_alike(ops, B, T, layout):
    """Both families run the one kernel pair of csrc/bvt_stats.h, so what they both sum comes out bit for bit equal: the counts,
    Pearson's Sy (index 1) = regression's sum t (index 3), and Pearson's Syy (index 3) = regression's sum t^2 (index 4; either
    accumulator adds the exact f64 square of the widened f32 target in one fma).  Only shapes with a fixed summation order: the strided
    kernel (one workgroup per output adds its rows in order; group 0 receives two of them), and the rows kernel with B = 1, where one
    wave adds once into a zeroed state (with B > 1 several waves add with atomics in no fixed order)."""
    V = 5
    pred, true = regression_data(B, V, T, seed=T + B)
    gid = torch.tensor([0, 1, 0])[:B].cuda()
    p, t = _device_view(pred, layout), _device_view(true, layout)
    pearson, regression = (torch.zeros(2, V, 6, dtype=torch.float64, device="cuda") for _ in range(2))
    ops.pearson_stats_update(pearson, p, t, gid)
    ops.regression_stats_update(regression, p, t, gid)
    want_n = torch.tensor([(B + 1) // 2, B // 2], dtype=torch.float64).mul(T)[:, None].expand(2, V)
    assert torch.equal(pearson[..., 5].cpu(), want_n) and torch.equal(regression[..., 5], pearson[..., 5]), "sample counts differ"
    assert torch.equal(pearson[..., 1], regression[..., 3]), "Pearson's Sy and regression's sum t differ in bits"
    assert torch.equal(pearson[..., 3], regression[..., 4]), "Pearson's Syy and regression's sum t^2 differ in bits"
    assert (pearson[0, :, 3] > 0).all()


# ------------------------------------------------------------------------------------------------
# metric classes and GroupedMetric
# ------------------------------------------------------------------------------------------------
def _want_class(stats: np.ndarray, kind: str, mode: str):
    """(want, bound) of what a class reports (f32) from the float64 statistics [V, 6] of its samples."""
    if mode == "raw_values":
        want = raw_scores(stats, kind)
        return want, _score_bound(stats, kind) + F32 * np.abs(want)
    want = reduced_score(stats, kind, mode)
    return want, _reduced_bound(stats, kind, mode) + F32 * abs(want)


CLASS_CASES = [
    ("MeanSquaredError", {}, "mse", "pooled"),
    ("MeanSquaredError", {"squared": False}, "rmse", "pooled"),
    ("MeanSquaredError", {"num_outputs": 33}, "mse", "raw_values"),
    ("MeanAbsoluteError", {}, "mae", "pooled"),
    ("MeanAbsoluteError", {"num_outputs": 33}, "mae", "raw_values"),
    ("R2Score", {}, "r2", "uniform_average"),
    ("R2Score", {"multioutput": "variance_weighted", "num_outputs": 33}, "r2", "variance_weighted"),
    ("R2Score", {"multioutput": "raw_values"}, "r2", "raw_values"),
    ("ExplainedVariance", {}, "explained_variance", "uniform_average"),
    ("ExplainedVariance", {"multioutput": "variance_weighted"}, "explained_variance", "variance_weighted"),
    ("ExplainedVariance", {"multioutput": "raw_values"}, "explained_variance", "raw_values"),
]


@pytest.mark.parametrize("name,kwargs,kind,mode", CLASS_CASES)
def test_metric_classes(name, kwargs, kind, mode):
    """[N, V] and [B, V, T'] inputs (two updates each) give the same result, the restatement's; reset() and the errors."""
    import modeling_utils.metrics as mm

    B, V, T = 5, 33, 100
    pred, true, _, _, _ = _case(B, V, T)
    want_stats, _ = sums64(flatten_bt(pred), flatten_bt(true))
    want, bound = _want_class(want_stats, kind, mode)
    for form in ("bvt", "nv"):
        metric = getattr(mm, name)(**kwargs)
        with pytest.raises(RuntimeError):
            metric.compute()
        for b0, b1 in ((0, 2), (2, B)):
            p, t = pred[b0:b1].cuda(), true[b0:b1].cuda()
            if form == "nv":
                p, t = tribe_ref.flatten_bt(p).contiguous(), tribe_ref.flatten_bt(t).contiguous()
            metric.update(p, t)
        got = metric.compute()
        assert got.dtype == torch.float32 and got.shape == ((V,) if mode == "raw_values" else ())
        _assert_close(got.cpu().numpy(), want, bound, f"{name}({kwargs}) {form}")
        metric.reset()
        with pytest.raises(RuntimeError):
            metric.compute()
        metric.update(pred[:1].cuda(), true[:1].cuda())                   # after reset: the first row alone
        first, _ = sums64(flatten_bt(pred[:1]), flatten_bt(true[:1]))
        _assert_close(metric.compute().cpu().numpy(), *_want_class(first, kind, mode), f"{name}({kwargs}) {form} after reset")


def test_one_dimensional_inputs_and_width_errors():
    import modeling_utils.metrics as mm

    pred, true, _, _, _ = _case(5, 33, 100)
    p, t = pred[:, 7].reshape(-1), true[:, 7].reshape(-1)                 # [N]: one output
    stats, _ = sums64(p.double().numpy()[:, None], t.double().numpy()[:, None])
    for name, kind, mode in (("MeanSquaredError", "mse", "pooled"), ("MeanAbsoluteError", "mae", "pooled"),
                             ("R2Score", "r2", "uniform_average"), ("ExplainedVariance", "explained_variance", "uniform_average")):
        metric = getattr(mm, name)()
        metric.update(p.cuda(), t.cuda())
        _assert_close(metric.compute().cpu().numpy(), *_want_class(stats, kind, mode), f"{name} on [N]")
    with pytest.raises(ValueError):
        mm.MeanSquaredError(num_outputs=7).update(pred.cuda(), true.cuda())   # the data has 33 outputs
    metric = mm.MeanAbsoluteError()
    metric.update(pred.cuda(), true.cuda())
    with pytest.raises(ValueError):
        metric.update(pred[:, :8].contiguous().cuda(), true[:, :8].contiguous().cuda())


def test_r2_adjusted():
    """1 - (1 - r2) (n - 1) / (n - k - 1) on the reduced score; unadjusted when k >= n - 1 (torchmetrics' documented rule, restated)."""
    import modeling_utils.metrics as mm

    pred, true, _, _, _ = _case(5, 33, 100)
    n = 5 * 100
    stats, _ = sums64(flatten_bt(pred), flatten_bt(true))
    want, bound = _want_class(stats, "r2", "uniform_average")
    for k in (3, n - 1, n + 5):
        metric = mm.R2Score(adjusted=k)
        metric.update(pred.cuda(), true.cuda())
        scale = (n - 1) / (n - k - 1) if k < n - 1 else 1.0
        want_k = 1 - (1 - want) * scale if k < n - 1 else want
        # the score's own bound scaled, plus the f32 rounding of the result and of the score it was made from
        _assert_close(metric.compute().cpu().numpy(), want_k, bound * scale + F32 * (abs(want_k) + abs(want) * scale), f"adjusted={k}")


@pytest.mark.parametrize("name,kwargs,kind,mode", [c for c in CLASS_CASES if c[3] != "raw_values" and "num_outputs" not in c[1]])
def test_grouped_metric(name, kwargs, kind, mode):
    """GroupedMetric(name): [B, V, T'] with groups [B, 1] and [N, V] with groups [N] give the same {group: value}, first-seen order."""
    from modeling_utils.metrics import GroupedMetric

    B, V, T = 16, 33, 100
    pred, true, _, _, _ = _case(B, V, T)
    subj = torch.tensor([7, 7, 2, 9, 2, 7, 9, 9, 2, 2, 7, 9, 7, 2, 9, 7])
    order = ["7", "2", "9"]
    want = {}
    for s in order:
        stats, _ = sums64(flatten_bt(pred[subj == int(s)]), flatten_bt(true[subj == int(s)]))
        want[s] = _want_class(stats, kind, mode)
    for form in ("bvt", "nv"):
        metric = GroupedMetric(name, kwargs)
        assert metric.compute() == {}
        for b0, b1 in ((0, 6), (6, B)):
            p, t, g = pred[b0:b1].cuda(), true[b0:b1].cuda(), subj[b0:b1].cuda()
            if form == "nv":
                p, t = tribe_ref.flatten_bt(p).contiguous(), tribe_ref.flatten_bt(t).contiguous()
                metric.update(p, t, groups=g.repeat_interleave(T))
            else:
                metric.update(p, t, groups=g[:, None])
        got = metric.compute()
        assert list(got) == order and all(isinstance(v, float) for v in got.values())
        for s in order:
            _assert_close(got[s], *want[s], f"GroupedMetric({name}, {kwargs}) {form} group {s}")
        metric.reset()
        metric.update(pred[:3].cuda(), true[:3].cuda(), groups=subj[:3].cuda())
        got = metric.compute()                                            # the slots survive a reset, as for Pearson
        stats, _ = sums64(flatten_bt(pred[:2]), flatten_bt(true[:2]))
        _assert_close(got["7"], *_want_class(stats, kind, mode), "after reset")
        assert np.isnan(got["9"])


def test_grouped_metric_needs_a_scalar_per_group():
    from modeling_utils.metrics import GroupedMetric

    pred, true, _, _, _ = _case(5, 33, 100)
    for name, kwargs in (("R2Score", {"multioutput": "raw_values"}), ("ExplainedVariance", {"multioutput": "raw_values"}),
                         ("MeanSquaredError", {"num_outputs": 33}), ("MeanAbsoluteError", {"num_outputs": 33})):
        metric = GroupedMetric(name, kwargs)
        metric.update(pred.cuda(), true.cuda(), groups=torch.tensor([0, 1, 0, 1, 1]).cuda())
        with pytest.raises(ValueError):
            metric.compute()


# ------------------------------------------------------------------------------------------------
# BrainModule
# ------------------------------------------------------------------------------------------------
def test_brain_module_logs_regression_metrics():
    """Two validation batches of B = 3 with mixed subjects through the small model of tests/test_gpu_model.py (hidden 768, depth 2, 4
    subjects): every metric equals the restatement applied to the host copies validation_step returns, flattened as '(b t) d'; one
    val/subj_r2/<id> per subject seen; and the Pearson metrics of a module without the regression metrics are bit-identical."""
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig
    from modeling_utils.metrics import MetricConfig
    from tests.test_gpu_model import _cuda_batch, _small_pair
    import pydantic

    fdims = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
    V, Tout, S = 50, 10, 4
    ref, m = _small_pair(fdims, V, Tout, S)
    adapter = pydantic.TypeAdapter(MetricConfig)
    pearson_cfgs = [{"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": V}},
                    {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": V}}]
    regression_cfgs = [{"log_name": "r2", "name": "R2Score"},
                       {"log_name": "mse", "name": "MeanSquaredError", "kwargs": {"num_outputs": V}},
                       {"log_name": "mae", "name": "MeanAbsoluteError"},
                       {"log_name": "ev", "name": "ExplainedVariance", "kwargs": {"multioutput": "variance_weighted"}},
                       {"log_name": "subj_r2", "name": "GroupedMetric", "metric_name": "R2Score"}]

    def build(cfgs):
        return {f"val/{c['log_name']}": adapter.validate_python(c).build() for c in cfgs}

    subjects = [torch.tensor([[2], [0], [2]]), torch.tensor([[3], [2], [0]])]      # subject 1 is never seen
    batches = []
    for i, subj in enumerate(subjects):
        data = tribe_ref.synthetic_batch(3, 31, fdims, S, seed=40 + i)
        data["subject_id"] = subj
        with torch.no_grad():
            yr = ref(data)
        data["fmri"] = 0.3 * yr + torch.randn(yr.shape, generator=torch.Generator().manual_seed(50 + i))
        batches.append(data)

    def run(metrics):
        bm = BrainModule(m, TorchLossConfig(name="MSELoss").build(), None, metrics)
        outs = [bm.validation_step(_cuda_batch(data), i) for i, data in enumerate(batches)]
        bm.on_validation_epoch_end()
        return bm, outs

    metrics = build(pearson_cfgs + regression_cfgs)
    bm, outs = run(metrics)
    preds, trues = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    assert not preds.is_cuda and preds.shape == (6, V, Tout)
    stats, _ = sums64(flatten_bt(preds), flatten_bt(trues))
    for key, kind, mode in (("val/r2", "r2", "uniform_average"), ("val/mse", "mse", "raw_values"), ("val/mae", "mae", "pooled"),
                            ("val/ev", "explained_variance", "variance_weighted")):
        assert bm.logged[key] is metrics[key]
        _assert_close(metrics[key].compute().cpu().numpy(), *_want_class(stats, kind, mode), key)
    all_subj = torch.cat(subjects).flatten()
    seen = ["2", "0", "3"]                                                      # first-seen order
    assert [k for k in bm.logged if k.startswith("val/subj_r2/")] == [f"val/subj_r2/{s}" for s in seen]
    for s in seen:
        sel = all_subj == int(s)
        st, _ = sums64(flatten_bt(preds[sel]), flatten_bt(trues[sel]))
        _assert_close(bm.logged[f"val/subj_r2/{s}"], *_want_class(st, "r2", "uniform_average"), f"val/subj_r2/{s}")
    # the same batches through a module that holds the Pearson metrics alone
    only = build(pearson_cfgs)
    bm2, outs2 = run(only)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(outs, outs2))
    assert torch.equal(only["val/pearson"].compute(), metrics["val/pearson"].compute())
    assert torch.equal(only["val/pearson"].per_output(), metrics["val/pearson"].per_output())
    pearson_keys = [k for k in bm.logged if k.startswith("val/subj_pearson/")]
    assert len(pearson_keys) == 3 and all(bm2.logged[k] == bm.logged[k] for k in pearson_keys)
