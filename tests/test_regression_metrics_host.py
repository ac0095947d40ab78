"""CPU (no GPU): the regression metrics' host side -- the config registry and constructor checks -- and the formula pin: a float64
numpy restatement of the scores csrc/regression_metrics.hip computes from its statistics, against scikit-learn's r2_score,
explained_variance_score, mean_squared_error and mean_absolute_error.  tests/test_gpu_regression_metrics.py imports the
restatement and the data below, so the kernels are checked against formulas that scikit-learn itself pins here."""

import warnings

import numpy as np
import pydantic
import pytest
import torch

EPS64 = 2.0**-52      # f64 machine epsilon (DBL_EPSILON)
KINDS = ("mse", "rmse", "mae", "r2", "explained_variance")
MODES = ("uniform_average", "variance_weighted")
N_EDGE = 5            # edge columns of regression_data


# ------------------------------------------------------------------------------------------------
# data and the float64 restatement
# ------------------------------------------------------------------------------------------------
def regression_data(B: int, V: int, T: int, seed: int):
    """pred / true [B, V, T] f32.  Edge columns: v0 constant target -3.3 with an imperfect prediction, v1 constant target 1.7 with a
    perfect prediction, v2 pred = true + 0.7 (explained variance 1, R2 < 1), v3 true = 1e3 + N(0, 1) with pred = true + 1e-3 N(0, 1)
    (the column on which a residual sum derived from moments cancels), v4 pred == true; the others true = 0.5 pred + noise, the
    prediction scale varying across voxels."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, V, T, generator=g) * torch.logspace(-1, 1, V)[None, :, None]
    true = 0.5 * pred + torch.randn(B, V, T, generator=g)
    true[:, 0] = -3.3
    true[:, 1] = 1.7
    pred[:, 1] = 1.7
    pred[:, 2] = true[:, 2] + 0.7
    true[:, 3] = 1e3 + torch.randn(B, T, generator=g)
    pred[:, 3] = true[:, 3] + 1e-3 * torch.randn(B, T, generator=g)
    pred[:, 4] = true[:, 4]
    return pred, true


def flatten_bt(x: torch.Tensor) -> np.ndarray:
    """[B, V, T] -> the '(b t) v' matrix, float64."""
    return x.permute(0, 2, 1).reshape(-1, x.shape[1]).double().numpy()


def sums64(pred: np.ndarray, true: np.ndarray):
    """float64 [N, V] -> (stats [V, 6] = {sum d, sum d^2, sum |d|, sum t, sum t^2, n}, mags [V, 5]: the sums of the magnitudes behind
    the five sums), d = true - pred."""
    n, V = pred.shape
    d = true - pred
    stats = np.stack([d.sum(0), (d * d).sum(0), np.abs(d).sum(0), true.sum(0), (true * true).sum(0), np.full(V, float(n))], -1)
    mags = np.stack([np.abs(d).sum(0), (d * d).sum(0), np.abs(d).sum(0), np.abs(true).sum(0), (true * true).sum(0)], -1)
    return stats, mags


def centred_ss(s1, s2, n):
    """S2 - S1^2 / n, 0 when within n ulps of S2 (onepass_centred_ss of csrc/common.h)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        v = s2 - s1 * s1 / n
        return np.where(v > n * EPS64 * s2, v, 0.0)


def raw_scores(stats: np.ndarray, kind: str) -> np.ndarray:
    """stats [..., 6] float64 -> the score of every output, scikit-learn's force_finite conventions."""
    sd, rss, sad, st, stt, n = (stats[..., k] for k in range(6))
    tss, vres = centred_ss(st, stt, n), centred_ss(sd, rss, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "mse":
            out = rss / n
        elif kind == "rmse":
            out = np.sqrt(rss / n)
        elif kind == "mae":
            out = sad / n
        elif kind == "r2":
            out = np.where(tss == 0, np.where(rss == 0, 1.0, 0.0), 1.0 - rss / tss)
            out = np.where(n < 2, np.nan, out)
        elif kind == "explained_variance":
            out = np.where(tss == 0, np.where(vres == 0, 1.0, 0.0), 1.0 - vres / tss)
        else:
            raise ValueError(kind)
    return np.where(n > 0, out, np.nan)


def reduced_score(stats: np.ndarray, kind: str, mode: str):
    """stats [V, 6] -> one float: 'pooled' (mse / rmse / mae), 'uniform_average' or 'variance_weighted' (weights tss)."""
    if mode == "pooled":
        num = stats[:, 2].sum() if kind == "mae" else stats[:, 1].sum()
        n = stats[:, 5].sum()
        out = num / n if n > 0 else np.nan
        return np.sqrt(out) if kind == "rmse" else out
    raw = raw_scores(stats, kind)
    w = centred_ss(stats[:, 3], stats[:, 4], stats[:, 5])
    if mode == "variance_weighted" and w.sum() != 0:
        return (w * raw).sum() / w.sum()
    return raw.mean()


# ------------------------------------------------------------------------------------------------
# formula pin against scikit-learn
# ------------------------------------------------------------------------------------------------
def _sklearn(t, p, kind, multioutput):
    from sklearn import metrics as skm

    if kind == "rmse":                                             # the root of every column's mse
        return np.sqrt(skm.mean_squared_error(t, p, multioutput="raw_values"))
    if kind == "mse":
        return skm.mean_squared_error(t, p, multioutput=multioutput)
    if kind == "mae":
        return skm.mean_absolute_error(t, p, multioutput=multioutput)
    fn = skm.r2_score if kind == "r2" else skm.explained_variance_score
    return fn(t, p, multioutput=multioutput, force_finite=True)


@pytest.mark.parametrize("B,V,T", [(3, 12, 100), (67, 33, 100), (3, 4000, 100)])
def test_restatement_equals_sklearn(B, V, T):
    """n = 300 and n = 6700 samples, all three multioutput modes ('variance_weighted' where scikit-learn has it: R2 and explained
    variance), 1e-12 absolute.

    'variance_weighted' is held to 1e-12 at V = 4000 and to a derived bound at V = 12 and 33.  The one-pass tss_v = sum t^2 -
    (sum t)^2 / n cannot resolve less than an ulp of sum t^2: on the 1e3-offset column (sum t^2 = 1e6 n) that is ~1e-10 of tss_v, a few
    times more after the roundings of the sum and of (sum t)^2 / n.  The raw score multiplies it by rss / tss ~ 1e-6 and stays far
    inside 1e-12, but as a WEIGHT it moves sum_v tss_v score_v / sum_v tss_v by dtss_v |1 - R| / sum_v tss_v: below 1e-12 only when
    sum_v tss_v >~ 2000 n, i.e. from about a thousand outputs of this data on (mean variance 3.7).  With few outputs the deviation from
    scikit-learn's two-pass weights is ~1e-10; its bound is sum_v dtss_v (|score_v| + |R|) / sum_v tss_v with dtss_v =
    2 (n + 2) 2^-53 sum t^2 (the n adds behind each of the two sums, as in the kernel tests)."""
    from sklearn import metrics as skm

    pred, true = regression_data(B, V, T, seed=B * 31 + V)
    p, t = flatten_bt(pred), flatten_bt(true)
    stats, _ = sums64(p, t)
    n = p.shape[0]
    exact = {"r2": [0, 1, 4], "explained_variance": [0, 1]}       # force-finite 0 / 1 and the perfect column: exactly equal
    for kind in KINDS:
        want = _sklearn(t, p, kind, "raw_values")
        got = raw_scores(stats, kind)
        assert np.abs(got - want).max() <= 1e-12, f"{kind} raw: {np.abs(got - want).max():.3e}"
        for v in exact.get(kind, []):
            assert got[v] == want[v], f"{kind} column {v}: {got[v]!r} vs {want[v]!r}"
        want_u = want.mean() if kind == "rmse" else _sklearn(t, p, kind, "uniform_average")
        assert abs(reduced_score(stats, kind, "uniform_average") - want_u) <= 1e-12, f"{kind} uniform_average"
        if kind in ("r2", "explained_variance"):
            want_w = _sklearn(t, p, kind, "variance_weighted")
            err = abs(reduced_score(stats, kind, "variance_weighted") - want_w)
            tss = centred_ss(stats[:, 3], stats[:, 4], stats[:, 5])
            dtss = 2 * (n + 2) * 2.0**-53 * stats[:, 4]
            bound = 1e-12 + (0.0 if V >= 1000 else (dtss * (np.abs(want) + abs(want_w))).sum() / tss.sum())
            assert err <= bound, f"{kind} variance_weighted: {err:.3e} (bound {bound:.3e})"
    assert raw_scores(stats, "r2")[0] == 0.0 and raw_scores(stats, "explained_variance")[0] == 0.0
    assert raw_scores(stats, "r2")[1] == 1.0 and raw_scores(stats, "explained_variance")[1] == 1.0
    assert raw_scores(stats, "explained_variance")[2] == 1.0 and raw_scores(stats, "r2")[2] < 1.0
    # pooled = every element flattened (torchmetrics' num_outputs = 1)
    assert abs(reduced_score(stats, "mse", "pooled") - skm.mean_squared_error(t.ravel(), p.ravel())) <= 1e-12
    assert abs(reduced_score(stats, "rmse", "pooled") - np.sqrt(skm.mean_squared_error(t.ravel(), p.ravel()))) <= 1e-12
    assert abs(reduced_score(stats, "mae", "pooled") - skm.mean_absolute_error(t.ravel(), p.ravel())) <= 1e-12


def test_restatement_edge_values_equal_sklearn():
    """All-constant targets: 'variance_weighted' falls back to the uniform average (0.0 for imperfect predictions); one sample: R2 is
    NaN, explained variance 1; no sample: NaN."""
    from sklearn import metrics as skm

    t = np.tile(np.array([1.5, -2.0, 0.25]), (40, 1))
    p = t + np.random.default_rng(0).normal(size=t.shape)
    stats, _ = sums64(p, t)
    for kind, fn in (("r2", skm.r2_score), ("explained_variance", skm.explained_variance_score)):
        for mode in MODES:
            assert reduced_score(stats, kind, mode) == fn(t, p, multioutput=mode) == 0.0
    p[:, 1] = t[:, 1]
    stats, _ = sums64(p, t)
    assert reduced_score(stats, "r2", "variance_weighted") == skm.r2_score(t, p, multioutput="variance_weighted") == 1.0 / 3.0
    one_t, one_p = np.array([[2.0, 3.0]]), np.array([[2.5, 3.0]])
    stats, _ = sums64(one_p, one_t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_r2 = skm.r2_score(one_t, one_p, multioutput="raw_values")
    assert np.isnan(want_r2).all() and np.isnan(raw_scores(stats, "r2")).all()
    assert (raw_scores(stats, "explained_variance") == skm.explained_variance_score(one_t, one_p, multioutput="raw_values")).all()
    assert (raw_scores(stats, "explained_variance") == 1.0).all()
    for kind in KINDS:
        assert np.isnan(raw_scores(np.zeros((2, 6)), kind)).all()
        for mode in MODES:
            assert np.isnan(reduced_score(np.zeros((2, 6)), kind, mode))
    assert np.isnan(reduced_score(np.zeros((2, 6)), "mse", "pooled"))


# ------------------------------------------------------------------------------------------------
# registry and constructors
# ------------------------------------------------------------------------------------------------
def test_configs_validate_and_build():
    from modeling_utils.metrics import (ExplainedVariance, GroupedMetric, MeanAbsoluteError, MeanSquaredError, MetricConfig, R2Score,
                                        TorchMetricConfig)

    adapter = pydantic.TypeAdapter(MetricConfig)
    classes = {"MeanSquaredError": MeanSquaredError, "MeanAbsoluteError": MeanAbsoluteError, "R2Score": R2Score,
               "ExplainedVariance": ExplainedVariance}
    for name, cls in classes.items():
        cfg = adapter.validate_python({"log_name": "m", "name": name})
        assert isinstance(cfg, TorchMetricConfig) and cfg.kwargs == {} and type(cfg.build()) is cls
        grouped = adapter.validate_python({"log_name": "g", "name": "GroupedMetric", "metric_name": name}).build()
        assert isinstance(grouped, GroupedMetric) and grouped.base_metric_cls is cls and grouped.compute() == {}
    mse = adapter.validate_python({"log_name": "rmse", "name": "MeanSquaredError", "kwargs": {"squared": False, "num_outputs": 7}}).build()
    assert mse.squared is False and mse.num_outputs == 7 and mse.kind == "rmse" and MeanSquaredError().kind == "mse"
    assert adapter.validate_python({"log_name": "mae", "name": "MeanAbsoluteError", "kwargs": {"num_outputs": 3}}).build().num_outputs == 3
    r2 = adapter.validate_python({"log_name": "r2", "name": "R2Score",
                                  "kwargs": {"adjusted": 2, "multioutput": "variance_weighted", "num_outputs": 1000}}).build()
    assert r2.adjusted == 2 and r2.multioutput == "variance_weighted"
    assert R2Score().adjusted == 0 and R2Score().multioutput == "uniform_average"
    ev = adapter.validate_python({"log_name": "ev", "name": "ExplainedVariance", "kwargs": {"multioutput": "raw_values"}}).build()
    assert ev.multioutput == "raw_values"
    g = adapter.validate_python({"log_name": "g", "name": "GroupedMetric", "metric_name": "R2Score", "kwargs": {"adjusted": 1}}).build()
    assert g._state.adjusted == 1


def test_bad_kwargs_and_constructor_errors():
    from modeling_utils.metrics import ExplainedVariance, GroupedMetric, MeanAbsoluteError, MeanSquaredError, MetricConfig, R2Score

    adapter = pydantic.TypeAdapter(MetricConfig)
    for bad in ({"log_name": "m", "name": "MeanSquaredError", "kwargs": {"multioutput": "raw_values"}},
                {"log_name": "m", "name": "MeanAbsoluteError", "kwargs": {"squared": False}},
                {"log_name": "m", "name": "R2Score", "kwargs": {"adjust": 1}},
                {"log_name": "m", "name": "ExplainedVariance", "kwargs": {"num_outputs": 4}},
                {"log_name": "m", "name": "ExplainedVariance", "multioutput": "raw_values"},
                {"log_name": "m", "name": "SpearmanCorrCoef"}):
        with pytest.raises(pydantic.ValidationError):
            adapter.validate_python(bad)
    for make in (lambda: R2Score(adjusted=-1), lambda: R2Score(adjusted=1.5), lambda: R2Score(multioutput="mean"),
                 lambda: ExplainedVariance(multioutput="none"), lambda: MeanSquaredError(num_outputs=0),
                 lambda: MeanAbsoluteError(num_outputs=-2)):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(AssertionError):
        GroupedMetric("SpearmanCorrCoef")
    with pytest.raises(RuntimeError):
        R2Score().compute()


def test_reference_default_metric_list_still_validates():
    from modeling_utils.metrics import MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    # grids/defaults.py:107-124 of the reference, as data, plus what a user adds next to it
    for raw in ({"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "retrieval_top1", "name": "TopkAcc", "topk": 1},
                {"log_name": "r2", "name": "R2Score"},
                {"log_name": "subj_mse", "name": "GroupedMetric", "metric_name": "MeanSquaredError"}):
        cfg = adapter.validate_python(raw)
        assert cfg.log_name == raw["log_name"] and cfg.name == raw["name"]
        cfg.build()


def test_cpu_tensors_are_refused():
    from modeling_utils.metrics import MeanSquaredError
    from tribe_hip import ops
    from tribe_hip._lib import TribeHipError

    with pytest.raises(TribeHipError):
        MeanSquaredError().update(torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(TribeHipError):
        ops.regression_from_stats(torch.zeros(1, 3, 6, dtype=torch.float64), "mse")
    with pytest.raises(TribeHipError):
        ops.regression_reduce(torch.zeros(1, 3, 6, dtype=torch.float64), "mse", "pooled")


@pytest.mark.parametrize("entry", ["tribe_pearson_stats_update", "tribe_regression_stats_update"])
def test_stats_update_abi_argument_checks(entry):
    """Both [G, V, 6] update entry points share one argument check (csrc/bvt_stats.h) and refuse bad arguments before any launch (no GPU
    needed): rc < 0 -> ValueError with the library's message under the entry point's own name."""
    import ctypes as C

    from tribe_hip._lib import check, lib

    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def update(pred=p, truth=p, B=1, V=2, T=4, G=1, stats=p):
        check(getattr(lib(), entry)(pred, truth, B, V, T, V * T, T, 1, None, G, stats, None), entry)

    for kwargs, message in (({"pred": None}, "null pointer"), ({"truth": None}, "null pointer"), ({"stats": None}, "null pointer"),
                            ({"B": 0}, "bad shape"), ({"V": 0}, "bad shape"), ({"T": 0}, "bad shape"), ({"G": 0}, "bad shape"),
                            ({"V": 2**31}, "exceeds the grid")):
        with pytest.raises(ValueError, match=f"{entry}: .*{message}"):
            update(**kwargs)


def test_pearson_loss_abi_refuses_a_width_beyond_the_grid():
    """tribe_pearson_loss_fwd launches the same kernel pair, one workgroup column per output: V = 2^31 is refused.  The workspace size
    is given as the number the entry point asks for (the pointer is never read), so it is the grid check that fires."""
    import ctypes as C

    from tribe_hip._lib import check, lib

    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    V = 2**31
    with pytest.raises(ValueError, match="tribe_pearson_loss_fwd: .*exceeds the grid"):
        check(lib().tribe_pearson_loss_fwd(p, p, 1, V, 4, V * 4, 4, 1, 0, p, p, lib().tribe_pearson_loss_workspace_bytes(V), None),
              "tribe_pearson_loss_fwd")
