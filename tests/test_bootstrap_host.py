"""CPU (no GPU): the host side of BootstrapPearsonCorrCoef -- the config registry, constructor and argument checks, the C ABI's
argument checks (which return before any launch), `paired_difference`'s refusals and `sync()` over a 2-rank gloo group on block
statistics filled by hand -- plus the numpy restatement of what csrc/bootstrap.hip computes: a vectorised Philox4x32-10 pinned to
known answers, the draw and its counts, the resampled r from block statistics pinned against scipy.stats.pearsonr on the
concatenated resampled rows, and the per-column summary.  tests/test_gpu_bootstrap.py imports the restatement."""

import ctypes as C
import os
import socket
import warnings

import numpy as np
import pydantic
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter: np.ndarray, key: np.ndarray) -> np.ndarray:
    """uint32 [..., 4] counters and uint32 [..., 2] keys (broadcast against each other) -> uint32 [..., 4]."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def draws(seed: int, n_boot: int, n_sel: int) -> np.ndarray:
    """int64 [n_boot, n_sel]: draw k of replicate r = (u * n_sel) >> 32, u = word k & 3 of Philox(counter (k >> 2, r, 0, 0), key
    (seed & 0xffffffff, seed >> 32))."""
    quads = (n_sel + 3) // 4
    counter = np.zeros((n_boot, quads, 4), dtype=np.uint32)
    counter[..., 0] = np.arange(quads, dtype=np.uint32)[None, :]
    counter[..., 1] = np.arange(n_boot, dtype=np.uint32)[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    u = philox4x32_10(counter, key).reshape(n_boot, quads * 4)[:, :n_sel].astype(np.uint64)
    return ((u * np.uint64(n_sel)) >> np.uint64(32)).astype(np.int64)


def counts_of(seed: int, n_boot: int, n_sel: int) -> np.ndarray:
    """int32 [n_boot, n_sel]"""
    d = draws(seed, n_boot, n_sel)
    return np.stack([np.bincount(row, minlength=n_sel) for row in d]).astype(np.int32)


def block_stats(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """f64 [blocks, V, 6] = {Sx, Sy, Sxx, Syy, Sxy, n} of predictions x / targets y [blocks, V, T]."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    n = np.full(x.shape[:2], float(x.shape[2]))
    return np.stack([x.sum(-1), y.sum(-1), (x * x).sum(-1), (y * y).sum(-1), (x * y).sum(-1), n], -1)


def r64_from_stats(s: np.ndarray) -> np.ndarray:
    """f64 [...]: the one-pass rule of pearson_from_stats_kernel on [..., 6] sums; NaN for n < 2 or a constant column."""
    sx, sy, sxx, syy, sxy, n = (s[..., k] for k in range(6))
    eps = np.finfo(np.float64).eps
    with np.errstate(invalid="ignore", divide="ignore"):
        vx, vy = sxx - sx * sx / n, syy - sy * sy / n
        vx, vy = np.where(vx > n * eps * sxx, vx, 0.0), np.where(vy > n * eps * syy, vy, 0.0)
        r = np.clip((sxy - sx * sy / n) / np.sqrt(vx * vy), -1.0, 1.0)
    r[~(n >= 2) | (vx == 0) | (vy == 0)] = np.nan
    return r


def r_from_stats(s: np.ndarray) -> np.ndarray:
    return r64_from_stats(s).astype(np.float32)


def resampled_stats(stats: np.ndarray, blocks: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """f64 [n_boot + 1, V, 6]: count-weighted sums of the selected blocks' statistics; the last row takes every count as 1."""
    sel = stats[blocks]                                                     # [n_sel, V, 6]
    w = np.concatenate([counts.astype(np.float64), np.ones((1, len(blocks)))], 0)
    return np.einsum("rj,jvq->rvq", w, sel)


def mean_over_parcels(r: np.ndarray) -> np.ndarray:
    """f32 [rows]: the f64 mean of the f32 values of every row, rounded once; NaN when one value is NaN."""
    return r.astype(np.float64).mean(-1).astype(np.float32)


def resample(stats: np.ndarray, blocks: np.ndarray, counts: np.ndarray):
    """(observed f32 [V], replicates f32 [n_boot, V], mean_observed f32, mean_replicates f32 [n_boot])"""
    r = r_from_stats(resampled_stats(stats, blocks, counts))
    m = mean_over_parcels(r)
    return r[-1], r[:-1], m[-1], m[:-1]


def summary(table: np.ndarray, quantiles) -> dict:
    """Per column of f32 [n, C]: quantiles (numpy "linear" over the non-NaN values, f64), std (ddof = 1), the counts and p-values."""
    t = table.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = np.nanquantile(t, list(quantiles), axis=0, method="linear")
        sd = np.nanstd(t, axis=0, ddof=1)
    valid = ~np.isnan(t)
    m = valid.sum(0)
    n_le, n_ge = (valid & (t <= 0)).sum(0), (valid & (t >= 0)).sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_le = np.where(m > 0, (1.0 + n_le) / (m + 1.0), np.nan)
        p_ge = np.where(m > 0, (1.0 + n_ge) / (m + 1.0), np.nan)
        p_two = np.where(m > 0, np.minimum(1.0, 2.0 * np.minimum(p_le, p_ge)), np.nan)
    return {"q": q, "std": sd, "n_le": n_le, "n_ge": n_ge, "n_valid": m, "p_le": p_le.astype(np.float32),
            "p_ge": p_ge.astype(np.float32), "p_two": p_two.astype(np.float32)}


def signal_data(blocks: int, V: int, T: int, seed: int, noise: float = 1.0):
    """(predictions, targets) f32 [blocks, V, T]: targets N(0, 1) noise + 0.3 signal, predictions `noise` N(0, 1) + 0.3 signal: every
    column's |mean| stays well below its standard deviation."""
    rng = np.random.default_rng(seed)
    sig = rng.standard_normal((blocks, V, T))
    y = rng.standard_normal((blocks, V, T)) + 0.3 * sig
    x = noise * rng.standard_normal((blocks, V, T)) + 0.3 * sig
    return x.astype(np.float32), y.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the generator and the draw
# ------------------------------------------------------------------------------------------------
def _words(text: str) -> np.ndarray:
    return np.array([int(w, 16) for w in text.split()], dtype=np.uint32)


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert (philox4x32_10(_words(counter), _words(key)) == _words(want)).all()


def _philox_scalar(c, k):
    """the generator written out word by word with Python integers"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + _W0) & 0xFFFFFFFF, (k[1] + _W1) & 0xFFFFFFFF]
    return c


def test_draws_follow_the_definition():
    seed, n_boot, n_sel = (7 << 32) + 11, 5, 13
    d = draws(seed, n_boot, n_sel)
    for r in range(n_boot):
        for k in range(n_sel):
            u = _philox_scalar((k >> 2, r, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[k & 3]
            assert d[r, k] == (u * n_sel) >> 32


@pytest.mark.parametrize("n_sel", [1, 2, 3, 4, 5, 63, 64, 65, 1000])
def test_draws_and_counts(n_sel):
    for seed in (0, 5, (1 << 32) + 5):
        d = draws(seed, 7, n_sel)
        assert d.shape == (7, n_sel) and (d >= 0).all() and (d < n_sel).all()
        c = counts_of(seed, 7, n_sel)
        assert c.dtype == np.int32 and (c.sum(1) == n_sel).all()
    if n_sel > 4:
        assert (draws(5, 7, n_sel) != draws((1 << 32) + 5, 7, n_sel)).any()   # the high word of the seed is part of the key
        assert (draws(5, 7, n_sel)[0] != draws(5, 7, n_sel)[1]).any()         # and the replicate part of the counter


def test_restatement_equals_scipy_on_resampled_rows():
    """The statistics route (count-weighted block sums, one-pass rule) against scipy.stats.pearsonr on the concatenation of the drawn
    blocks' samples: <= 1e-12 (measured 1.1e-16 when written)."""
    from scipy import stats as sps

    nb, V, T, n_boot = 37, 5, 12, 64
    x, y = signal_data(nb, V, T, seed=3)
    st = block_stats(x, y)
    d = draws(9, n_boot, nb)
    got = r64_from_stats(resampled_stats(st, np.arange(nb), counts_of(9, n_boot, nb)))
    worst = 0.0
    for r in range(n_boot + 1):
        rows = d[r] if r < n_boot else np.arange(nb)
        xs = x[rows].transpose(1, 0, 2).reshape(V, -1).astype(np.float64)
        ys = y[rows].transpose(1, 0, 2).reshape(V, -1).astype(np.float64)
        for v in range(V):
            worst = max(worst, abs(got[r, v] - sps.pearsonr(xs[v], ys[v]).statistic))
    print(f"worst |statistics route - scipy| = {worst:.3e}")
    assert worst <= 1e-12


def test_degenerate_blocks_in_the_restatement():
    """Two one-sample blocks: NaN exactly where both draws coincide (28 of 64 replicates at seed 5), r = +-1 elsewhere."""
    x = np.array([[[1.0]], [[2.0]]], dtype=np.float32)
    y = np.array([[[3.0]], [[1.0]]], dtype=np.float32)
    d = draws(5, 64, 2)
    _, rep, _, _ = resample(block_stats(x, y), np.arange(2), counts_of(5, 64, 2))
    same = d[:, 0] == d[:, 1]
    assert same.sum() == 28
    assert (np.isnan(rep[:, 0]) == same).all() and (rep[~same, 0] == -1.0).all()


def test_summary_restatement_counts_and_p_values():
    t = np.array([[0.0, np.nan, 1.0], [-0.0, np.nan, 2.0], [-1.0, np.nan, np.nan], [3.0, np.nan, -1.0]], dtype=np.float32)
    s = summary(t, (0.0, 0.5, 1.0))
    assert s["n_valid"].tolist() == [4, 0, 3] and s["n_le"].tolist() == [3, 0, 1] and s["n_ge"].tolist() == [3, 0, 2]
    assert s["q"][:, 0].tolist() == [-1.0, 0.0, 3.0] and np.isnan(s["q"][:, 1]).all() and s["q"][:, 2].tolist() == [-1.0, 1.0, 2.0]
    assert s["p_le"][0] == np.float32(4 / 5) and np.isnan(s["p_le"][1]) and s["p_two"][2] == np.float32(1.0)


# ------------------------------------------------------------------------------------------------
# registry and constructors
# ------------------------------------------------------------------------------------------------
def test_config_validates_and_builds():
    from modeling_utils.metrics import BootstrapPearsonCorrCoef, BootstrapPearsonCorrCoefConfig, GroupedMetric, MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    cfg = adapter.validate_python({"log_name": "boot", "name": "BootstrapPearsonCorrCoef",
                                   "kwargs": {"num_outputs": 1000, "num_bootstraps": 200, "quantiles": [0.05, 0.5, 0.95], "seed": 3}})
    assert isinstance(cfg, BootstrapPearsonCorrCoefConfig) and cfg.log_name == "boot"
    metric = cfg.build()
    assert type(metric) is BootstrapPearsonCorrCoef
    assert (metric.num_outputs, metric.num_bootstraps, metric.quantiles, metric.seed) == (1000, 200, (0.05, 0.5, 0.95), 3)
    default = adapter.validate_python({"log_name": "b", "name": "BootstrapPearsonCorrCoef"}).build()
    assert (default.num_outputs, default.num_bootstraps, default.quantiles, default.seed) == (1, 1000, (0.025, 0.975), 0)
    grouped = adapter.validate_python({"log_name": "subj_boot", "name": "GroupedMetric", "metric_name": "BootstrapPearsonCorrCoef",
                                       "kwargs": {"num_bootstraps": 100}}).build()
    assert isinstance(grouped, GroupedMetric) and grouped.base_metric_cls is BootstrapPearsonCorrCoef
    assert grouped.compute() == {} and grouped.intervals() == {}
    assert repr(grouped) == "GroupedMetric(BootstrapPearsonCorrCoef)"
    with pytest.raises(TypeError):
        GroupedMetric("MultidimPearsonCorrCoef").intervals()


def test_bad_kwargs_and_constructor_errors():
    from modeling_utils.metrics import BootstrapPearsonCorrCoef, GroupedMetric, MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    for bad in ({"log_name": "m", "name": "BootstrapPearsonCorrCoef", "kwargs": {"n_boot": 10}},
                {"log_name": "m", "name": "BootstrapPearsonCorrCoef", "kwargs": {"num_outputs": 3, "alpha": 0.05}},
                {"log_name": "m", "name": "BootstrapPearsonCorrCoef", "num_outputs": 3},
                {"log_name": "m", "name": "BootstrapPearson"}):
        with pytest.raises(pydantic.ValidationError):
            adapter.validate_python(bad)
    for kwargs in ({"num_outputs": 0}, {"num_outputs": -3}, {"num_outputs": 2.5}, {"num_outputs": "7"}, {"num_outputs": True},
                   {"num_bootstraps": 0}, {"num_bootstraps": 10.0}, {"num_bootstraps": None}, {"num_bootstraps": 16385},
                   {"quantiles": ()}, {"quantiles": (0.5, 1.5)}, {"quantiles": (-0.1,)}, {"quantiles": (float("nan"),)}, {"quantiles": 0.5},
                   {"seed": -1}, {"seed": 1 << 64}, {"seed": 1.0}):
        with pytest.raises(ValueError):
            BootstrapPearsonCorrCoef(**kwargs)
    BootstrapPearsonCorrCoef(num_bootstraps=16384, seed=(1 << 64) - 1, quantiles=(0.0, 1.0))
    metric = BootstrapPearsonCorrCoef(3)
    for call in (metric.compute, metric.per_output, metric.intervals):
        with pytest.raises(RuntimeError, match=r"compute\(\) called before update\(\)"):
            call()
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8, 4), torch.zeros(8, 4))            # width != num_outputs (checked before the device)
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8), torch.zeros(8))
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8, 3), torch.zeros(9, 3))
    # the block limit: one block per batch row, and GroupedMetric's 2-D path makes every row a batch row
    with pytest.raises(ValueError, match=r"\[B, V, T'\]"):
        metric.update_bvt(torch.zeros(32769, 3, 1), torch.zeros(32769, 3, 1))
    with pytest.raises(ValueError, match=r"\[B, V, T'\]"):
        GroupedMetric("BootstrapPearsonCorrCoef").update(torch.zeros(32769, 2), torch.zeros(32769, 2), groups=torch.zeros(32769, dtype=torch.int64))


def test_reference_default_metric_list_with_bootstrap_validates():
    from modeling_utils.metrics import MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    # grids/defaults.py:107-124 of the reference, as data, plus the new entries next to it
    for raw in ({"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "retrieval_top1", "name": "TopkAcc", "topk": 1},
                {"log_name": "pearson_ci", "name": "BootstrapPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "subj_pearson_ci", "name": "GroupedMetric", "metric_name": "BootstrapPearsonCorrCoef",
                 "kwargs": {"num_outputs": 1000}}):
        cfg = adapter.validate_python(raw)
        assert cfg.log_name == raw["log_name"] and cfg.name == raw["name"]
        cfg.build()


def test_cpu_tensors_are_refused():
    from modeling_utils.metrics import BootstrapPearsonCorrCoef
    from tribe_hip import ops
    from tribe_hip._lib import TribeHipError

    with pytest.raises(TribeHipError):
        ops.bootstrap_counts(0, 4, 4, "cpu")
    with pytest.raises(TribeHipError):
        ops.bootstrap_pearson(torch.zeros(2, 3, 6, dtype=torch.float64), torch.arange(2), None)
    with pytest.raises(TribeHipError):
        ops.bootstrap_summary(torch.zeros(4, 3), (0.5,))
    with pytest.raises(TribeHipError):
        BootstrapPearsonCorrCoef(3).update(torch.zeros(8, 3), torch.zeros(8, 3))
    for kwargs in ({"seed": -1}, {"seed": 1 << 64}, {"n_boot": 0}, {"n_boot": 16385}, {"n_sel": 0}, {"n_sel": 32769}):
        with pytest.raises(ValueError):
            ops.bootstrap_counts(**{"seed": 0, "n_boot": 4, "n_sel": 4, "device": "cuda", **kwargs})


def test_abi_argument_checks():
    """The C entry points refuse bad arguments before any launch (no GPU needed): rc < 0 -> ValueError with the library's message."""
    from tribe_hip._lib import check, lib

    L = lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def counts(seed=0, n_boot=4, n_sel=4, out=p):
        check(L.tribe_bootstrap_counts(seed, n_boot, n_sel, out, None), "tribe_bootstrap_counts")

    for kwargs, message in (({"out": None}, "null pointer"), ({"n_boot": 0}, "n_boot"), ({"n_boot": 16385}, "n_boot"), ({"n_sel": 0}, "n_sel"),
                            ({"n_sel": 32769}, "n_sel")):
        with pytest.raises(ValueError, match=message):
            counts(**kwargs)

    def pearson(stats=p, n_blocks=2, V=3, blocks=p, n_sel=2, cnt=p, n_boot=4, r=p, ld=4, mean=p, mean_stride=4):
        check(L.tribe_bootstrap_pearson(stats, n_blocks, V, blocks, n_sel, cnt, n_boot, r, ld, mean, mean_stride, None), "tribe_bootstrap_pearson")

    for kwargs, message in (({"stats": None}, "null pointer"), ({"blocks": None}, "null pointer"), ({"r": None}, "null pointer"),
                            ({"mean": None}, "null pointer"), ({"cnt": None}, "null counts"), ({"n_boot": -1}, "n_boot"),
                            ({"n_boot": 16385}, "n_boot"), ({"n_blocks": 0}, "bad shape"), ({"V": 0}, "bad shape"), ({"ld": 2}, "bad shape"),
                            ({"mean_stride": 0}, "bad shape"), ({"n_sel": 0}, "n_sel"), ({"n_sel": 32769}, "n_sel")):
        with pytest.raises(ValueError, match=message):
            pearson(**kwargs)

    def summarise(rep=p, n=4, Cn=3, ld=3, q=p, n_q=2, qv=p, sd=p, n_le=p, n_ge=p, n_valid=p):
        check(L.tribe_bootstrap_summary(rep, n, Cn, ld, q, n_q, qv, sd, n_le, n_ge, n_valid, None), "tribe_bootstrap_summary")

    for kwargs, message in (({"rep": None}, "null pointer"), ({"q": None}, "null pointer"), ({"sd": None}, "null pointer"),
                            ({"n_valid": None}, "null pointer"), ({"n": 0}, "replicates"), ({"n": 16385}, "replicates"),
                            ({"Cn": 0}, "bad shape"), ({"ld": 2}, "bad shape"), ({"n_q": 0}, "quantiles"), ({"n_q": 1025}, "quantiles")):
        with pytest.raises(ValueError, match=message):
            summarise(**kwargs)


# ------------------------------------------------------------------------------------------------
# paired_difference: refusals (decided on the host, before any launch)
# ------------------------------------------------------------------------------------------------
def _hand_filled(n: int, V: int = 2, groups=None, **kwargs):
    from modeling_utils.metrics import BootstrapPearsonCorrCoef

    metric = BootstrapPearsonCorrCoef(V, **kwargs)
    metric._stats = torch.zeros(max(n, 1), V, 6, dtype=torch.float64)
    metric._groups = torch.zeros(max(n, 1), dtype=torch.int64) if groups is None else torch.tensor(groups, dtype=torch.int64)
    metric._n, metric.n_groups = n, 1
    return metric


def test_paired_difference_refuses_mismatches():
    a = _hand_filled(4, seed=1)
    with pytest.raises(ValueError, match="seed"):
        a.paired_difference(_hand_filled(4, seed=2))
    with pytest.raises(ValueError, match="num_bootstraps"):
        a.paired_difference(_hand_filled(4, seed=1, num_bootstraps=10))
    with pytest.raises(ValueError, match="num_outputs"):
        a.paired_difference(_hand_filled(4, V=3, seed=1))
    with pytest.raises(ValueError, match="block counts"):
        a.paired_difference(_hand_filled(5, seed=1))
    with pytest.raises(ValueError, match="groups"):
        _hand_filled(4, seed=1, groups=[0, 0, 1, 1]).paired_difference(_hand_filled(4, seed=1, groups=[0, 1, 0, 1]))
    with pytest.raises(TypeError):
        a.paired_difference(object())


# ------------------------------------------------------------------------------------------------
# sync(): 2 ranks, gloo, CPU state filled by hand
# ------------------------------------------------------------------------------------------------
V_SYNC = 3
SYNC_BLOCKS = {0: [0, 1, 0, 0, 1], 1: [0, 0]}     # rank -> group of every block: uneven lengths, and rank 1 has not seen group 1


def _sync_stats(rank: int, n: int) -> torch.Tensor:
    base = torch.arange(n * V_SYNC * 6, dtype=torch.float64).reshape(n, V_SYNC, 6)
    return base + 1000.0 * rank + 0.5


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sync_worker(rank: int, world: int, port: int, q):
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "algonauts-2025_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from modeling_utils.metrics import BootstrapPearsonCorrCoef

        groups = SYNC_BLOCKS[rank]
        n, cap = len(groups), 8                                        # more capacity than blocks: sync must send the filled part only
        metric = BootstrapPearsonCorrCoef(V_SYNC)
        metric._stats = torch.full((cap, V_SYNC, 6), float("nan"), dtype=torch.float64)
        metric._stats[:n] = _sync_stats(rank, n)
        metric._groups = torch.full((cap,), 7, dtype=torch.int64)
        metric._groups[:n] = torch.tensor(groups)
        metric._n, metric.n_groups = n, max(groups) + 1
        metric.sync()
        q.put((rank, metric._n, metric.n_groups, metric._stats.numpy(), metric._groups.numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sync_concatenates_blocks_in_rank_order():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == [0, 1]
    want_stats = torch.cat([_sync_stats(r, len(SYNC_BLOCKS[r])) for r in range(world)]).numpy()
    want_groups = np.array(SYNC_BLOCKS[0] + SYNC_BLOCKS[1])
    for _, n, n_groups, stats, groups in results:                      # every rank ends with the same, whole state
        assert n == 7 and n_groups == 2
        assert stats.shape == (7, V_SYNC, 6) and (stats == want_stats).all() and (groups == want_groups).all()


def test_sync_without_process_group_is_a_no_op():
    from modeling_utils.metrics import BootstrapPearsonCorrCoef

    metric = BootstrapPearsonCorrCoef(2)
    metric.sync()
    assert metric._stats is None and metric._n == 0
