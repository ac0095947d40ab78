"""CPU (no GPU): the host side of MultidimSpearmanCorrCoef -- the config registry, constructor and argument checks, the C ABI's
argument checks (which return before any launch) and `sync()` over a 2-rank gloo group on sample buffers filled by hand -- plus the
formula pin: a numpy restatement of what csrc/rank_corr.hip computes (doubled centred ranks as integers, int64 sums, rho from
them in f64, rounded once to f32) against scipy.stats.rankdata and scipy.stats.spearmanr.  tests/test_gpu_rank_corr.py imports the
restatement and the data families below."""

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

FAMILIES = ("normal", "levels2", "levels8", "equal", "zeros_infs", "sorted", "reversed")


# ------------------------------------------------------------------------------------------------
# data and the restatement
# ------------------------------------------------------------------------------------------------
def family(kind: str, n: int, V: int, seed: int) -> np.ndarray:
    """f32 [n, V]: N(0, 1); quantised to 2 / 8 levels (massive ties); one value everywhere; +0.0 / -0.0 / +inf / -inf / a few
    finite values mixed; every column ascending; every column descending."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, V)).astype(np.float32)
    if kind == "normal":
        return x
    if kind == "levels2":
        return (x > 0).astype(np.float32)
    if kind == "levels8":
        return np.floor(np.clip((x + 2) * 2, 0, 7)).astype(np.float32)
    if kind == "equal":
        return np.full((n, V), 1.25, dtype=np.float32)
    if kind == "zeros_infs":
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 1e-45, -1e-45], dtype=np.float32)
        return pool[rng.integers(0, len(pool), size=(n, V))]
    if kind == "sorted":
        return np.sort(x, axis=0)
    if kind == "reversed":
        return np.sort(x, axis=0)[::-1].copy()
    raise ValueError(kind)


def centred_ranks(x: np.ndarray) -> np.ndarray:
    """int64 [n, V]: a_i = #{x_j < x_i} + #{x_j <= x_i} - n per column, by sorting (IEEE order: -0.0 == +0.0)."""
    x = np.asarray(x, dtype=np.float32) + np.float32(0.0)
    n = x.shape[0]
    s = np.sort(x, axis=0)
    out = np.empty(x.shape, dtype=np.int64)
    for v in range(x.shape[1]):
        out[:, v] = np.searchsorted(s[:, v], x[:, v], "left") + np.searchsorted(s[:, v], x[:, v], "right") - n
    return out


def rank_sums(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """int64 [V, 3] = {sum a b, sum a^2, sum b^2}; 0 in a column with a NaN (the kernel's convention)."""
    bad = np.isnan(x).any(0) | np.isnan(y).any(0)
    a, b = centred_ranks(np.nan_to_num(x)), centred_ranks(np.nan_to_num(y))
    sums = np.stack([(a * b).sum(0), (a * a).sum(0), (b * b).sum(0)], -1)
    sums[bad] = 0
    return sums


def rho_from_sums(sums: np.ndarray, n: int, bad: np.ndarray) -> np.ndarray:
    """f32 [V]: sab / sqrt(saa sbb) in f64, clamped, rounded once; NaN for n < 2, a constant column or a flagged (NaN) column."""
    sab, saa, sbb = (sums[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.clip(sab / np.sqrt(saa * sbb), -1.0, 1.0)
    rho[(saa == 0) | (sbb == 0) | bad | (n < 2)] = np.nan
    return rho.astype(np.float32)


def scipy_rho(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """f64 [V]: scipy.stats.spearmanr per column (NaN for a constant column, a NaN sample or n < 2)."""
    from scipy import stats

    out = np.full(x.shape[1], np.nan)
    if x.shape[0] < 2:
        return out
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for v in range(x.shape[1]):
            out[v] = stats.spearmanr(x[:, v].astype(np.float64), y[:, v].astype(np.float64)).statistic
    return out


# ------------------------------------------------------------------------------------------------
# formula pin against scipy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 65, 1000])
def test_restatement_equals_scipy(n):
    """(a + n + 1) / 2 equals rankdata(method="average") exactly for every family, and the f32 rho from the integer sums is within
    2^-24 of spearmanr: the sums are exact, the f64 evaluation errs at the 1e-16 level and the one rounding of a value in [-1, 1] to
    f32 by at most 2^-25."""
    from scipy import stats

    V = 4
    for kind in FAMILIES:
        x, y = family(kind, n, V, seed=n), family("normal", n, V, seed=n + 1) + 0.5 * family("levels8", n, V, seed=n)
        a = centred_ranks(x)
        assert ((a + n + 1) * 0.5 == stats.rankdata(x.astype(np.float64), "average", axis=0)).all(), kind
        got = rho_from_sums(rank_sums(x, y), n, np.zeros(V, bool))
        want = scipy_rho(x, y)
        assert (np.isnan(got) == np.isnan(want)).all(), kind
        ok = ~np.isnan(want)
        assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= 2.0**-24).all(), kind


# ------------------------------------------------------------------------------------------------
# registry and constructors
# ------------------------------------------------------------------------------------------------
def test_config_validates_and_builds():
    from modeling_utils.metrics import GroupedMetric, MetricConfig, MultidimSpearmanCorrCoef, MultidimSpearmanCorrCoefConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    cfg = adapter.validate_python({"log_name": "spearman", "name": "MultidimSpearmanCorrCoef", "kwargs": {"num_outputs": 1000}})
    assert isinstance(cfg, MultidimSpearmanCorrCoefConfig) and cfg.log_name == "spearman"
    metric = cfg.build()
    assert type(metric) is MultidimSpearmanCorrCoef and metric.num_outputs == 1000
    assert adapter.validate_python({"log_name": "s", "name": "MultidimSpearmanCorrCoef"}).build().num_outputs == 1
    grouped = adapter.validate_python({"log_name": "subj_spearman", "name": "GroupedMetric", "metric_name": "MultidimSpearmanCorrCoef",
                                       "kwargs": {"num_outputs": 1000}}).build()
    assert isinstance(grouped, GroupedMetric) and grouped.base_metric_cls is MultidimSpearmanCorrCoef and grouped.compute() == {}
    assert repr(grouped) == "GroupedMetric(MultidimSpearmanCorrCoef)"


def test_bad_kwargs_and_constructor_errors():
    from modeling_utils.metrics import GroupedMetric, MetricConfig, MultidimSpearmanCorrCoef

    adapter = pydantic.TypeAdapter(MetricConfig)
    for bad in ({"log_name": "m", "name": "MultidimSpearmanCorrCoef", "kwargs": {"eps": 1e-6}},
                {"log_name": "m", "name": "MultidimSpearmanCorrCoef", "kwargs": {"num_outputs": 3, "dim": 0}},
                {"log_name": "m", "name": "MultidimSpearmanCorrCoef", "num_outputs": 3},
                {"log_name": "m", "name": "SpearmanCorrCoef"},
                {"log_name": "m", "name": "SpearmanCorrCoef", "kwargs": {"num_outputs": 3}}):
        with pytest.raises(pydantic.ValidationError):
            adapter.validate_python(bad)
    for num_outputs in (0, -3, 2.5, "7", None, True):
        with pytest.raises(ValueError):
            MultidimSpearmanCorrCoef(num_outputs=num_outputs)
    with pytest.raises(RuntimeError, match=r"compute\(\) called before update\(\)"):
        MultidimSpearmanCorrCoef(3).compute()
    with pytest.raises(RuntimeError, match=r"compute\(\) called before update\(\)"):
        MultidimSpearmanCorrCoef(3).per_output()
    with pytest.raises(AssertionError):
        GroupedMetric("SpearmanCorrCoef")
    metric = MultidimSpearmanCorrCoef(3)
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8, 4), torch.zeros(8, 4))            # width != num_outputs (checked before the device)
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8), torch.zeros(8))
    with pytest.raises(ValueError):
        metric.update(torch.zeros(8, 3), torch.zeros(9, 3))
    with pytest.raises(ValueError, match="2\\^20"):
        metric.update(torch.zeros((1 << 20) + 1, 3), torch.zeros((1 << 20) + 1, 3))   # one group's samples: at most 2^20


def test_reference_default_metric_list_with_spearman_validates():
    from modeling_utils.metrics import MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    # grids/defaults.py:107-124 of the reference, as data, plus the new entries next to it
    for raw in ({"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "retrieval_top1", "name": "TopkAcc", "topk": 1},
                {"log_name": "spearman", "name": "MultidimSpearmanCorrCoef", "kwargs": {"num_outputs": 1000}},
                {"log_name": "subj_spearman", "name": "GroupedMetric", "metric_name": "MultidimSpearmanCorrCoef",
                 "kwargs": {"num_outputs": 1000}}):
        cfg = adapter.validate_python(raw)
        assert cfg.log_name == raw["log_name"] and cfg.name == raw["name"]
        cfg.build()


def test_cpu_tensors_are_refused():
    from modeling_utils.metrics import GroupedMetric, MultidimSpearmanCorrCoef
    from tribe_hip import ops
    from tribe_hip._lib import TribeHipError

    x = torch.zeros(8, 3)
    with pytest.raises(TribeHipError):
        ops.rank_columns(x)
    with pytest.raises(TribeHipError):
        ops.spearman_columns(x, x)
    with pytest.raises(TribeHipError):
        ops.spearman_from_state(torch.zeros(3, 8), torch.zeros(3, 8), 8)
    with pytest.raises(TribeHipError):
        ops.rank_append(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 3, 8), torch.zeros(1, 3, 8))
    with pytest.raises(TribeHipError):
        MultidimSpearmanCorrCoef(3).update(x, x)
    with pytest.raises(TribeHipError):
        GroupedMetric("MultidimSpearmanCorrCoef", {"num_outputs": 3}).update(x, x, groups=torch.zeros(8, dtype=torch.int64))


def test_abi_argument_checks():
    """The C entry points refuse bad arguments before any launch (no GPU needed): rc < 0 -> ValueError with the library's message."""
    from tribe_hip._lib import check, lib

    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    C_default, n_max = L.tribe_spearman_default_chunk(), L.tribe_spearman_max_samples()
    assert C_default == 16384 and n_max == 1 << 20 and 2 * 4 * C_default <= 160 * 1024

    def columns(pred=p, truth=p, ld=8, n=8, V=1, chunk=0, rho=p, sums=p, ws=None, ws_bytes=0):
        check(L.tribe_spearman_columns(pred, truth, ld, n, V, chunk, rho, sums, None, None, ws, ws_bytes, None), "tribe_spearman_columns")

    for kwargs, message in (({"pred": None}, "null pointer"), ({"truth": None}, "null pointer"), ({"rho": None}, "null pointer"),
                            ({"sums": None}, "null pointer"), ({"n": 0}, "bad shape"), ({"V": 0}, "bad shape"), ({"ld": 7}, "bad shape"),
                            ({"n": n_max + 1, "ld": n_max + 1}, "2\\^20"), ({"chunk": 100}, "power of two"), ({"chunk": 32}, "power of two"),
                            ({"chunk": 2 * C_default}, "power of two"),
                            ({"n": 1000, "ld": 1000, "chunk": 256}, "workspace too small"),
                            ({"n": 1000, "ld": 1000, "chunk": 256, "ws": p, "ws_bytes": 255}, "workspace too small"),
                            ({"n": C_default + 1, "ld": C_default + 1}, "workspace too small")):
        with pytest.raises(ValueError, match=message):
            columns(**kwargs)
    # the workspace: none on the one-workgroup route; on the merge route it stops growing with V (columns go in rounds)
    ws = L.tribe_spearman_workspace_bytes
    assert ws(256, 1000, 256) == 0 and ws(C_default, 1000, 0) == 0 and ws(0, 5, 0) == 0
    assert ws(257, 1, 256) >= 4 * 257 * 4 and ws(257, 2, 256) > ws(257, 1, 256)
    assert ws(102400, 1000, 0) == ws(102400, 5000, 0) <= 128 << 20

    def append(pred=p, truth=p, B=1, V=2, T=4, group=None, G=1, cap=8, counts=p, pos=p, ps=p, ts=p):
        check(L.tribe_rank_append(pred, truth, B, V, T, V * T, T, 1, group, G, cap, counts, pos, ps, ts, None), "tribe_rank_append")

    for kwargs, message in (({"pred": None}, "null pointer"), ({"counts": None}, "null pointer"), ({"pos": None}, "null pointer"),
                            ({"ts": None}, "null pointer"), ({"B": 0}, "bad shape"), ({"G": 0}, "bad shape"), ({"cap": 3}, "capacity"),
                            ({"T": 64 * 40000, "cap": 64 * 40000}, "too large")):
        with pytest.raises(ValueError, match=message):
            append(**kwargs)


# ------------------------------------------------------------------------------------------------
# sync(): 2 ranks, gloo, CPU state buffers filled by hand
# ------------------------------------------------------------------------------------------------
V_SYNC = 3
SYNC_COUNTS = {0: [5, 2], 1: [3]}     # rank -> samples per group: uneven lengths, and rank 1 has not seen group 1


def _sync_samples(rank: int, g: int, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    base = torch.arange(n, dtype=torch.float32)[None, :] + 10.0 * torch.arange(V_SYNC, dtype=torch.float32)[:, None]
    return base + 100.0 * g + 1000.0 * rank, -(base + 100.0 * g + 1000.0 * rank)


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
        from modeling_utils.metrics import MultidimSpearmanCorrCoef

        counts = SYNC_COUNTS[rank]
        metric = MultidimSpearmanCorrCoef(V_SYNC)
        cap = 8                                                        # more capacity than samples: sync must send the filled part only
        metric._pred = torch.full((len(counts), V_SYNC, cap), float("nan"))
        metric._true = torch.full((len(counts), V_SYNC, cap), float("nan"))
        for g, n in enumerate(counts):
            metric._pred[g, :, :n], metric._true[g, :, :n] = _sync_samples(rank, g, n)
        metric._counts = torch.tensor(counts, dtype=torch.int64)
        metric._total = max(counts)
        metric.sync()
        q.put((rank, metric._counts.tolist(), metric._total, metric._pred.numpy(), metric._true.numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sync_concatenates_per_group():
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
    want_counts = [5 + 3, 2 + 0]
    for _, counts, total, pred, true in results:                       # every rank ends with the same, whole state
        assert counts == want_counts and total == max(want_counts)
        assert pred.shape == true.shape == (2, V_SYNC, max(want_counts))
        for g, n in enumerate(want_counts):
            parts = [_sync_samples(r, g, SYNC_COUNTS[r][g]) for r in range(world) if g < len(SYNC_COUNTS[r])]
            want_p, want_t = (torch.cat([part[k] for part in parts], dim=1).numpy() for k in range(2))
            assert (pred[g, :, :n] == want_p).all() and (true[g, :, :n] == want_t).all()


def test_sync_without_process_group_is_a_no_op():
    from modeling_utils.metrics import MultidimSpearmanCorrCoef

    metric = MultidimSpearmanCorrCoef(2)
    metric.sync()
    assert metric._pred is None and metric._total == 0
