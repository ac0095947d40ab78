"""CPU (no GPU): the retrieval metrics' host side -- config registry, the two-rank `sync()` of the rank buffers (gloo), and the
g14 fixture the GPU tests read."""

import os
import socket

import numpy as np
import pydantic
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

# grids/defaults.py:107-124 of the reference, as data
REFERENCE_DEFAULT_METRICS = [
    {"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
    {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": 1000}},
    {"log_name": "retrieval_top1", "name": "TopkAcc", "topk": 1},
]


def test_reference_default_metrics_validate_and_build():
    from modeling_utils.metrics import MetricConfig
    from modeling_utils.metrics.metrics import TopkAcc

    adapter = pydantic.TypeAdapter(MetricConfig)
    built = {}
    for raw in REFERENCE_DEFAULT_METRICS:
        cfg = adapter.validate_python(raw)
        assert cfg.log_name == raw["log_name"] and cfg.name == raw["name"]
        built[cfg.log_name] = cfg.build()
    top1 = built["retrieval_top1"]
    assert isinstance(top1, TopkAcc) and top1.topk == 1 and top1.relative is False


def test_rank_and_online_pearson_configs():
    from modeling_utils.metrics import MetricConfig, OnlinePearsonCorr, Rank

    adapter = pydantic.TypeAdapter(MetricConfig)
    rank = adapter.validate_python({"log_name": "rank", "name": "Rank", "reduction": "mean", "relative": True}).build()
    assert type(rank) is Rank and rank.reduction == "mean" and rank.relative is True
    default = adapter.validate_python({"log_name": "rank", "name": "Rank"}).build()
    assert default.reduction == "median" and default.relative is False
    opc = adapter.validate_python({"log_name": "r", "name": "OnlinePearsonCorr", "dim": 1, "reduction": "sum"}).build()
    assert isinstance(opc, OnlinePearsonCorr) and opc.dim == 1 and opc.reduction == "sum"
    assert adapter.validate_python({"log_name": "t", "name": "TopkAcc"}).build().topk == 5
    for bad in ({"log_name": "rank", "name": "Rank", "topk": 1},
                {"log_name": "t", "name": "TopkAcc", "topk": 1, "relative": True},
                {"log_name": "r", "name": "OnlinePearsonCorr", "dim": 0, "kwargs": {}},
                {"log_name": "rank", "name": "Rank", "reduction": "max"}):
        with pytest.raises(pydantic.ValidationError):
            adapter.validate_python(bad)


def test_labels_are_resolved_like_the_reference():
    from modeling_utils.metrics.metrics import Rank

    idx = Rank._true_indices(3, 5, ["b", "a", "b"], ["a", "b", "c", "b", "a"], torch.device("cpu"))
    assert idx.tolist() == [1, 0, 1]   # first occurrence
    assert Rank._true_indices(4, 4, None, None, torch.device("cpu")) is None
    with pytest.raises(ValueError):
        Rank._true_indices(1, 2, ["z"], ["a", "b"], torch.device("cpu"))
    with pytest.raises(ValueError):
        Rank._true_indices(3, 4, None, None, torch.device("cpu"))
    with pytest.raises(ValueError):
        Rank._true_indices(2, 2, ["a", "b"], None, torch.device("cpu"))


def test_compute_before_update_is_nan_and_reset_keeps_nothing():
    from modeling_utils.metrics.metrics import Rank, TopkAcc

    for m in (Rank(), TopkAcc(1)):
        assert torch.isnan(m.compute())
        m._buf, m._count = torch.arange(8, dtype=torch.float32), 8
        m.reset()
        assert m.ranks.numel() == 0 and torch.isnan(m.compute())


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
        from modeling_utils.metrics.metrics import TopkAcc

        lens = [3, 5]
        m = TopkAcc(topk=2)
        local = torch.arange(lens[rank], dtype=torch.float32) + 10.0 * rank + 0.5
        buf = torch.full((16,), -7.0)   # a grown state buffer: capacity beyond the count
        buf[: lens[rank]] = local
        m._buf, m._count = buf, lens[rank]
        m.sync()
        want = torch.cat([torch.arange(n, dtype=torch.float32) + 10.0 * r + 0.5 for r, n in enumerate(lens)])
        q.put((rank, m._count, m.ranks.tolist(), want.tolist()))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sync_concatenates_uneven_buffers_in_rank_order():
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
    for _, count, got, want in results:
        assert count == 8 and got == want


def test_g14_fixture_is_well_formed(golden_dir):
    path = golden_dir / "g14_retrieval.npz"
    assert path.exists() and path.stat().st_size < 200 * 1024
    g = np.load(path)
    cases = [str(c) for c in g["cases"]]
    assert {"bvt", "plain", "labelled", "ties", "nanrow", "zeronorm", "relative", "seq"} <= set(cases)
    for c in cases:
        n_up = int(g[f"{c}__n_updates"])
        rel = bool(g[f"{c}__relative"])
        n = sum(g[f"{c}__x{i}"].shape[0] for i in range(n_up))
        ranks = g[f"{c}__ranks"]
        assert ranks.dtype == np.float32 and ranks.shape == (n,)
        assert np.all(ranks >= 0) and (rel or np.all(ranks * 2 == np.round(ranks * 2)))
        assert g[f"{c}__compute"].shape == ((3,) if rel else (5,))
        for i in range(n_up):
            x, y = g[f"{c}__x{i}"], g[f"{c}__y{i}"]
            assert x.dtype == np.float32 and x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1]
            if f"{c}__xl{i}" in g:
                assert set(g[f"{c}__xl{i}"].tolist()) <= set(g[f"{c}__yl{i}"].tolist())
            else:
                assert x.shape[0] == y.shape[0]
    assert np.any(g["ties__ranks"] % 1 == 0.5)   # exact ties give half-integer ranks
    assert int(g["seq__n_updates"]) == 3 and [g[f"seq__x{i}"].shape[0] for i in range(3)] == [16, 7, 16]
    assert g["bvt__pred"].shape == (16, 64, 8) and np.allclose(g["bvt__x0"], g["bvt__pred"].mean(-1), atol=1e-6)
    for kind in ("None", "x", "y", "xy"):
        assert g[f"sim__{kind}"].shape == (g["sim__xin"].shape[0], g["sim__yin"].shape[0])
