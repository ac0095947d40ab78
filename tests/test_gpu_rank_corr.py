"""GPU: the sort-and-rank kernels of csrc/rank_corr.hip, MultidimSpearmanCorrCoef on top of them and its use in GroupedMetric and
BrainModule, against scipy.stats (rankdata, spearmanr) and the integer restatement of tests/test_rank_corr_host.py (which scipy pins
there).

Bounds (none tuned):
  * average ranks: `==` scipy.stats.rankdata(method="average").
  * sums {sum a b, sum a^2, sum b^2} of the doubled centred ranks: `==` the numpy int64 sums (integers below 2^60).
  * rho: |rho - spearmanr| <= 2^-24: the sums are exact, the f64 quotient errs at the 1e-16 level, the one rounding of a value in
    [-1, 1] to f32 by at most 2^-25.  The one-workgroup route and the merge route give the same bits.  NaN exactly where scipy's is.
  * MultidimSpearmanCorrCoef.compute() (f64 mean of the f32 rho, rounded once): 2^-23 against the f64 mean of scipy's rho
    (2^-24 per term carried through the mean, 2^-25 for the rounding).
  * GroupedMetric takes the f32 mean of V values in torch (metrics/base.py): 2^-25 from each rho, and with u = 2^-24 the V - 1 adds
    and the division add at most u * sum of the partial sums' magnitudes.  The grouped test uses V = 3 weakly correlated outputs
    (|rho| < 0.25), for which that is 2^-25 + (0.5 + 0.75 + 0.25) u < 2^-23, the bound the test then asserts.
"""

import functools

import numpy as np
import pydantic
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tribe_ref  # noqa: E402
from tests.test_rank_corr_host import FAMILIES, family, rank_sums, rho_from_sums, scipy_rho  # noqa: E402

RHO_TOL = 2.0**-24
MEAN_TOL = 2.0**-23


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    return _ops


# ------------------------------------------------------------------------------------------------
# data and references (computed once per shape)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(kind: str, n: int, V: int):
    """x of the family under test, y a continuous signal correlated with it (finite even where x is infinite)."""
    x = family(kind, n, V, seed=7 * n + V)
    y = (0.5 * np.nan_to_num(x, posinf=3.0, neginf=-3.0) + family("normal", n, V, seed=7 * n + V + 1)).astype(np.float32)
    return x, y                                                       # shared between cases: nobody writes to them


@functools.lru_cache(maxsize=None)
def _reference(kind: str, n: int, V: int):
    from scipy import stats

    x, y = _pair(kind, n, V)
    ranks = stats.rankdata(x.astype(np.float64), "average", axis=0).reshape(n, V)
    sums = rank_sums(x, y)
    return ranks, sums, scipy_rho(x, y)


def _check_case(ops, kind: str, n: int, V: int, chunk: int):
    """ranks ==, sums ==, rho within 2^-24 and NaN where scipy's is; returns rho's bits for the route comparison."""
    x, y = _pair(kind, n, V)
    ranks, sums, want = _reference(kind, n, V)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    got_ranks = ops.rank_columns(xd, chunk=chunk)
    assert got_ranks.shape == (n, V) and got_ranks.dtype == torch.float32
    assert (got_ranks.cpu().numpy().astype(np.float64) == ranks).all(), f"{kind} n={n} V={V} chunk={chunk}: ranks"
    rho, got_sums = ops.spearman_columns(xd, yd, chunk=chunk)
    assert got_sums.dtype == torch.int64 and (got_sums.cpu().numpy() == sums).all(), f"{kind} n={n} V={V} chunk={chunk}: sums"
    rho = rho.cpu().numpy()
    assert (np.isnan(rho) == np.isnan(want)).all(), f"{kind} n={n} V={V} chunk={chunk}: NaN pattern {rho} vs {want}"
    ok = ~np.isnan(want)
    err = np.abs(rho[ok].astype(np.float64) - want[ok]).max() if ok.any() else 0.0
    assert err <= RHO_TOL, f"{kind} n={n} V={V} chunk={chunk}: rho off by {err:.3e}"
    assert (rho.view(np.uint32) == rho_from_sums(sums, n, np.zeros(V, bool)).view(np.uint32))[ok].all()
    return rho.view(np.uint32)


# ------------------------------------------------------------------------------------------------
# 1. ranks, exact; 3. score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_ranks_sums_and_rho_default_route(ops, n):
    for V in (1, 3, 65):
        for kind in FAMILIES:
            _check_case(ops, kind, n, V, 0)


# ------------------------------------------------------------------------------------------------
# 2. both routes and the boundary
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 511, 513, 1000, 1029])
def test_forced_chunk_256_routes_agree(ops, n):
    """chunk = 256: n <= 256 stays in one workgroup, above it chunks are sorted and merged over one (257 .. 512), two (513 .. 1024)
    and three (1029) levels with ragged last chunks; V = 65 takes two rounds of columns.  Same bits as the default route."""
    for V in (3, 65):
        for kind in FAMILIES:
            assert (_check_case(ops, kind, n, V, 256) == _check_case(ops, kind, n, V, 0)).all(), f"{kind} n={n} V={V}"
    assert (_check_case(ops, "normal", n, 3, 64) == _check_case(ops, "normal", n, 3, 0)).all()


@pytest.mark.parametrize("offset", ["C-1", "C", "C+1", "2C+37"])
def test_default_chunk_boundary(ops, offset):
    C = ops.spearman_default_chunk()
    n = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+37": 2 * C + 37}[offset]
    other = C // 2 if n <= C else 256            # the other route where there is one, else another depth of the merge route
    for kind in FAMILIES:
        assert (_check_case(ops, kind, n, 3, 0) == _check_case(ops, kind, n, 3, other)).all(), f"{kind} n={n}"


@pytest.mark.parametrize("n,chunk", [(600, 0), (600, 256), (1, 0), (2, 0)])
def test_nan_exactly_where_scipy_gives_nan(ops, n, chunk):
    """Column 1 constant predictions, 3 constant targets, 2 a NaN among the predictions, 4 among the targets; 0 and 5 ordinary:
    they are unaffected (same bits as the call without the NaN columns)."""
    V = 6
    x, y = (a.copy() for a in _pair("normal", n, V))
    x[:, 1], y[:, 3] = 0.75, -2.0
    clean = ops.spearman_columns(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), chunk=chunk)[0].cpu().numpy()
    x[n // 2, 2], y[n - 1, 4] = np.nan, np.nan
    want = scipy_rho(x, y)
    rho, sums = ops.spearman_columns(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), chunk=chunk)
    rho = rho.cpu().numpy()
    assert (np.isnan(want) == ([True] * V if n < 2 else [False, True, True, True, True, False])).all()
    assert (np.isnan(rho) == np.isnan(want)).all(), (rho, want)
    ok = ~np.isnan(want)
    assert (np.abs(rho[ok].astype(np.float64) - want[ok]) <= RHO_TOL).all()
    assert (rho.view(np.uint32)[[0, 5]] == clean.view(np.uint32)[[0, 5]]).all()
    assert (sums.cpu().numpy() == rank_sums(x, y)).all()
    ranks = ops.rank_columns(torch.from_numpy(x).cuda(), chunk=chunk).cpu().numpy()
    assert np.isnan(ranks[:, 2]).all() and not np.isnan(np.delete(ranks, 2, axis=1)).any()


# ------------------------------------------------------------------------------------------------
# the append op
# ------------------------------------------------------------------------------------------------
def test_append_places_every_row_behind_its_group(ops):
    """2500 batch rows (three tiles of the position kernel) of T = 2 samples over G = 3 groups, ids -1 and G among them (dropped),
    appended in two calls onto counts that start uneven; then [1, V, N] (the view of an [N, V] matrix) and a T-contiguous batch."""
    B, V, T, G, cap = 2500, 3, 2, 3, 6000
    gen = torch.Generator().manual_seed(3)
    pred, true = torch.randn(B, V, T, generator=gen), torch.randn(B, V, T, generator=gen)
    group = torch.randint(-1, G + 1, (B,), generator=gen)
    ps, ts = torch.full((G, V, cap), -7.0).cuda(), torch.full((G, V, cap), -7.0).cuda()
    counts = torch.zeros(G, dtype=torch.int64).cuda()
    want_p, want_t = [[] for _ in range(G)], [[] for _ in range(G)]
    for lo, hi in ((0, 1100), (1100, B)):
        ops.rank_append(ps, ts, counts, pred[lo:hi].cuda(), true[lo:hi].cuda(), group[lo:hi].cuda())
        for b in range(lo, hi):
            if 0 <= group[b] < G:
                want_p[group[b]].append(pred[b])
                want_t[group[b]].append(true[b])
    assert counts.tolist() == [T * len(rows) for rows in want_p] and min(counts.tolist()) > 0
    for g in range(G):
        n = T * len(want_p[g])
        assert torch.equal(ps[g, :, :n].cpu(), torch.cat(want_p[g], dim=1)) and torch.equal(ts[g, :, :n].cpu(), torch.cat(want_t[g], dim=1))
        assert bool((ps[g, :, n:] == -7.0).all()) and bool((ts[g, :, n:] == -7.0).all())
    # a row that would pass the capacity is dropped, nothing is written past the run
    small_p, small_t = torch.full((1, V, 5), -7.0).cuda(), torch.full((1, V, 5), -7.0).cuda()
    c1 = torch.zeros(1, dtype=torch.int64).cuda()
    ops.rank_append(small_p, small_t, c1, pred[:3].cuda(), true[:3].cuda())
    assert c1.tolist() == [4] and torch.equal(small_p[0, :, :4].cpu(), torch.cat([pred[0], pred[1]], dim=1))
    assert bool((small_p[0, :, 4] == -7.0).all())
    # layouts: the [1, V, N] view of a matrix (v-contiguous reads) and odd sizes over several tiles
    N, V2 = 333, 70
    m = torch.randn(N, V2, generator=gen)
    sp, st = torch.zeros(1, V2, N).cuda(), torch.zeros(1, V2, N).cuda()
    ops.rank_append(sp, st, torch.zeros(1, dtype=torch.int64).cuda(), m.cuda().t().unsqueeze(0), (-m).cuda().t().unsqueeze(0))
    assert torch.equal(sp[0].cpu(), m.t()) and torch.equal(st[0].cpu(), -m.t())
    bvt = torch.randn(3, V2, 130, generator=gen)
    sp, st = torch.zeros(1, V2, 390).cuda(), torch.zeros(1, V2, 390).cuda()
    ops.rank_append(sp, st, torch.zeros(1, dtype=torch.int64).cuda(), bvt.cuda(), (2 * bvt).cuda())
    assert torch.equal(sp[0].cpu(), bvt.permute(1, 0, 2).reshape(V2, 390)) and torch.equal(st[0].cpu(), 2 * bvt.permute(1, 0, 2).reshape(V2, 390))


# ------------------------------------------------------------------------------------------------
# 4. the metric
# ------------------------------------------------------------------------------------------------
def _metric_data(B: int, V: int, T: int, seed: int, slope: float = 0.5):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, V, T, generator=gen)
    pred[:, 0] = torch.round(pred[:, 0] * 2)                          # a column with ties
    true = slope * pred + torch.randn(B, V, T, generator=gen)
    return pred, true


def test_metric_updates_accumulate_bit_for_bit():
    """One update of the [N, V] matrix == updates of its row blocks == one update of the [B, V, T] tensor it flattens ("b v t -> (b t) v")
    == the same tensor as a non-contiguous permuted view == updates whose sizes cross the buffer's doubling points (64, 128, 256, ...);
    compute() within 2^-23 of the f64 mean of scipy's rho; reset() keeps the buffers and starts over."""
    from modeling_utils.metrics import MultidimSpearmanCorrCoef

    B, V, T = 7, 5, 100
    pred, true = _metric_data(B, V, T, seed=1)
    flat_p, flat_t = tribe_ref.flatten_bt(pred).contiguous(), tribe_ref.flatten_bt(true).contiguous()    # [700, V]
    want = scipy_rho(flat_p.numpy(), flat_t.numpy())

    def run(feed):
        metric = MultidimSpearmanCorrCoef(num_outputs=V)
        feed(metric)
        return metric

    whole = run(lambda m: m.update(flat_p.cuda(), flat_t.cuda()))
    rho = whole.per_output()
    assert rho.shape == (1, V) and rho.dtype == torch.float32
    assert (np.abs(rho[0].cpu().numpy().astype(np.float64) - want) <= RHO_TOL).all()
    assert abs(float(whole.compute()) - want.mean()) <= MEAN_TOL

    def blocks(sizes):
        def feed(m):
            at = 0
            for k in sizes:
                m.update(flat_p[at: at + k].cuda(), flat_t[at: at + k].cuda())
                at += k
            assert at == flat_p.shape[0]
        return feed

    p_perm = pred.permute(2, 0, 1).contiguous().cuda().permute(1, 2, 0)      # [B, V, T] view, strides (V, 1, B V)
    t_perm = true.permute(2, 0, 1).contiguous().cuda().permute(1, 2, 0)
    assert not p_perm.is_contiguous() and p_perm.shape == (B, V, T)
    others = {"row blocks": run(blocks([100, 250, 350])),
              "doubling points": run(blocks([1, 62, 1, 1, 63, 1, 127, 200, 244])),
              "bvt": run(lambda m: m.update(pred.cuda(), true.cuda())),
              "bvt permuted view": run(lambda m: m.update(p_perm, t_perm)),
              "bvt in two updates": run(lambda m: (m.update(pred[:3].cuda(), true[:3].cuda()), m.update(pred[3:].cuda(), true[3:].cuda()))),
              "mixed strides": run(lambda m: m.update(p_perm, true.cuda()))}
    for name, metric in others.items():
        assert torch.equal(metric.per_output(), rho), name
        assert torch.equal(metric.compute(), whole.compute()), name
    # reset() followed by reuse: the buffers stay, the result is that of a fresh metric
    metric = others["doubling points"]
    buffer = metric._pred.data_ptr()
    metric.reset()
    with pytest.raises(RuntimeError):
        metric.compute()
    pred2, true2 = _metric_data(2, V, 90, seed=2)
    metric.update(pred2.cuda(), true2.cuda())
    assert metric._pred.data_ptr() == buffer
    fresh = run(lambda m: m.update(pred2.cuda(), true2.cuda()))
    assert torch.equal(metric.per_output(), fresh.per_output())
    want2 = scipy_rho(tribe_ref.flatten_bt(pred2).numpy(), tribe_ref.flatten_bt(true2).numpy())
    assert abs(float(metric.compute()) - want2.mean()) <= MEAN_TOL
    with pytest.raises(ValueError):
        metric.update(torch.zeros(4, V + 1).cuda(), torch.zeros(4, V + 1).cuda())


def test_update_never_synchronises_with_the_host():
    """Plain and with a device-side group tensor (what GroupedMetric hands over after its own groups.tolist()), across buffer growth
    and a new group: torch's synchronisation debug mode raises on any host synchronisation."""
    from modeling_utils.metrics import MultidimSpearmanCorrCoef

    V = 5
    pred, true = (x.cuda() for x in _metric_data(4, V, 30, seed=5))
    slots = [torch.tensor([0, 1, 0, 0]).cuda(), torch.tensor([1, 1, 2, 0]).cuda()]
    plain, grouped = MultidimSpearmanCorrCoef(V), MultidimSpearmanCorrCoef(V)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):   # capacity 120 -> 240 -> 480 -> 960
            plain.update(pred, true)
        grouped.update_bvt(pred, true, slots[0], 2)
        grouped.update_bvt(pred, true, slots[1], 3)
        plain.reset()
        plain.update(pred, true)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert plain._counts.tolist() == [120] and plain._pred.shape[2] >= 600
    assert grouped._counts.tolist() == [4 * 30, 3 * 30, 30] and grouped.per_output().shape == (3, V)


def test_grouped_metric_ranks_within_each_group():
    """3 groups of unequal size interleaved over three [B, V, T] batches (groups [B, 1], as BrainModule passes them), then the
    same rows as [N, V] matrices with one group id per row: each group's value is within 2^-23 of scipy on that group's rows alone (the
    bound for V = 3 weakly correlated outputs, see the module docstring); keys in first-seen order."""
    from modeling_utils.metrics import GroupedMetric

    V, T = 3, 400
    labels = [torch.tensor([5, 2, 5, 5]), torch.tensor([2, 9, 5]), torch.tensor([9, 5, 5, 2, 5])]       # 7 x 5, 3 x 2, 2 x 9
    batches = [_metric_data(len(lab), V, T, seed=10 + i, slope=0.1) for i, lab in enumerate(labels)]
    metric = GroupedMetric("MultidimSpearmanCorrCoef", {"num_outputs": V})
    by_rows = GroupedMetric("MultidimSpearmanCorrCoef", {"num_outputs": V})
    for (pred, true), lab in zip(batches, labels):
        metric.update(pred.cuda(), true.cuda(), groups=lab.view(-1, 1).cuda())
        by_rows.update(tribe_ref.flatten_bt(pred).cuda(), tribe_ref.flatten_bt(true).cuda(), groups=lab.repeat_interleave(T).cuda())
    got = metric.compute()
    assert list(got) == ["5", "2", "9"] and list(by_rows.compute()) == ["5", "2", "9"]
    all_lab = torch.cat(labels)
    all_p, all_t = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    for key in got:
        sel = all_lab == int(key)
        want = scipy_rho(tribe_ref.flatten_bt(all_p[sel]).numpy(), tribe_ref.flatten_bt(all_t[sel]).numpy())
        assert np.abs(want).max() < 0.25
        assert abs(got[key] - want.mean()) <= MEAN_TOL, f"group {key}: {got[key]!r} vs {want.mean()!r}"
        assert by_rows.compute()[key] == got[key]
    assert torch.equal(by_rows._state.per_output(), metric._state.per_output())
    bare = GroupedMetric("MultidimSpearmanCorrCoef")                   # no kwargs: the width of the first update, as for Pearson
    for (pred, true), lab in zip(batches, labels):
        bare.update(pred.cuda(), true.cuda(), groups=lab.cuda())
    assert bare.compute() == got
    metric.reset()
    assert metric._state._total == 0 and metric._state._counts.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------
# BrainModule
# ------------------------------------------------------------------------------------------------
def test_brain_module_logs_spearman_metrics():
    """Two validation batches of B = 3 with mixed subjects through the small model of tests/test_gpu_model.py: val/spearman equals
    scipy on the host copies validation_step returns, one val/subj_spearman/<id> per subject seen, and the Pearson metrics next to
    them are bit-identical to those of a module without the new metric.  The grouped value is the f32 mean of V = 50 values:
    2^-25 + V 2^-24 mean |rho| (a rounding per add of partial sums no larger than sum |rho|)."""
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig
    from modeling_utils.metrics import MetricConfig
    from tests.test_gpu_model import _cuda_batch, _small_pair

    fdims = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
    V, Tout, S = 50, 10, 4
    ref, m = _small_pair(fdims, V, Tout, S)
    adapter = pydantic.TypeAdapter(MetricConfig)
    pearson_cfgs = [{"log_name": "pearson", "name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": V}},
                    {"log_name": "subj_pearson", "name": "GroupedMetric", "metric_name": "MultidimPearsonCorrCoef", "kwargs": {"num_outputs": V}}]
    spearman_cfgs = [{"log_name": "spearman", "name": "MultidimSpearmanCorrCoef", "kwargs": {"num_outputs": V}},
                     {"log_name": "subj_spearman", "name": "GroupedMetric", "metric_name": "MultidimSpearmanCorrCoef",
                      "kwargs": {"num_outputs": V}}]

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

    metrics = build(pearson_cfgs + spearman_cfgs)
    bm, outs = run(metrics)
    preds, trues = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    assert bm.logged["val/spearman"] is metrics["val/spearman"]
    want = scipy_rho(tribe_ref.flatten_bt(preds).numpy(), tribe_ref.flatten_bt(trues).numpy())
    got = metrics["val/spearman"].per_output()[0].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= RHO_TOL).all()
    assert abs(float(metrics["val/spearman"].compute()) - want.mean()) <= MEAN_TOL
    all_subj = torch.cat(subjects).flatten()
    seen = ["2", "0", "3"]                                                      # first-seen order
    assert [k for k in bm.logged if k.startswith("val/subj_spearman/")] == [f"val/subj_spearman/{s}" for s in seen]
    for s in seen:
        sel = all_subj == int(s)
        want_s = scipy_rho(tribe_ref.flatten_bt(preds[sel]).numpy(), tribe_ref.flatten_bt(trues[sel]).numpy())
        bound = 2.0**-25 + V * 2.0**-24 * np.abs(want_s).mean()
        assert abs(bm.logged[f"val/subj_spearman/{s}"] - want_s.mean()) <= bound, s
    only = build(pearson_cfgs)
    bm2, outs2 = run(only)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(outs, outs2))
    assert torch.equal(only["val/pearson"].per_output(), metrics["val/pearson"].per_output())
    pearson_keys = [k for k in bm.logged if k.startswith("val/subj_pearson/")]
    assert len(pearson_keys) == 3 and all(bm2.logged[k] == bm.logged[k] for k in pearson_keys)


# ------------------------------------------------------------------------------------------------
# 5. nothing existing moves
# ------------------------------------------------------------------------------------------------
def test_the_name_spearman_corr_coef_stays_rejected():
    from modeling_utils.metrics import GroupedMetric, MetricConfig

    adapter = pydantic.TypeAdapter(MetricConfig)
    for bad in ({"log_name": "m", "name": "SpearmanCorrCoef"}, {"log_name": "m", "name": "SpearmanCorrCoef", "kwargs": {"num_outputs": 3}}):
        with pytest.raises(pydantic.ValidationError):
            adapter.validate_python(bad)
    with pytest.raises(AssertionError):
        GroupedMetric("SpearmanCorrCoef")
