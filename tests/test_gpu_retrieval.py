"""GPU: the retrieval metrics Rank / TopkAcc (csrc/metrics.hip) against the reference's own results (g14, produced by executing its
metrics.py) and, at gallery sizes the fixture cannot hold, against an f64 restatement of metrics.py:66-218."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
REDUCTIONS = ("mean", "median", "std")


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(golden_dir / "g14_retrieval.npz")


def _updates(g, case):
    ups = []
    for i in range(int(g[f"{case}__n_updates"])):
        xl = [str(int(c)) for c in g[f"{case}__xl{i}"]] if f"{case}__xl{i}" in g else None
        yl = [str(int(c)) for c in g[f"{case}__yl{i}"]] if f"{case}__yl{i}" in g else None
        ups.append((torch.from_numpy(g[f"{case}__x{i}"]).to(DEV), torch.from_numpy(g[f"{case}__y{i}"]).to(DEV), xl, yl))
    return ups


def ranks_f64(x, y, true_idx=None, relative=False, tol=1e-5):
    """metrics.py:114-153 in f64 (s = x y^T / (1e-15 + |y|)).  Also returns the queries whose rank is decided at f32 precision: no
    score of a gallery row that differs from the true row lies within `tol` relative of the true score."""
    x64, y64 = x.double(), y.double()
    n, m = x.shape[0], y.shape[0]
    t = torch.arange(n, device=x.device) if true_idx is None else true_idx
    inv = 1.0 / (1e-15 + y64.norm(dim=1))
    ranks = torch.empty(n, dtype=torch.float64, device=x.device)
    decided = torch.empty(n, dtype=torch.bool, device=x.device)
    for c0 in range(0, n, 1024):
        sl = slice(c0, min(n, c0 + 1024))
        s = (x64[sl] @ y64.T) * inv
        ts = s.gather(1, t[sl, None])
        gt = (s > ts).sum(1)
        ge = (s >= ts).sum(1) - 1
        ranks[sl] = (gt + ge).double() / 2
        same_row = (y[None, :, :] == y[t[sl]][:, None, :]).all(-1) if m * (sl.stop - c0) * y.shape[1] <= 2**24 else \
            torch.zeros_like(s, dtype=torch.bool)
        scale = torch.maximum(ts.abs(), s.square().mean(1, keepdim=True).sqrt())   # relative to the scores' own size
        near = ((s - ts).abs() <= tol * scale) & ~same_row
        near.scatter_(1, t[sl, None], False)
        decided[sl] = ~near.any(1)
    ranks[ranks < 0] = n // 2
    if relative:
        ranks /= m
    return ranks.float(), decided


def test_g14_ranks_and_reductions_equal_the_reference(g14):
    from modeling_utils.metrics.metrics import Rank, TopkAcc

    for case in [str(c) for c in g14["cases"]]:
        rel = bool(g14[f"{case}__relative"])
        want = torch.from_numpy(g14[f"{case}__ranks"])
        expect = g14[f"{case}__compute"]
        metrics = [Rank(reduction=r, relative=rel) for r in REDUCTIONS] + ([] if rel else [TopkAcc(1), TopkAcc(5)])
        for m in metrics:
            for x, y, xl, yl in _updates(g14, case):
                m.update(x, y, xl, yl)
            got = m.ranks.cpu()
            assert torch.equal(got, want), f"{case}: ranks {got.tolist()} vs reference {want.tolist()}"
        for i, m in enumerate(metrics):
            val = float(m.compute())
            if i == 1:   # median: exact
                assert val == expect[i], f"{case}: median {val} vs {expect[i]}"
            else:
                assert abs(val - expect[i]) <= 1e-6 * max(1.0, abs(expect[i])), f"{case}: compute[{i}] {val} vs {expect[i]}"


def test_compute_ranks_returns_without_touching_the_state(g14):
    from modeling_utils.metrics.metrics import Rank

    m = Rank()
    x, y, xl, yl = _updates(g14, "labelled")[0]
    r = m._compute_ranks(x, y, xl, yl)
    assert torch.equal(r.cpu(), torch.from_numpy(g14["labelled__ranks"])) and m.ranks.numel() == 0
    with pytest.raises(ValueError):
        m.update(x, y)   # N != M without labels
    with pytest.raises(ValueError):
        m.update(x, y, ["nope"] + xl[1:], yl)


def test_update_bvt_fuses_the_time_means(g14):
    from modeling_utils.metrics.metrics import Rank
    from tribe_hip import ops

    pred = torch.from_numpy(g14["bvt__pred"]).to(DEV)
    target = torch.from_numpy(g14["bvt__target"]).to(DEV)
    want = torch.from_numpy(g14["bvt__ranks"])
    m = Rank()
    m.update_bvt(pred, target)
    got = m.ranks.cpu()
    # queries whose reference means sit within 1e-5 of a tie are compared against the ranks of the kernel's own means instead
    _, decided = ranks_f64(torch.from_numpy(g14["bvt__x0"]), torch.from_numpy(g14["bvt__y0"]))
    xk, yk, _, _ = ops.retrieval_prep(pred, target, mean=True)
    own = Rank()
    own.update(xk, yk)
    assert torch.equal(got[decided], want[decided]), (got, want)
    assert torch.equal(got[~decided], own.ranks.cpu()[~decided])
    assert int(decided.sum()) >= 14 and (got % 1 == 0.5).any()   # the duplicated target rows tie exactly
    # kernel means: f64 sums rounded once
    torch.testing.assert_close(xk.cpu(), torch.from_numpy(g14["bvt__x0"]), rtol=1e-6, atol=1e-7)
    # a strided (non T'-contiguous) view of the same data takes the fallback path and gives the same ranks
    p2 = pred.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    t2 = target.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    m2 = Rank()
    m2.update_bvt(p2, t2)
    assert torch.equal(m2.ranks.cpu(), got)


def test_compute_sim_four_norm_kinds(g14):
    from modeling_utils.metrics.metrics import Rank

    x = torch.from_numpy(g14["sim__xin"]).to(DEV)
    y = torch.from_numpy(g14["sim__yin"]).to(DEV)
    for kind in (None, "x", "y", "xy"):
        got = Rank._compute_sim(x, y, norm_kind=kind).cpu()
        want = torch.from_numpy(g14[f"sim__{kind}"])
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6, msg=f"norm_kind {kind}")
    with pytest.raises(ValueError):
        Rank._compute_sim(x, y, norm_kind="z")
    labels, scores = Rank._compute_topk_scores(x, y, [f"g{i}" for i in range(y.shape[0])], k=3)
    s = g14["sim__y"]
    for n in range(x.shape[0]):
        assert scores[n] == sorted(scores[n], reverse=True) and len(labels[n]) == 3
        assert abs(scores[n][0] - s[n].max()) <= 1e-5 * max(1.0, abs(s[n].max()))


def test_reset_starts_a_new_epoch(g14):
    from modeling_utils.metrics.metrics import TopkAcc

    m = TopkAcc(topk=1)
    for x, y, xl, yl in _updates(g14, "plain"):
        m.update(x, y, xl, yl)
    m.reset()
    for x, y, xl, yl in _updates(g14, "ties"):
        m.update(x, y, xl, yl)
    assert torch.equal(m.ranks.cpu(), torch.from_numpy(g14["ties__ranks"]))
    assert abs(float(m.compute()) - g14["ties__compute"][3]) <= 1e-6


def test_update_bvt_never_synchronises_with_the_host():
    from modeling_utils.metrics.metrics import TopkAcc

    g = torch.Generator(device=DEV).manual_seed(3)
    pred = torch.randn(16, 1000, 100, device=DEV, generator=g)
    target = 0.2 * pred + torch.randn(16, 1000, 100, device=DEV, generator=g)
    m = TopkAcc(topk=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):   # the state buffer grows (64 -> 128 -> 256) along the way
            m.update_bvt(pred, target)
        out = m.compute()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert m.ranks.numel() == 160
    r = m.ranks.view(10, 16)
    assert torch.equal(r, r[:1].expand(10, 16)) and float(out) == float((r[0] < 1).float().mean())


def test_gallery_8192_matches_the_f64_restatement_without_a_score_matrix():
    from modeling_utils.metrics.metrics import Rank

    N = M = 8192
    V = 1000
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, V, device=DEV, generator=g)
    y = 0.03 * x + torch.randn(N, V, device=DEV, generator=g)
    m = Rank(reduction="mean")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.update(x, y)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < N * M * 4, f"update allocated {peak} bytes at its peak"
    want, decided = ranks_f64(x, y)
    got = m.ranks
    assert int(decided.sum()) >= 0.9 * N
    assert torch.equal(got[decided], want[decided]), int((got[decided] != want[decided]).sum())
    assert float(got.max()) > 100   # the ranks are spread: the comparison covers much more than rank 0
    torch.testing.assert_close(m.compute().double(), got.double().mean(), rtol=1e-6, atol=0)


def test_labelled_gallery_of_ten_thousand_rows():
    from modeling_utils.metrics.metrics import Rank

    N, M, V = 3000, 10000, 256
    g = torch.Generator(device=DEV).manual_seed(12)
    y = torch.randn(M, V, device=DEV, generator=g)
    codes = torch.randint(0, 7000, (M,), generator=torch.Generator().manual_seed(1)).tolist()   # repeated labels
    y_labels = [f"seg{c}" for c in codes]
    pick = torch.randint(0, M, (N,), generator=torch.Generator().manual_seed(2)).tolist()
    x_labels = [y_labels[i] for i in pick]
    t = torch.tensor([y_labels.index(lab) for lab in x_labels], device=DEV)
    x = 0.1 * y[t] + torch.randn(N, V, device=DEV, generator=g)
    for rel in (False, True):
        m = Rank(relative=rel)
        m.update(x, y, x_labels, y_labels)
        want, decided = ranks_f64(x, y, t, relative=rel)
        assert int(decided.sum()) >= 0.9 * N
        assert torch.equal(m.ranks[decided], want[decided])
        if not rel:
            assert float(m.compute()) == float(torch.sort(m.ranks).values[(N - 1) // 2])   # lower median


def test_run_step_logs_retrieval_top1():
    from algonauts2025.model import FmriEncoderConfig
    from algonauts2025.pl_module import BrainModule
    from data_utils.dataloader import SegmentData
    from modeling_utils.losses import TorchLossConfig
    from modeling_utils.metrics import MultidimPearsonCorrCoef
    from modeling_utils.metrics.metrics import TopkAcc
    from oracle import tribe_ref

    fdims = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
    V, Tout, S, B, T = 60, 12, 3, 8, 40
    model = FmriEncoderConfig(n_subjects=S, hidden=768, depth=2, heads=4).build(fdims, V, Tout)
    ref = tribe_ref.FmriEncoderRef(fdims, V, Tout, S, dims=tribe_ref.EncoderDims(hidden=768, depth=2, heads=4))
    with torch.no_grad():
        tribe_ref.fill_params_(ref, seed=0)
    model.load_state_dict(ref.state_dict())
    model = model.to(DEV).eval()
    data = tribe_ref.synthetic_batch(B, T, fdims, S, seed=1)
    fmri = torch.randn(B, V, Tout, generator=torch.Generator().manual_seed(5))
    batch = SegmentData(data={**{k: v.to(DEV) for k, v in data.items()}, "fmri": fmri.to(DEV)}, segments=[None] * B)
    top1 = TopkAcc(topk=1)
    metrics = {"val/retrieval_top1": top1, "val/pearson": MultidimPearsonCorrCoef(V)}
    bm = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, metrics)
    with torch.no_grad():
        _, pred, target = bm._run_step(batch, 0, "val")
    assert bm.logged["val/retrieval_top1"] is top1 and "val/pearson" in bm.logged
    want, decided = ranks_f64(pred.mean(-1), target.mean(-1))
    got = top1.ranks.cpu()
    assert got.shape == (B,) and int(decided.sum()) >= B - 1
    assert torch.equal(got[decided], want[decided])
    assert float(top1.compute()) == float((got < 1).float().mean())
