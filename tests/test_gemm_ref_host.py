"""CPU (no GPU): oracle/gemm_ref.py is what tests/test_gpu_gemm_bounds.py holds the bf16 GEMM to, so it is pinned here first -- the
exactness argument to three f32 summation orders, the float64 activations to torch's, the replays of the launcher's stream-K and split-K
plans to the case table (and to the library's own planner, a host-only call)."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gemm_ref as ref


@pytest.mark.parametrize("name,K,alpha,addends,scale,bmax", ref.EXACT_FAMILIES, ids=[f[0] for f in ref.EXACT_FAMILIES])
def test_every_exact_case_meets_its_exactness_condition(name, K, alpha, addends, scale, bmax):
    assert ref.is_exact(K, alpha, addends, scale, bmax), name
    assert K % ref.BK == 0
    if name == "ext activations":
        assert K <= ref.ACT_MAX_K and bmax == 1


def test_exactness_condition_refuses_what_is_not_exact():
    assert not ref.is_exact(2**21, 1.0, False)            # 9 K >= 2^24
    assert not ref.is_exact(4096, 2.0, True, 2.0, 3)      # 9 * 4096 * 2 * 2 * 2 >= 2^18: the split-K operator cases draw B from [-1, 1]
    assert not ref.is_exact(64, 0.3, False)               # alpha is no power of two
    assert ref.is_exact(131072, 0.5, False) and ref.is_exact(4096, 2.0, True)


@pytest.mark.parametrize("K,alpha,addends", [(131072, 0.5, False), (22016, 0.5, False), (4096, 2.0, True), (256, 1.0, True)])
def test_sums_of_integer_products_are_exact_in_any_order(K, alpha, addends):
    """Forward, reversed and pairwise f32 summation of a case's products give the same bits -- also with every product at full
    magnitude and one sign (the worst case of the condition) -- and the epilogue on top of the sum is exact in f32 too."""
    a, b = ref.exact_operands((4, K), (4, K), seed=K)
    g = np.random.default_rng(K)
    for row in range(4):
        p = a[row] * b[row]
        fwd, rev, pair = ref.f32_sums(p)
        assert fwd.tobytes() == rev.tobytes() == pair.tobytes()
        assert float(fwd) == float(a[row].astype(np.float64) @ b[row].astype(np.float64))
        y = np.float32(fwd) * np.float32(alpha)
        y64 = float(fwd) * alpha
        if addends:
            bias, res, rs = ref.sixty_fourths(g, 1)[0], ref.sixty_fourths(g, 1)[0], np.float32(0.5)
            y = np.float32(np.float32(y + bias) + np.float32(res * rs))
            y64 = y64 + float(bias) + float(res) * 0.5
        assert float(y) == y64
    worst = np.full(K, 9.0, dtype=np.float32)
    fwd, rev, pair = ref.f32_sums(worst)
    assert float(fwd) == float(rev) == float(pair) == 9.0 * K


def test_generators_give_what_the_argument_assumes():
    g = np.random.default_rng(0)
    a, b = ref.exact_operands((50, 64), (70, 64), seed=1, bmax=1)
    assert np.abs(a).max() == 3 and np.abs(b).max() == 1 and np.array_equal(a, np.rint(a))
    assert np.array_equal(torch.from_numpy(a).bfloat16().float().numpy(), a)
    q = ref.sixty_fourths(g, 1000)
    assert np.abs(q).max() <= 2 and np.array_equal(q * 64, np.rint(q * 64)) and len(np.unique(q)) > 100
    e = ref.sixty_fourths(g, 1000, lo=-24.0, hi=0.0)
    assert e.min() >= -24 and e.max() <= 0 and e.min() < -20
    assert set(np.unique(ref.power_of_two(g, 200))) == {0.5, 1.0, 2.0}
    t = ref.random_inputs(24, 16, 64, trans_ab=True)
    assert t["a"].shape == (64, 24) and t["base"].shape == (24, 16) and (t["S"] >= np.abs(t["base"])).all()
    assert np.array_equal(torch.from_numpy(t["a"]).bfloat16().float().numpy(), t["a"])


def test_activations_agree_with_torch_float64():
    g = torch.Generator().manual_seed(3)
    v = (torch.randn(64, 48, generator=g, dtype=torch.float64) * 4)
    v[0, :8] = torch.tensor([-40.0, -12.0, -6.0, -0.0, 0.0, 6.0, 12.0, 40.0], dtype=torch.float64)
    n = v.numpy()
    close = lambda got, want: np.testing.assert_allclose(got, want.numpy(), rtol=1e-13, atol=1e-300)      # noqa: E731
    close(ref.act64(n, "silu"), F.silu(v))
    # torch's 1 + erf cancels on the negative side (absolute error ~1e-16 |v|); the reference takes erfc there
    np.testing.assert_allclose(ref.act64(n, "gelu"), F.gelu(v).numpy(), rtol=1e-13, atol=1e-14)
    close(ref.act64(n, "exp2"), torch.exp2(v))
    # torch's glu splits into halves, the kernels pair adjacent columns (even = first half's role)
    close(ref.act64(n, "glu"), F.glu(torch.cat([v[:, 0::2], v[:, 1::2]], dim=1), dim=1))
    close(ref.act64(n, "swiglu"), F.silu(v[:, 0::2]) * v[:, 1::2])
    aux = (torch.randn(64, 48, generator=g, dtype=torch.float64) * 3).requires_grad_()
    F.gelu(aux).sum().backward()
    np.testing.assert_allclose(ref.gelu_grad64(aux.detach().numpy()), aux.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref.act64(n, "gelu_bwd", aux.detach().numpy()), (v * aux.grad).numpy(), rtol=1e-11, atol=1e-14)
    close(ref.act64(n, "mul_aux", aux.detach().numpy()), v * aux.detach())


def test_reference_of_a_whole_descriptor_agrees_with_torch():
    """Every operator at once (a launch never carries all of them, the reference does not care), batches and gather1."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    M, N, K = 13, 10, 64
    a, b = r(M, K), r(N, K)
    rs, rb, res, rsc, rowadd, gadd = r(M), r(M), r(M, N), r(N), r(3, N), r(4, N)
    gidx = np.array([3, 0, 3, 1, 2])
    got, pre = ref.epilogue64((a @ b.t()).numpy(), alpha=0.5, row_scale=rs.numpy(), row_bias=rb.numpy(), act="gelu", res=res.numpy(),
                              res_scale=rsc.numpy(), rowadd=rowadd.numpy(), rowadd_period=3, gadd=gadd.numpy(), gadd_index=gidx, gadd_div=3,
                              want_preact=True)
    v = 0.5 * (a @ b.t()) * rs[:, None] + rb[:, None]
    rows = torch.arange(M)
    want = F.gelu(v) + res * rsc + rowadd[rows % 3] + gadd[torch.from_numpy(gidx)[rows // 3]]
    np.testing.assert_allclose(pre, v.numpy(), rtol=1e-13)
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-13)
    # transposed operands, batches, gather
    at, bt = r(3, 2, K, M), r(3, 2, K, N)
    cb, rsd = r(3, 2, N), r(3, 2, M, N)
    gather = [2, 0, 2]
    for flag in ("gather_a", "gather_b", "gather_bias"):
        got = ref.reference64(at.numpy(), bt.numpy(), trans_ab=True, gather1=gather, col_bias=cb.numpy(), res=rsd.numpy(), alpha=2.0,
                              **{flag: True})
        for b1 in range(3):
            ia, ib, ibias = (gather[b1] if flag == f else b1 for f in ("gather_a", "gather_b", "gather_bias"))
            for b0 in range(2):
                want = 2.0 * at[ia, b0].t() @ bt[ib, b0] + cb[ibias, b0] + rsd[b1, b0]
                np.testing.assert_allclose(got[b1, b0], want.numpy(), rtol=1e-12, atol=1e-12)
    assert ref.bf16_value(np.array([0x3F80, 0xC040, 0x0000], dtype=np.uint16)).tolist() == [1.0, -3.0, 0.0]


@pytest.mark.parametrize("shape", list(ref.STREAM_K_CASES), ids=["x".join(map(str, s)) for s in ref.STREAM_K_CASES])
def test_stream_k_replay_classifies_the_cases_as_the_table_claims(shape):
    M, N, K = shape
    claim = ref.STREAM_K_CASES[shape]
    tiles, nk = ref.tiles256(M, N), K // ref.BK
    plan = ref.plan_stream_k(tiles, nk)
    if claim is None:
        assert plan is None
    else:
        assert tiles == claim["tiles"]
        assert {k: plan[k] for k in ("tiles_dp", "q", "second", "idle", "parts")} == {k: claim[k] for k in ("tiles_dp", "q", "second", "idle", "parts")}
        # inside the stream-K region no run holds a whole tile: the two branches the GPU test cannot reach (its docstring)
        assert plan["q"] < nk and plan["parts"][0] >= 2
    # the library's planner (host-only; 256 workers where there is no GPU to ask) says the same, and the kernel-side decode of that
    # schedule covers every K-step once: the replay tests/test_abi_and_host.py already holds
    from tribe_hip import _lib
    from test_abi_and_host import test_stream_k_schedule_covers_every_k_step_once as decode_replay

    out = (ctypes.c_int32 * 260)()
    grid = _lib.lib().tribe_gemm_stream_k_plan(tiles, nk, out)
    if plan is None:
        assert grid == tiles
    else:
        assert (grid, out[0], out[1], out[2], out[3]) == (plan["grid"], plan["tiles_dp"], plan["rem_units"], plan["q"], 256)
        assert list(out[4: 4 + plan["second"]]) == plan["second_worker"]
    decode_replay(tiles, nk)


def test_stream_k_with_half_a_round_never_hands_a_run_a_whole_tile():
    """With W = 256 and a remainder of at most half a round q = ceil(rem nk / 256) <= ceil(nk / 2) < nk (nk >= 16 there): `partial ==
    false` inside the stream-K region and `w_lo == w_hi` in the reduce kernel cannot happen."""
    for tiles in range(1, 129):
        for nk in (16, 17, 31, 64, 344, 2048):
            plan = ref.plan_stream_k(tiles, nk)
            if plan is not None:
                assert plan["q"] < nk and plan["parts"][0] >= 2


@pytest.mark.parametrize("shape", list(ref.SPLIT_K_CASES), ids=["x".join(map(str, s)) for s in ref.SPLIT_K_CASES])
def test_split_k_replay_gives_the_share_counts_the_table_claims(shape):
    M, N, K = shape
    shares = ref.split_k_shares(M, N, K)
    assert shares == ref.SPLIT_K_CASES[shape] and sum(shares) == K // ref.BK and min(shares) >= 8
    from tribe_hip import _lib

    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0, d.alpha, d.stream_k, d.tile_hint = M, N, K, 1, 1, 1.0, 1, 3
    d.lda = d.ldb = K
    d.ldc = N
    assert _lib.lib().tribe_gemm_stream_k_workspace_bytes(ctypes.byref(d)) == len(shares) * M * N * 4


def test_split_k_replay_leaves_short_and_large_launches_whole():
    assert ref.split_k_shares(128, 128, 960) == [15]           # 15 K-steps: fewer than two shares of 8
    assert ref.split_k_shares(2048, 2048, 4096) == [64]        # 256 tiles: a whole round already
    assert ref.split_k_shares(128, 3072, 12288) == [24] * 8
