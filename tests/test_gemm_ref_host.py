"""CPU (no GPU): oracle/gemm_ref.py is what tests/test_gpu_gemm_bounds.py holds the bf16 GEMM to, so it is pinned here first -- the
exactness argument to three f32 summation orders, the float64 activations to torch's, the replays of the launcher's stream-K and split-K
plans to the case table (and to the library's own planner, a host-only call).  For tests/test_gpu_gemm_forward_bounds.py: its case table
(exactness, the replayed epilogue path of every row, coverage of every kernel x path x operator set, no row to spare, the kernel the
library's planner gives each row) and the faults its inputs must be able to tell from correct code."""

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


# ------------------------------------------------------------------------------------------------
# the forward operators on the four NT tile kernels: the case table of tests/test_gpu_gemm_forward_bounds.py
# ------------------------------------------------------------------------------------------------
FWD = ref.FWD_CASES
FWD_PATHS_OF = [ref.fwd_paths(c) for c in FWD]
FWD_SHAPES = sorted({(c.M, c.N, c.K, c.ops) for c in FWD if ref.fwd_exact(c.ops)})


def _spec(ops):
    return ref.FWD_OPS[ops]


def _slow(ops):
    """Sets epilogue_fast never takes: a gadd, a rowadd beside a residual."""
    return bool(_spec(ops).get("gadd") or (_spec(ops).get("rowadd") and _spec(ops).get("res")))


def test_forward_exact_cases_meet_their_exactness_condition():
    assert ref.is_exact_sumsq(128, 1, 64) and ref.is_exact_sumsq(128, 1, 48)
    assert not ref.is_exact_sumsq(128, 3, 64) and not ref.is_exact_sumsq(256, 1, 64)      # 1158^2 * 64 and 774^2 * 64 pass 2^24
    for c in FWD:
        spec = _spec(c.ops)
        if not ref.fwd_exact(c.ops):
            assert spec["bmax"] == 1 and c.K <= ref.ACT_MAX_K, c.id          # bounded: the GELU sees an exact pre-activation near 0
            continue
        addends = any(spec.get(k) for k in ("col_bias", "row_bias", "res", "rowadd", "gadd"))
        assert ref.is_exact(c.K, spec.get("alpha", 1.0), addends, 2.0 if spec.get("row_scale") else 1.0, spec.get("bmax", 3)), c.id
        if spec.get("fused"):
            assert ref.is_exact_sumsq(c.K, spec["bmax"], ref.FWD_KERNELS[c.kernel][3]), c.id
        assert c.K % ref.BK == 0 and (c.hint == 0 or (c.M, c.N, c.K) <= ref.FWD_SUMSQ_SHAPE and c.N <= 768), c.id
    # the argument, on the values themselves: every EXACT reference is an f32 value, every slot an integer below 2^24
    for M, N, K, ops in FWD_SHAPES:
        y, _ = ref.fwd_reference(M, N, K, ops)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y), (M, N, K, ops)
        if _spec(ops).get("fused"):
            assert np.array_equal(y, np.rint(y)) and np.abs(y).max() <= 3 * K + 6
            for cols in (48, 64):
                s = ref.fwd_slots(y, cols)
                assert s.max() < 2**24 and s.shape == (M, N // cols)
                # summed in f32 in two orders: the same bits
                x2 = (y.astype(np.float32) ** 2).reshape(M, N // cols, cols)
                fwd, rev = np.cumsum(x2, axis=2, dtype=np.float32)[:, :, -1], np.cumsum(x2[:, :, ::-1], axis=2, dtype=np.float32)[:, :, -1]
                assert np.array_equal(fwd, rev) and np.array_equal(fwd.astype(np.float64), s)


def _forward_requirements():
    """What the table must hold, as (name, predicate of a case and its replayed paths), stated from the issue's lists and not from the
    table: every operator set on every kernel on every path that admits it in every dtype it runs with; the three ways into the scalar
    branch and into the vector branch; the ragged bottoms; tile_hint 6; the three auto-dispatch kinds."""
    req = {}

    def need(name, **want):
        paths = want.pop("paths", None)
        has = want.pop("has", None)
        req[name] = lambda c, p: all(getattr(c, k) == v for k, v in want.items()) and (paths is None or p == frozenset(paths)) and \
            (has is None or frozenset(has) <= p)

    for kernel, (_, _, bn, _, hint) in ref.FWD_KERNELS.items():
        for ops, spec in ref.FWD_OPS.items():
            p2 = {"P2b"} if spec.get("gadd") else {"P2c"} if _slow(ops) else {"P1", "P2a"}
            routes = {} if _slow(ops) else {"P1": {"P1"}}
            if not spec.get("p1_only"):
                routes |= {"P2": p2, "P3": {"P3a"}}
            for out in ref.fwd_dtypes(ops):
                for route, paths in routes.items():
                    if spec.get("fused"):
                        M, N, K = ref.FWD_SUMSQ_SHAPE
                        for variant in ("pad", "sspad"):                 # packed slots, and a slot pitch above the slot count
                            need((kernel, ops, out, route, variant), hint=hint, kernel=kernel, ops=ops, out=out, M=M, N=N, K=K, variant=variant,
                                 paths=paths)
                    else:
                        need((kernel, ops, out, route), hint=hint, kernel=kernel, ops=ops, out=out, M=300, K=128, paths=paths)
        for out in ("f32", "bf16"):
            need((kernel, "C + 1", out), hint=hint, kernel=kernel, ops="res", out=out, variant="c1", paths={"P3b"})
            need((kernel, "bias + 1", out), hint=hint, kernel=kernel, ops="col_bias", out=out, variant="bias1", paths={"P3b"})
            need((kernel, "N % 4 == 2", out), hint=hint, kernel=kernel, ops="res", out=out, N=bn + 6, paths={"P1", "P2a", "P3c"})
            need((kernel, "M = 70", out), hint=hint, kernel=kernel, ops="none", out=out, M=70, paths={"P1"})
        for M in (70, 200):
            need((kernel, "in place", M), hint=hint, kernel=kernel, ops="out_proj", out="f32", M=M, paths={"P1"})
    for ops in ref.FWD_OPS:
        for out in ref.fwd_dtypes(ops):
            paths = {"P2b"} if _spec(ops).get("gadd") else {"P2c"} if _slow(ops) else {"P1"}
            need((6, ops, out), hint=6, kernel="w8_256", ops=ops, out=out, has=paths)
    need((6, "192 wide", "f32"), hint=6, kernel="w8_192", ops="out_proj", out="f32", paths={"P1"})
    need((6, "192 wide", "bf16"), hint=6, kernel="w8_192", ops="col_bias", out="bf16", paths={"P1"})
    for kernel in ("db128", "ring128", "w8_192"):
        need((0, kernel), hint=0, kernel=kernel)
    return req


def _unmet(cases, paths):
    return [name for name, ok in _forward_requirements().items() if not any(ok(c, p) for c, p in zip(cases, paths))]


def test_forward_table_covers_every_kernel_path_and_operator_set():
    assert _unmet(FWD, FWD_PATHS_OF) == []
    assert len(set(FWD)) == len(FWD)
    forced = [(c, p) for c, p in zip(FWD, FWD_PATHS_OF) if c.hint in (1, 2, 3, 4)]
    # every cell of {4 kernels} x {7 paths}
    cells = {(c.kernel, path) for c, p in forced for path in p}
    assert cells == {(k, path) for k in ref.FWD_KERNELS for path in ref.FWD_PATHS}
    # every operator set on every kernel, on every path it admits
    for kernel in ref.FWD_KERNELS:
        for ops, spec in ref.FWD_OPS.items():
            got = set().union(*[p for c, p in forced if c.kernel == kernel and c.ops == ops])
            want = {"P1"} if spec.get("p1_only") else {"P2b", "P3a"} if spec.get("gadd") else {"P2c", "P3a"} if _slow(ops) else {"P1", "P2a", "P3a"}
            assert want <= got, (kernel, ops, got)
    # P3c sits beside vector quads of the same rows: ldc % 4 == 0 there
    for c, p in forced:
        assert ("P3c" in p) == (c.N % 4 == 2) and (c.N % 4 == 0 or ref.fwd_layout(c)["ldc"] % 4 == 0), c.id
    # the layouts the issue asks for: every pitch above its matrix, one ldc pad that is no multiple of 4
    for c in FWD:
        lay = ref.fwd_layout(c)
        assert lay["ldc"] > c.N and lay["ldres"] > c.N and lay["ld_c_bf16"] > c.N and lay["lda"] > c.K and lay["ldb"] > c.K
    assert any((ref.fwd_layout(c)["ldc"] - c.N) % 4 for c in FWD)
    assert any(ref.fwd_layout(c).get("ld_row_sumsq", 0) > ref.fwd_layout(c).get("slots", 0) for c in FWD)


def test_forward_table_has_no_row_to_spare():
    """A thinned table fails: every row is the only one that meets some requirement."""
    req = _forward_requirements()
    sole = set()
    for name, ok in req.items():
        who = [i for i, (c, p) in enumerate(zip(FWD, FWD_PATHS_OF)) if ok(c, p)]
        assert who, name
        if len(who) == 1:
            sole.add(who[0])
    spare = [FWD[i].id for i in range(len(FWD)) if i not in sole]
    assert spare == []
    for drop in (0, len(FWD) // 2, len(FWD) - 1):                      # and said the long way, for three rows
        assert _unmet(FWD[:drop] + FWD[drop + 1:], FWD_PATHS_OF[:drop] + FWD_PATHS_OF[drop + 1:]) != []


def test_forward_path_replay_on_hand_made_cases():
    mk = lambda N, ops, variant, out="f32", kernel="db128", hint=1: ref.FwdCase(hint, 300, N, 128, ops, variant, out, kernel)      # noqa: E731
    P = lambda *a, **k: set(ref.fwd_paths(mk(*a, **k)))                                                                          # noqa: E731
    assert P(256, "none", "pad") == {"P1"} and P(128, "res", "pad") == {"P1"}
    assert P(136, "none", "pad") == {"P1", "P2a"} and P(120, "none", "pad") == {"P2a"}
    assert P(264, "none", "pad", kernel="w8_256", hint=2) == {"P1", "P2a"} and P(264, "none", "pad", kernel="w8_192", hint=4) == {"P1", "P2a"}
    assert P(192, "none", "pad", kernel="w8_256", hint=2) == {"P2a"} and P(192, "none", "pad", kernel="w8_192", hint=4) == {"P1"}
    assert P(256, "projector", "pad") == {"P2b"} and P(256, "rowadd_res", "pad") == {"P2c"} and P(256, "bias_rowadd7", "pad") == {"P1"}
    assert P(256, "none", "ldc2") == {"P3a"} and P(256, "projector", "ldc2") == {"P3a"}
    assert P(256, "none", "c1") == {"P3b"} and P(256, "none", "c1", out="bf16") == {"P3b"}
    assert P(256, "col_bias", "bias1") == {"P3b"} and P(256, "none", "bias1") == {"P1"}       # no bias: nothing is misaligned
    assert P(134, "res", "pad") == {"P1", "P2a", "P3c"} and P(126, "projector", "pad") == {"P2b", "P3c"}


@pytest.mark.parametrize("case", FWD, ids=[c.id for c in FWD])
def test_forward_case_gets_the_kernel_it_names_from_the_library_planner(case):
    """tribe_debug_gemm_plan is a host call (256 compute units where there is no GPU to ask): kind, tile and the generic epilogue."""
    from tribe_hip import _lib

    names = ("a", "b", "c", "cb", "icb", "rb", "res", "ires", "rs", "irs", "row_scale", "rowadd7", "rowadd32", "gadd", "gidx", "c_bf16", "row_sumsq")
    d = ref.fwd_fill_desc(_lib.GemmDesc(), _lib, case, {n: (i + 1) << 32 for i, n in enumerate(names)})
    out = (ctypes.c_int64 * 19)()
    assert _lib.lib().tribe_debug_gemm_plan(ctypes.byref(d), 0, out, 19) == 0, _lib.lib().tribe_last_error()
    kind, _, bn, cols, _ = ref.FWD_KERNELS[case.kernel]
    assert (out[1], out[3], out[7], out[5]) == (kind, bn, 0, 1), case.id
    if _spec(case.ops).get("fused"):
        assert out[4] == cols and _lib.lib().tribe_gemm_sumsq_slots(ctypes.byref(d)) == ref.fwd_layout(case)["slots"]


def _differs(want, fault, bits):
    assert want.shape == fault.shape
    if not (want != fault).any():
        return False
    return not bits or (ref.fwd_bf16_bits(want) != ref.fwd_bf16_bits(fault)).any()


FAULT_SETS = {"rowadd_next_row": ("bias_rowadd7", "bias_rowadd32", "rowadd_res", "projector"),
              "rowadd_mod16": ("bias_rowadd7", "bias_rowadd32", "rowadd_res", "projector"), "gadd_next_row": ("projector",),
              "bias_shift4": ("col_bias", "out_proj", "bias_rowadd7", "bias_rowadd32", "fused_norm"), "res_scale_shift4": ("out_proj", "fused_norm"),
              "quads_permuted": tuple(o for o in ref.FWD_OPS if ref.fwd_exact(o)), "subtiles_swapped": tuple(o for o in ref.FWD_OPS if ref.fwd_exact(o))}


@pytest.mark.parametrize("fault", list(FAULT_SETS))
def test_forward_inputs_tell_an_addressing_fault_from_the_true_result(fault):
    """The float64 result of a kernel with the fault differs from the true one on every EXACT case that carries the operator -- in
    value, and where the case has a bf16 output in the rounded bit patterns too.  Otherwise a pass would prove nothing."""
    seen = 0
    for M, N, K, ops in FWD_SHAPES:
        if ops not in FAULT_SETS[fault]:
            continue
        for lead in sorted({ref.fwd_layout(c)["bias_lead"] for c in FWD if (c.M, c.N, c.K, c.ops) == (M, N, K, ops)}):
            want, bad = ref.fwd_reference(M, N, K, ops, lead)[0], ref.fwd_reference(M, N, K, ops, lead, fault)[0]
            bits = any(c.out == "bf16" for c in FWD if (c.M, c.N, c.K, c.ops) == (M, N, K, ops)) or bool(_spec(ops).get("fused"))
            assert _differs(want, bad, bits), (fault, M, N, K, ops)
            # not in a corner only: the fault shows in more than one row and more than one column
            rows, cols = np.nonzero(want != bad)
            assert len(set(rows)) > 1 and len(set(cols)) > 1
            seen += 1
    assert seen >= 3          # (shapes are shared between kernels: three tile widths at the least)


def test_forward_inputs_tell_slot_faults_and_a_double_rounding():
    M, N, K = ref.FWD_SUMSQ_SHAPE
    y, _ = ref.fwd_reference(M, N, K, "fused_norm")
    for cols in (48, 64):
        assert (ref.fwd_slots(y, cols) != ref.fwd_slots(y, cols, "slots_swapped")).any(axis=1).all()       # in every row
        assert np.array_equal(ref.fwd_slots(y, cols).sum(1), ref.fwd_slots(y, cols, "slots_swapped").sum(1))   # (the sum cannot see it)
    assert (ref.fwd_slots(y, 48) != ref.fwd_slots(y, 48, "slot48_over_64")).any(axis=1).all()
    # a 192-wide tile's 48-column slots written in 64-column order are 64-column sums: fwd_slots(y, 64) has another shape and other values
    assert not np.array_equal(ref.fwd_slots(y, 48)[:, :12], ref.fwd_slots(y, 64))
    # double rounding through an intermediate of 4 extra bits: every EXACT case with a bf16 output and a fractional addend holds values
    # it rounds elsewhere (the sets without one give integers: bf16 holds the small ones, and a cut to 12 bits leaves the others alone)
    seen = 0
    for M, N, K, ops in FWD_SHAPES:
        if not any(c.out == "bf16" for c in FWD if (c.M, c.N, c.K, c.ops) == (M, N, K, ops)) or ops in ("none", "row_scale"):
            continue
        y, _ = ref.fwd_reference(M, N, K, ops)
        assert (ref.fwd_bf16_bits(y) != ref.fwd_bf16_bits(y, "bf16_rounded_twice", 4)).any(), (M, N, K, ops)
        seen += 1
    assert seen >= 8 * 3
    # 16 extra bits is the f32 itself, and every EXACT result is an f32 value: no such input can see that one
    y, _ = ref.fwd_reference(300, 136, 128, "out_proj")
    assert np.array_equal(ref.fwd_bf16_bits(y), ref.fwd_bf16_bits(y, "bf16_rounded_twice", 16))
