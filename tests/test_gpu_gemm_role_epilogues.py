"""The 8-wave 256-row GEMM kernel compiles its epilogue per encoder role (QKV, FF1, out-proj, FF2: csrc/gemm_common.h, epilogue_role).
For every role, tile width and the shapes at which the kernel takes another path (K = 64: one K-tile, prologue branch; 128: steady loop;
192: the K rotation wraps; M = 300: masked bottom rows; two tile columns):
 (a) the role path equals the generic epilogue on the same tiles (tile_hint 6) BIT FOR BIT on C, c_bf16 and row_sumsq;
 (b) every element is within a derived bound of a float64 product with the same operators;
 (c) two launches on the same inputs are bit-identical;
 (d) a descriptor one operator off the role's set runs the generic epilogue and still computes that operator.

Bound of (b), u = 2^-24 (f32 unit roundoff), S = sum_k |a b| per element, s = row scale:
   accumulation          K u S                     (f32 accumulation of exact bf16 products)
   each f32 operation    u |its result|            (scale, bias add, residual fma)
   FF1                   GELU is 1.13-Lipschitz; gelu_poly2 is within 8.3e-5 of it; the bf16 store rounds by 2^-8 relative (8 significand bits)
   QKV                   the bf16 store rounds by 2^-8 relative (8 significand bits)
row_sumsq is checked against the float64 sum of squares of the f32 output the kernel itself stored: N terms summed in f32, N u sum(x^2)."""

import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0**-24
BF_U = 2.0**-8   # bf16 keeps 8 significand bits: round-to-nearest is within 2^-8 relative
ROLES = ["qkv", "ff1", "out_proj", "ff2"]
GRID = [(hint, M, N, K) for hint, Ns in ((2, (256, 512)), (4, (192, 384))) for M in (256, 300, 512) for N in Ns for K in (64, 128, 192)]


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    """Seeded N(0, 1) operands (shared by the four roles, never modified) and the float64 product / absolute product."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a, b = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g))
    t = {"a": a, "b": b, "bias": torch.randn(N, generator=g), "rs": torch.rand(N, generator=g) + 0.5, "scale": torch.rand(M, generator=g) + 0.5,
         "res": torch.randn(M, N, generator=g), "rbias": torch.randn(M, generator=g)}
    t["base"] = a.double() @ b.double().t()
    t["S"] = a.double().abs() @ b.double().abs().t()
    t["dev"] = {k: (v.cuda().bfloat16() if k in ("a", "b") else v.cuda()) for k, v in t.items() if k not in ("base", "S")}
    return t


def _run(role, hint, M, N, K, *, ldc=None, alpha=1.0, optional=True, off=None):
    """One launch; returns (C, c_bf16, row_sumsq slots, epilogue path).  off = the operator added to / removed from the role's set."""
    from tribe_hip import _lib

    t = _inputs(M, N, K)
    dv = t["dev"]
    ldc = ldc or N
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = dv["a"].data_ptr(), K, dv["b"].data_ptr(), K
    d.alpha, d.tile_hint, d.role = alpha, hint, _lib.ROLE[role]
    res_role = role in ("out_proj", "ff2")
    xb = ssq = None
    if res_role:
        out = torch.zeros(M, ldc, device="cuda")
        out[:, :N] = dv["res"]
        d.C, d.ldc, d.c_dtype = out.data_ptr(), ldc, _lib.F32
        d.res, d.ldres = out.data_ptr(), ldc
        if (role == "ff2") != (off == "bias"):   # FF2 without its bias / out-proj with one
            d.bias, d.bias_mode = dv["bias"].data_ptr(), _lib.BIAS_COL
        if optional:
            d.res_scale = dv["rs"].data_ptr()
            xb = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
            ssq = torch.full((M, N // 32), float("nan"), device="cuda")
            d.c_bf16, d.ld_c_bf16, d.row_sumsq = xb.data_ptr(), N, ssq.data_ptr()
            d.ld_row_sumsq = _lib.lib().tribe_gemm_sumsq_slots(C.byref(d))
            assert d.ld_row_sumsq == N // (48 if hint == 4 or N % 256 else 64)
    else:
        out = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        d.C, d.ldc, d.c_dtype = out.data_ptr(), ldc, _lib.BF16
        if role == "ff1":
            d.act = _lib.ACT_GELU
            if off == "row_bias":
                d.bias, d.bias_mode = dv["rbias"].data_ptr(), _lib.BIAS_ROW
            else:
                d.bias, d.bias_mode = dv["bias"].data_ptr(), _lib.BIAS_COL
        elif off == "bias":
            d.bias, d.bias_mode = dv["bias"].data_ptr(), _lib.BIAS_COL
        if optional:
            d.row_scale = dv["scale"].data_ptr()
    path = _lib.lib().tribe_gemm_epilogue_path(C.byref(d))
    _lib.check(_lib.lib().tribe_gemm_bf16(C.byref(d), torch.cuda.current_stream().cuda_stream), "gemm")
    slots = None if ssq is None else ssq.flatten()[: M * d.ld_row_sumsq].view(M, d.ld_row_sumsq).clone()
    return out[:, :N].contiguous(), xb, slots, path


def _want_and_bound(role, M, N, K, *, alpha=1.0, optional=True, off=None):
    t = _inputs(M, N, K)
    s = t["scale"].double()[:, None] if (optional and role in ("qkv", "ff1")) else 1.0
    y = t["base"] * alpha * s
    bound = K * U * t["S"] * abs(alpha) * s + U * y.abs()
    has_bias = (role in ("ff1", "ff2")) != (off == "bias") and off != "row_bias"
    if has_bias:
        y = y + t["bias"].double()
        bound = bound + U * y.abs()
    if off == "row_bias":
        y = y + t["rbias"].double()[:, None]
        bound = bound + U * y.abs()
    if role == "ff1":
        y = torch.nn.functional.gelu(y)
        bound = 1.13 * bound + 8.3e-5
    if role in ("out_proj", "ff2"):
        y = y + t["res"].double() * (t["rs"].double() if optional else 1.0)
        bound = bound + U * y.abs()
    else:
        bound = bound + BF_U * (y.abs() + bound)
    return y, bound


def _check_against_float64(role, got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    worst = float((err / bound).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("hint,M,N,K", GRID)
@pytest.mark.parametrize("role", ROLES)
def test_role_epilogue_grid(role, hint, M, N, K):
    from tribe_hip import _lib  # noqa: F401

    c, xb, slots, path = _run(role, hint, M, N, K)
    assert path == 1, "the role's own operator set must take the role-compiled epilogue"
    c2, xb2, slots2, _ = _run(role, hint, M, N, K)
    g, xbg, slotsg, pathg = _run(role, 6, M, N, K)
    assert pathg == 0
    # (c) deterministic, (a) bit-identical to the generic epilogue
    assert torch.equal(c, c2) and torch.equal(c.view(torch.int32 if c.dtype == torch.float32 else torch.int16),
                                              g.view(torch.int32 if g.dtype == torch.float32 else torch.int16))
    if xb is not None:
        assert torch.equal(xb, xb2) and torch.equal(xb.view(torch.int16), xbg.view(torch.int16))
        assert torch.equal(slots.view(torch.int32), slots2.view(torch.int32)) and torch.equal(slots.view(torch.int32), slotsg.view(torch.int32))
    # (b) per element against float64
    want, bound = _want_and_bound(role, M, N, K)
    _check_against_float64(role, c, want, bound, f"{role} hint {hint} {M}x{N}x{K}")
    if xb is not None:
        assert torch.equal(xb, c.bfloat16())
        x2 = (c.double().cpu() ** 2).sum(1)
        assert float(((slots.double().cpu().sum(1) - x2).abs() / (N * U * x2)).max()) <= 1.0


@pytest.mark.parametrize("hint,N", [(2, 256), (4, 192)])
@pytest.mark.parametrize("role", ROLES)
def test_role_epilogue_without_optional_operands(role, hint, N):
    """First-layer QKV (no row_scale), last-layer FF2 (no c_bf16 / row_sumsq), no res_scale: still the role path, still bit-identical."""
    M, K = 300, 128
    c, _, _, path = _run(role, hint, M, N, K, optional=False)
    g, _, _, pathg = _run(role, 6, M, N, K, optional=False)
    assert (path, pathg) == (1, 0)
    assert torch.equal(c.view(torch.int32 if c.dtype == torch.float32 else torch.int16), g.view(torch.int32 if g.dtype == torch.float32 else torch.int16))
    want, bound = _want_and_bound(role, M, N, K, optional=False)
    _check_against_float64(role, c, want, bound, f"{role} plain hint {hint}")


OFF_CASES = [("qkv", {"off": "bias"}), ("ff1", {"off": "row_bias"}), ("out_proj", {"off": "bias"}), ("ff2", {"off": "bias"}),
             ("qkv", {"alpha": 0.5}), ("ff1", {"alpha": 0.5}), ("out_proj", {"alpha": 0.5}), ("ff2", {"alpha": 0.5}),
             ("qkv", {"ldc": 258}), ("ff1", {"ldc": 258}), ("out_proj", {"ldc": 258}), ("ff2", {"ldc": 258})]


@pytest.mark.parametrize("role,kw", OFF_CASES, ids=[f"{r}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for r, kw in OFF_CASES])
def test_one_operator_off_runs_generic(role, kw):
    """A bias the role does not have (or lacks), a row bias instead of the column bias, alpha != 1, an ldc the vector stores cannot take:
    the launcher keeps such a descriptor away from the role kernel, and the result carries the operator."""
    M, N, K = 300, 256, 128
    optional = "ldc" not in kw   # (the fused-norm operands themselves insist on aligned rows)
    c, _, _, path = _run(role, 2, M, N, K, optional=optional, **kw)
    g, _, _, pathg = _run(role, 6, M, N, K, optional=optional, **kw)
    assert (path, pathg) == (0, 0)
    assert torch.equal(c.view(torch.int32 if c.dtype == torch.float32 else torch.int16), g.view(torch.int32 if g.dtype == torch.float32 else torch.int16))
    want, bound = _want_and_bound(role, M, N, K, optional=optional, alpha=kw.get("alpha", 1.0), off=kw.get("off"))
    _check_against_float64(role, c, want, bound, f"{role} {kw}")
