"""GPU: the row and column reductions (ScaleNorm / RMSNorm / LayerNorm forward, ScaleNorm backward, row softmax forward and
backward, row log-sum-exp and the InfoNCE logit gradient, MSE, the Pearson statistics, metric and loss) against plain float64
restatements written here, on every form their launchers pick.

Each form is reached by width and layout only: the register-resident templates at the widths they are compiled for, the
generic walks at every other width, the vector and the strided Pearson paths by T % 4 and by the '(b t) v' view.  Every grid
holds a row count that is not a multiple of 4 (a partly empty last workgroup), an all-zero row, a row below the eps clamp,
rows at a large common offset (1e3 + N(0, 1)) and, for scores, an entry 60 above the rest of its row.

Bounds follow from the output precision and the accumulation (u = 2^-24, one f32 rounding):
  * f32 results of f32 reductions: |err| <= 1e-5 x the row's largest reference magnitude.  A chain of k f32 adds errs by at
    most k u of the sum of magnitudes; k <= 80 here, and 1e-5 is ~170 u.  Where the kernel subtracts an f32 row statistic
    from the row (LayerNorm's mean, the projection in the ScaleNorm backward, delta in the softmax backward) the error that
    statistic carries, k u x the sum of magnitudes it was made from, is added, times the factor the output applies to it.
  * bf16 results: within one bf16 ulp of the float64 value (the f32 value is within a few u of it; rounding adds half an ulp),
    plus the same f32 term where the kernel subtracts nearly equal numbers; at least 99 % equal to round-to-nearest(float64).
  * e4m3 results: within one e4m3 step of float8_e4m3fn(bf16(reference) / scale), saturating at +-448.
  * Pearson r and loss scalars (f64 sufficient statistics): <= 2e-6 absolute (per voxel: x V for the 'sum' loss).
  * loss gradients: rtol 1e-4 against float64 autograd, plus the f32 rounding of the means and factors the kernel applies.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tribe_ref  # noqa: E402

U = 2.0**-24          # f32 unit roundoff
EPS64 = 2.0**-52      # f64 machine epsilon (DBL_EPSILON)
ROWS = 37             # 37 % 4 == 1: the last workgroup of four one-row waves has three idle waves


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    return _ops


def _call(name: str, *args) -> None:
    """A C-ABI entry point without an ops wrapper, on the current stream (the calling convention of modeling_utils/autograd.py)."""
    from tribe_hip._lib import check, lib

    check(getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def _p(t):
    return None if t is None else t.data_ptr()


def f32(v: float) -> float:
    """The value a float argument of the C ABI arrives with."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def assert_f32_rows(got, ref, floor=0.0, what=""):
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bound = 1e-5 * ref.abs().amax(dim=-1, keepdim=True) + floor
    err = (got - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} f32 outputs beyond 1e-5 of the row's largest magnitude; "
                           f"first at {tuple(bad.nonzero()[0].tolist())}, worst excess {float((err - bound).max()):.3e}")


def _bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 numbers (8 significant bits) in the binade of |ref|; the sub-normal spacing below the smallest normal."""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref.abs() >= 2.0**-126, torch.ldexp(torch.ones_like(ref), e - 8), torch.full_like(ref, 2.0**-133))


def assert_bf16(got, ref, floor=0.0, what=""):
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bound = _bf16_ulp(ref) + floor
    err = (got - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} bf16 outputs more than one ulp from the float64 value; "
                           f"first at {tuple(bad.nonzero()[0].tolist())}, worst excess {float((err - bound).max()):.3e}")
    same = float((got == ref.to(torch.bfloat16).double()).double().mean())
    assert same >= 0.99, f"{what}: only {same:.4f} of the bf16 outputs equal round-to-nearest of the float64 value"


def assert_zero_bits(t: torch.Tensor, what: str):
    """Pad columns: exactly +0 (the buffers start as NaN, so a pad the kernel skipped shows)."""
    assert t.numel() == 0 or not t.contiguous().view(torch.int16).any(), f"{what}: pad columns are not exactly 0"


def _e4m3_codes(v: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """float8_e4m3fn bytes of clamp(bf16(v) * inv_scale, +-448): what the fused quantiser stores for a norm output v."""
    q = (v.to(torch.bfloat16).float() * np.float32(inv_scale)).clamp(-448, 448)
    return q.to(torch.float8_e4m3fn).view(torch.uint8)


def _e4m3_order(u8: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> integers in the order of their values (adjacent representable values differ by 1, +0 == -0)."""
    c = u8.to(torch.int16)
    mag = c & 0x7F
    return torch.where(c >= 0x80, -mag, mag)


def assert_e4m3(got_u8, ref, inv_scale, floor, what=""):
    got = got_u8.cpu()
    assert not ((got & 0x7F) == 0x7F).any(), f"{what}: NaN code in the output (saturation must stop at +-448)"
    lo = _e4m3_order(_e4m3_codes(ref - floor, inv_scale))
    hi = _e4m3_order(_e4m3_codes(ref + floor, inv_scale))
    g = _e4m3_order(got)
    bad = (g < lo - 1) | (g > hi + 1)
    assert not bad.any(), f"{what}: {int(bad.sum())} e4m3 outputs more than one step from the reference, first at {tuple(bad.nonzero()[0].tolist())}"
    sat = (ref.abs() - floor) * inv_scale > 480           # clearly beyond +-448 (the top step is 32): must be exactly +-448
    assert sat.any(), f"{what}: the inputs do not reach the saturation"
    assert torch.equal(got[sat], _e4m3_codes(ref, inv_scale)[sat]), f"{what}: saturated outputs are not +-448"


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _norm_rows(dim: int, seed: int) -> torch.Tensor:
    """[ROWS, dim] f32: row 0 zero, row 3 far below the eps clamps (1e-9), rows 1-2 at 1e3 + N(0, 1), the rest N(0, 1) at scales
    from 1e-3 to 1e2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, dim, generator=g) * torch.logspace(-3, 2, ROWS)[:, None]
    x[0] = 0
    x[1:3] = 1e3 + torch.randn(2, dim, generator=g)
    x[3] = 1e-9 * torch.randn(dim, generator=g)
    return x


def _scores(R: int, T: int, seed: int) -> torch.Tensor:
    """[R, T] f32 scores 3 N(0, 1) with edge rows where they exist: an entry 60 above the rest on the diagonal of row 0 and in the
    last column of row 4, rows 1-2 at 1e3 + N(0, 1), row 3 all zero."""
    g = torch.Generator().manual_seed(seed)
    s = 3 * torch.randn(R, T, generator=g)
    if R > 1:
        s[1:3] = 1e3 + torch.randn(min(R, 3) - 1, T, generator=g)
    if R > 3:
        s[3] = 0
    s[0, 0] = s[0].max() + 60
    if R > 4:
        s[4, -1] = s[4].max() + 60
    return s


# ------------------------------------------------------------------------------------------------
# ScaleNorm forward: scalenorm_kernel<OUT, NV = 12 / 4 / 3> at 3072 / 1024 / 768, its walk (NV = 0) at every other width
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("dim", [768, 1024, 3072, 4, 260, 1408, 4096])
def test_scalenorm_fwd(ops, dim, legacy, out_dtype):
    x = _norm_rows(dim, seed=dim)
    g = torch.tensor([1.3])
    gs, eps = f32(1.0 if legacy else dim**0.5), f32(1e-5)    # gain_scale 1 (legacy g init dim^-0.5) or sqrt(dim) (x-transformers 2.x)
    y = ops.scalenorm(x.cuda(), g.cuda(), gs, eps, out_dtype)
    x64 = x.double()
    ref = x64 * (g.double() * gs) / x64.norm(dim=-1, keepdim=True).clamp(min=eps)
    # one multiply by an f32 scale made from an f32 sum of squares (no cancellation): no extra term
    (assert_f32_rows if out_dtype == torch.float32 else assert_bf16)(y, ref, what=f"scalenorm dim={dim}")


# ------------------------------------------------------------------------------------------------
# RMSNorm / LayerNorm forward: rowstat_norm_kernel<OUT, LN, NV = 4 / 6 / 8 / 12> for dim <= 1024 / 1536 / 2048 / 3072, else
# its walk (NV = 0).  1028: NV 6 with the last slot filled by lane 0 alone; 3088, 4096: the generic walk
# ------------------------------------------------------------------------------------------------
ROWSTAT_DIMS = [16, 512, 1024, 1028, 1408, 2048, 3072, 3088, 4096]
KINDS = ["rms", "ln", "ln_bias"]


def _rowstat_case(dim: int, kind: str):
    x = _norm_rows(dim, seed=dim + 1)
    g = torch.Generator().manual_seed(dim + 2)
    w = 1.0 + 0.2 * torch.randn(dim, generator=g)
    b = 0.1 * torch.randn(dim, generator=g) if kind == "ln_bias" else None
    eps = f32(1e-5)
    x64 = x.double()
    if kind == "rms":
        mean = torch.zeros(ROWS, 1, dtype=torch.float64)
        rstd = (x64.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    else:
        mean = x64.mean(-1, keepdim=True)
        rstd = ((x64 - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    ref = (x64 - mean) * rstd * w.double()
    if b is not None:
        ref = ref + b.double()
    # LayerNorm subtracts an f32 mean: its sum runs in chains of 3 (inside a float4) + ceil(dim / 256) (per lane) + 6 (across the
    # wave) adds, each off by <= u of the running magnitude, so the mean is off by <= k u mean|x|, and the output by that x rstd |w|
    k = 3 + -(-dim // 256) + 6
    floor = 0.0 if kind == "rms" else k * U * x64.abs().mean(-1, keepdim=True) * rstd * w.abs().max().double()
    return x, w, b, eps, ref, floor


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", ROWSTAT_DIMS)
def test_rmsnorm_layernorm_fwd(ops, dim, kind, out_dtype):
    x, w, b, eps, ref, floor = _rowstat_case(dim, kind)
    if kind == "rms":
        y = ops.rmsnorm(x.cuda(), w.cuda(), eps, out_dtype)
    else:
        y = ops.layernorm(x.cuda(), w.cuda(), None if b is None else b.cuda(), eps, out_dtype)
    (assert_f32_rows if out_dtype == torch.float32 else assert_bf16)(y, ref, floor, what=f"{kind} dim={dim}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [d for d in ROWSTAT_DIMS if d % 16 == 0])   # the e4m3 GEMM's K step
def test_norm_quantize_fp8_fwd(ops, dim, kind):
    x, w, b, eps, ref, floor = _rowstat_case(dim, kind)
    scale = 2.0 / 448                                                       # |y| > 2.14 saturates
    q = ops.norm_quantize_fp8(x.cuda(), w.cuda(), None if b is None else b.cuda(), eps, scale, kind != "rms")
    assert q.shape == (ROWS, dim) and q.dtype == torch.uint8
    assert_e4m3(q, ref, f32(1.0 / scale), floor, what=f"{kind} e4m3 dim={dim}")


# ------------------------------------------------------------------------------------------------
# ScaleNorm backward: scalenorm_bwd_reg_kernel<f32 / bf16, 12 / 3> at 3072 / 768, scalenorm_bwd_kernel at every other width
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dg", [False, True])
@pytest.mark.parametrize("residual", ["none", "dres", "dres_rs"])
@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", [768, 3072, 256, 1000, 1024])
def test_scalenorm_bwd(dim, dy_dtype, residual, with_dg):
    """dx = s / max(|x|, eps) (dy - x <x, dy> / |x|^2) (+ dres * rs), the projection dropped below eps; dg += gs <x, dy> / max(|x|, eps)."""
    from tribe_hip._lib import BF16, F32

    x = _norm_rows(dim, seed=dim + 3)
    g = torch.Generator().manual_seed(dim + 4)
    dy = torch.randn(ROWS, dim, generator=g).to(dy_dtype)
    dres = 2 * torch.randn(ROWS, dim, generator=g) if residual != "none" else None
    rs = 0.5 + torch.rand(dim, generator=g) if residual == "dres_rs" else None
    gain = torch.tensor([1.3])
    gs, eps = f32(dim**0.5), f32(1e-5)
    xd, dyd, gd = x.cuda(), dy.cuda(), gain.cuda()
    dresd, rsd = (None if t is None else t.cuda() for t in (dres, rs))
    dx = torch.full((ROWS, dim), float("nan"), device="cuda")
    dg = torch.full((1,), 0.5, device="cuda") if with_dg else None       # the kernel accumulates into dg
    _call("tribe_scalenorm_bwd", xd.data_ptr(), dyd.data_ptr(), F32 if dy_dtype == torch.float32 else BF16, gd.data_ptr(), gs, eps, ROWS, dim,
          _p(dresd), _p(rsd), dx.data_ptr(), _p(dg))
    x64, dy64 = x.double(), dy.double()
    s = float(gain) * gs
    norm = x64.norm(dim=-1, keepdim=True)
    inv = 1.0 / norm.clamp(min=eps)
    dot = (x64 * dy64).sum(-1, keepdim=True)
    proj = torch.where(norm < eps, torch.zeros_like(dot), dot * inv * inv)
    ref = s * inv * (dy64 - x64 * proj)
    if dres is not None:
        ref = ref + dres.double() * (1.0 if rs is None else rs.double())
    # <x, dy> is an f32 sum in chains of <= ceil(dim / 64) + 9 adds: proj is off by k u sum|x dy| / |x|^2, dx by s / |x| |x_i| times that
    k = -(-dim // 64) + 9
    absdot = (x64 * dy64).abs().sum(-1, keepdim=True)
    floor = s * inv * x64.abs() * (k * U * absdot * inv * inv)
    assert_f32_rows(dx, ref, floor, what=f"scalenorm_bwd dim={dim} dy={dy_dtype} {residual}")
    if with_dg:
        want = 0.5 + float((gs * dot * inv).sum())
        # the same per-row error of <x, dy>, then f32 adds of ROWS terms: 1e-5 of the sum of magnitudes
        tol = 1e-5 * (0.5 + float((gs * absdot * inv).sum()))
        assert abs(float(dg) - want) <= tol, f"dg {float(dg)} vs {want} (tol {tol:.3e})"


# ------------------------------------------------------------------------------------------------
# row softmax forward / backward: *_reg_kernel<1 / 2 / 4 / 8> when T_pad == T in {256, 512, 1024, 2048}, the generic walk otherwise
# (768: T % 256 == 0 but no compiled instance) and whenever T_pad > T (zero-filled pad columns)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,T_pad", [(t, t) for t in (256, 512, 1024, 2048, 70, 298, 768, 3000)] + [(70, 128), (256, 320), (298, 320)])
def test_softmax_fwd_bwd(T, T_pad):
    R = ROWS
    S = _scores(R, T, seed=T + T_pad)
    Sd = S.cuda()
    P = torch.full((R, T_pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    _call("tribe_softmax_fwd", Sd.data_ptr(), R, T, T, P.data_ptr(), T_pad, T_pad)
    Pc = P.cpu()
    # exp of arguments <= 0 (shifted by the row max) and one division: no cancellation, no extra term
    assert_bf16(Pc[:, :T], torch.softmax(S.double(), dim=-1), what=f"softmax T={T}")
    assert_zero_bits(Pc[:, T:], "softmax P")
    # backward with that P: dS = scale P (dP - sum_j P_j dP_j); the pad columns of dP must not be read, those of dS are written 0
    g = torch.Generator().manual_seed(T + 7)
    dP = torch.full((R, T_pad), float("nan"))
    dP[:, :T] = torch.randn(R, T, generator=g)
    dS = torch.full((R, T_pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    scale = 0.125
    dPd = dP.cuda()
    _call("tribe_softmax_bwd", P.data_ptr(), dPd.data_ptr(), R, T, T_pad, T_pad, T_pad, scale, dS.data_ptr(), T_pad)
    P64, dP64 = Pc[:, :T].double(), dP[:, :T].double()
    pd = P64 * dP64
    delta = pd.sum(-1, keepdim=True)
    ref = scale * P64 * (dP64 - delta)
    # delta is an f32 sum in chains of <= ceil(T / 64) + 8 adds; dP - delta cancels where P is one-hot (the +60 rows)
    k = -(-T // 64) + 8
    floor = scale * P64 * (k * U * pd.abs().sum(-1, keepdim=True) + U * (dP64.abs() + delta.abs()))
    dSc = dS.cpu()
    assert_bf16(dSc[:, :T], ref, floor, what=f"softmax_bwd T={T}")
    assert_zero_bits(dSc[:, T:], "softmax dS")


# ------------------------------------------------------------------------------------------------
# row log-sum-exp (one wave per row) and the InfoNCE logit gradient (one workgroup per row, zero-filled to N_pad)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 150, 1000, 4097])
def test_lse_rows_and_infonce_dlogits(N):
    S = _scores(N, N, seed=N + 11)
    S64 = S.double()
    Sd = S.cuda()
    lse_r, diag, lse_c = (torch.full((N,), float("nan"), device="cuda") for _ in range(3))
    _call("tribe_lse_rows_fwd", Sd.data_ptr(), N, N, lse_r.data_ptr(), diag.data_ptr())
    St = S.t().contiguous().cuda()                                        # column LSE = row LSE of S^T, as InfoNCE computes it
    _call("tribe_lse_rows_fwd", St.data_ptr(), N, N, lse_c.data_ptr(), None)
    # lse = m + log sum exp(s - m): every rounding is relative to |s| or to lse, so 1e-5 of the larger of the two
    for got, ref, rowmax in ((lse_r, torch.logsumexp(S64, 1), S64.abs().amax(1)), (lse_c, torch.logsumexp(S64, 0), S64.abs().amax(0))):
        err = (got.cpu().double() - ref).abs()
        assert (err <= 1e-5 * torch.maximum(ref.abs(), rowmax)).all(), f"lse N={N}: worst {float(err.max()):.3e}"
    assert torch.equal(diag.cpu(), S.diagonal())
    # dL = k (exp(s - lse_r) + exp(s - lse_c) - 2 [i == j]), k = gs / (2 N): the kernel alone, fed the float64 LSEs rounded to f32
    lr, lc = torch.logsumexp(S64, 1).float(), torch.logsumexp(S64, 0).float()
    gs = torch.tensor([f32(1.0 / 0.07)])
    N_pad = -(-N // 64) * 64
    assert N_pad > N
    dL = torch.full((N, N_pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    lrd, lcd, gsd = lr.cuda(), lc.cuda(), gs.cuda()
    _call("tribe_infonce_dlogits", Sd.data_ptr(), N, N, lrd.data_ptr(), lcd.data_ptr(), gsd.data_ptr(), dL.data_ptr(), N_pad)
    k = float(gs) * 0.5 / N
    ar, ac = S64 - lr.double()[:, None], S64 - lc.double()[None, :]
    pr, pc = ar.exp(), ac.exp()
    eye = torch.eye(N, dtype=torch.float64)
    ref = k * (pr + pc - 2 * eye)
    # exp of an f32 argument a errs by <= (2|a| + 3) u relative; the three-term sum cancels on the diagonal where p -> 1
    floor = k * U * (pr * (2 * ar.abs() + 6) + pc * (2 * ac.abs() + 6) + 4 * eye)
    dLc = dL.cpu()
    assert_bf16(dLc[:, :N], ref, floor, what=f"infonce dlogits N={N}")
    assert_zero_bits(dLc[:, N:], "infonce dlogits")


# ------------------------------------------------------------------------------------------------
# tribe_mse_fwd / tribe_mse_bwd, the (MSE, mean) instance of csrc/robust_loss.hip's element-wise family: forward (2048-workgroup
# capped grid, 4-deep float4 loop, float4 remainder, scalar tail for n % 4) and backward (4096-workgroup grid, 2-deep loop); the last
# n runs the forward's unrolled loop three times over (4 x 4 x 2048 x 256 floats per trip)
# ------------------------------------------------------------------------------------------------
def _mse_fwd(pd, td, n):
    """tribe_mse_fwd's return code and result on a workspace of tribe_mse_workspace_bytes(n)."""
    from tribe_hip._lib import lib

    ws = torch.empty(lib().tribe_mse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    out = torch.full((), float("nan"), device="cuda")
    rc = lib().tribe_mse_fwd(pd.data_ptr(), td.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return rc, out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097, 16_500, 64 * 1000 * 100, 3 * (4 * 4 * 2048 * 256) + 4 * 300_001 + 3])
def test_mse_fwd_bwd(ops, n):
    from tribe_hip._lib import check, lib

    g = torch.Generator().manual_seed(n % 100_003)
    pred = torch.randn(n, generator=g)
    true = torch.randn(n, generator=g).mul_(0.8).add_(pred, alpha=0.5)
    true[3::7] = pred[3::7]                                               # exact zeros of the gradient
    pd, td = pred.cuda(), true.cuda()
    assert lib().tribe_mse_workspace_bytes(n) == lib().tribe_elem_loss_workspace_bytes(n)
    rc, out = _mse_fwd(pd, td, n)
    check(rc, "tribe_mse_fwd")
    got = float(out)
    p64 = pred.double().requires_grad_()
    loss = (p64 - true.double()).pow(2).mean()
    # f32 squares summed in f32 chains of <= 16 terms, then in f64: 1e-5 relative
    assert abs(got - float(loss)) <= 1e-5 * float(loss), f"mse n={n}: {got} vs {float(loss)}"
    gs = 0.75
    (grad,) = torch.autograd.grad(loss, p64, torch.tensor(gs, dtype=torch.float64))
    dp = torch.full((n,), float("nan"), device="cuda")
    gsd = torch.tensor([gs], device="cuda")
    _call("tribe_mse_bwd", pd.data_ptr(), td.data_ptr(), n, gsd.data_ptr(), dp.data_ptr())
    torch.testing.assert_close(dp.cpu().double(), grad, rtol=1e-4, atol=0)
    if n in (5, 4097, 16_500):
        # the partly filled workgroup, the unrolled loop plus tail, the remainder loop: the wrappers run the family's kernels with the
        # family's (mse, mean) plan, so a single differing bit means a wrapper passes another factor
        same = ops.elem_loss(pd, td, "mse", 0.0, "mean")
        assert torch.equal(out.view(torch.int32), same.view(torch.int32)), f"mse n={n}: {got} vs elem_loss {float(same)}"
        dq = torch.full((n,), float("nan"), device="cuda")
        _call("tribe_elem_loss_bwd", pd.data_ptr(), td.data_ptr(), n, ops.ELEM_LOSS_KINDS["mse"], 0.0, ops.ELEM_LOSS_REDUCTIONS["mean"],
              gsd.data_ptr(), dq.data_ptr())
        assert torch.equal(dp.view(torch.int32), dq.view(torch.int32)), f"mse n={n}: tribe_mse_bwd and tribe_elem_loss_bwd differ in bits"
    if n == 4097:
        # the entry point's own contract: 16-byte aligned inputs (the family's entry point takes the scalar form there)
        buf = torch.zeros(n + 1, device="cuda")
        assert buf.data_ptr() % 16 == 0
        with pytest.raises(ValueError, match="tribe_mse_fwd: inputs must be 16-byte aligned"):
            check(_mse_fwd(buf[1:], td, n)[0], "tribe_mse_fwd")


# ------------------------------------------------------------------------------------------------
# Pearson statistics, metric and loss
# ------------------------------------------------------------------------------------------------
PB = [1, 5, 16, 64, 67]
PV = [33, 1000, 4097]
# rows: [B, V, 100] contiguous -> bvt_stats_rows_kernel<PearsonAcc> (+ the float4 loss backward);  t99: [B, V, 99] contiguous and
# nv: the '(b t) v' matrix viewed as [B, V, 100] (strides (100 V, 1, V)) -> bvt_stats_strided_kernel<PearsonAcc> (+ the scalar backward)
LAYOUTS = ["rows", "t99", "nv"]
G = 4                 # metric groups: rows go to 0 .. G - 2; group G - 1 receives none (n = 0 < 2)


def _pearson_data(B: int, V: int, T: int, seed: int):
    """pred / true [B, V, T] f32.  Edge columns: v0 constant prediction 1.7, v1 constant target -3.3, v2 1e3 + N(0, 1) on both sides
    (the one-pass sums), v3 true = 2 pred + 3 (r = 1 up to the f32 rounding of true: must stay <= 1), v4 true = -pred (r = -1);
    the others true = 0.5 pred + noise, the prediction scale varying across voxels."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, V, T, generator=g) * torch.logspace(-1, 1, V)[None, :, None]
    true = 0.5 * pred + torch.randn(B, V, T, generator=g)
    pred[:, 0] = 1.7
    true[:, 1] = -3.3
    pred[:, 2] = 1e3 + torch.randn(B, T, generator=g)
    true[:, 2] = 1e3 + 0.5 * (pred[:, 2] - 1e3) + torch.randn(B, T, generator=g)
    true[:, 3] = 2 * pred[:, 3] + 3
    true[:, 4] = -pred[:, 4]
    return pred, true


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


def _pearson_ref(pred: torch.Tensor, true: torch.Tensor, gid: torch.Tensor):
    """float64 per (group, voxel): r from centred sums (NaN for n < 2 and for a constant column, as scipy.stats.pearsonr gives),
    the six sufficient statistics, and the sums of the magnitudes behind them."""
    V = pred.shape[1]
    r = torch.full((G, V), float("nan"), dtype=torch.float64)
    stats = torch.zeros(G, V, 6, dtype=torch.float64)
    mags = torch.zeros(G, V, 5, dtype=torch.float64)
    for grp in range(G):
        sel = gid == grp
        if not sel.any():
            continue
        x, y = tribe_ref.flatten_bt(pred[sel]).double(), tribe_ref.flatten_bt(true[sel]).double()
        n = x.shape[0]
        stats[grp] = torch.stack([x.sum(0), y.sum(0), (x * x).sum(0), (y * y).sum(0), (x * y).sum(0),
                                  torch.full((V,), float(n), dtype=torch.float64)], -1)
        mags[grp] = torch.stack([x.abs().sum(0), y.abs().sum(0), (x * x).sum(0), (y * y).sum(0), (x * y).abs().sum(0)], -1)
        if n >= 2:
            xc, yc = x - x.mean(0), y - y.mean(0)
            r[grp] = (xc * yc).sum(0) / ((xc * xc).sum(0) * (yc * yc).sum(0)).sqrt()
    return r, stats, mags


def _assert_r(got: torch.Tensor, want: torch.Tensor, what: str):
    got = got.cpu().double()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (f"{what}: NaN pattern differs (constant column or n < 2 must give NaN, nothing else): "
                                                f"kernel NaN at {torch.isnan(got).nonzero().tolist()[:8]}, reference at {nan.nonzero().tolist()[:8]}")
    # f64 statistics, one f32 rounding of r: 2e-6 absolute
    err = (got[~nan] - want[~nan]).abs()
    assert err.numel() == 0 or float(err.max()) <= 2e-6, f"{what}: |r error| {float(err.max()):.3e}"
    assert err.numel() == 0 or float(got[~nan].abs().max()) <= 1.0, f"{what}: |r| > 1"


def _check_stats_and_r(ops, B: int, V: int, T: int, layout: str, seed: int):
    pred, true = _pearson_data(B, V, T, seed)
    gid = _groups(B)
    stats = torch.zeros(G, V, 6, dtype=torch.float64, device="cuda")
    for b0, b1 in _pieces(B):
        ops.pearson_stats_update(stats, _device_view(pred[b0:b1], layout), _device_view(true[b0:b1], layout), gid[b0:b1].cuda())
    want_r, want_stats, mags = _pearson_ref(pred, true, gid)
    got_stats = stats.cpu()
    assert torch.equal(got_stats[..., 5], want_stats[..., 5]), "sample counts differ (a row dropped, repeated or put in the wrong group)"
    # f64 sums of f32 values and exact f32 products, here and in the reference: n adds at most, each off by <= 2^-53 of the running
    # magnitude, on either side
    n = want_stats[..., 5:6].clamp(min=1)
    err = (got_stats[..., :5] - want_stats[..., :5]).abs()
    assert (err <= n * EPS64 * mags).all(), f"sufficient statistics off by up to {float((err / mags.clamp(min=1e-300)).max()):.3e} relative"
    _assert_r(ops.pearson_from_stats(stats), want_r, f"B={B} V={V} T={T} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V", PV)
@pytest.mark.parametrize("B", PB)
def test_pearson_stats_and_r(ops, B, V, layout):
    _check_stats_and_r(ops, B, V, 99 if layout == "t99" else 100, layout, seed=B * 7919 + V)


@pytest.mark.parametrize("B,V,T", [(5, 33, 1028), (9, 1000, 2000)])
def test_pearson_stats_rows_long(ops, B, V, T):
    """T > 768: the rows kernel's four-deep float4 loop (i + 192 < T / 4) runs before its remainder loop."""
    _check_stats_and_r(ops, B, V, T, "rows", seed=T)


def test_pearson_constant_columns_at_validation_length(ops):
    """A constant column gives NaN (scipy.stats.pearsonr's answer) however many samples the state holds.  At ~1e5 samples the one-pass
    variance Sxx - Sx^2 / n of a constant column is f64 rounding noise of either sign, so r would be noise over noise; a variance
    within n ulps of Sxx counts as 0.  A near-constant column four times above that threshold keeps a finite r."""
    B, T = 1024, 100                                                    # n = 102 400 samples per voxel, one group, four updates
    consts = [1.7, 123.456, 0.1, -3.3, 1000.37, 17.9, 2.2e-3, 5.5, -77.7, 0.3]
    nc = len(consts)
    V = 2 * nc + 2
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(B, V, T, generator=g)
    true = 0.5 * pred + torch.randn(B, V, T, generator=g)
    for i, c in enumerate(consts):
        pred[:, i] = c
        true[:, nc + i] = c
    n = B * T
    vn = 2 * nc                                                          # near-constant prediction: 1.7 +- delta
    sign = torch.where(torch.rand(B, T, generator=g) < 0.5, -1.0, 1.0)
    pred[:, vn] = 1.7 + 2 * 1.7 * math.sqrt(n * EPS64) * sign
    true[:, vn] = sign + 0.5 * torch.randn(B, T, generator=g)
    want, st_ref, _ = _pearson_ref(pred, true, torch.zeros(B, dtype=torch.long))
    want = want[0]
    assert torch.isnan(want[: 2 * nc]).all()
    s = [float(v) for v in st_ref[0, vn]]
    vx, vy = s[2] - s[0] ** 2 / n, s[3] - s[1] ** 2 / n
    assert 3 * n * EPS64 * s[2] < vx < 5 * n * EPS64 * s[2]            # the column sits ~4x above the threshold
    for layout in ("rows", "nv"):
        stats = torch.zeros(1, V, 6, dtype=torch.float64, device="cuda")
        for b0 in range(0, B, B // 4):
            b1 = b0 + B // 4
            ops.pearson_stats_update(stats, _device_view(pred[b0:b1], layout), _device_view(true[b0:b1], layout), None)
        r = ops.pearson_from_stats(stats).cpu().double()[0]
        bad = [consts[i % nc] for i in range(2 * nc) if not math.isnan(float(r[i]))]
        assert not bad, f"{layout}: constant columns of {bad} gave a finite r: {r[: 2 * nc].tolist()}"
        # near-constant column: finite, and off by at most what the worst-case error n eps Sxx of vx allows (half of it, relative),
        # plus the error of cov (n eps sqrt(Sxx Syy) over sqrt(vx vy))
        assert math.isfinite(float(r[vn])), f"{layout}: the near-constant column lost its r"
        tol = abs(float(want[vn])) * 0.5 * n * EPS64 * s[2] / vx + n * EPS64 * math.sqrt(s[2] * s[3] / (vx * vy)) + 2e-6
        assert abs(float(r[vn]) - float(want[vn])) <= tol, f"{layout}: near-constant r {float(r[vn])} vs {float(want[vn])}"
        _assert_r(r[vn + 1:], want[vn + 1:], f"{layout} ordinary column")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V", PV)
@pytest.mark.parametrize("B", PB)
def test_pearson_loss_fwd_bwd(B, V, layout):
    """PearsonLoss forward (mean and sum) and backward against float64 autograd of oracle.tribe_ref.pearson_loss.

    Known divergence: for a constant prediction column (v0) float64 autograd of the reference gives NaN (the derivative of sqrt at 0
    is infinite and multiplies 0); the kernel returns the finite term -k / den * (y - mean y) alone (den = 0 * sy + 1e-8), and that
    column is compared with this float64 formula instead."""
    from modeling_utils.losses import PearsonLoss

    T = 99 if layout == "t99" else 100
    pred, true = _pearson_data(B, V, T, seed=B * 104729 + V)
    x64 = tribe_ref.flatten_bt(pred).double().requires_grad_()
    y64 = tribe_ref.flatten_bt(true).double()
    # per-voxel factors of the gradient d(1 - r_v)/dx = -a (y - my) + c (x - mx), from centred float64 sums
    xc, yc = x64.detach() - x64.detach().mean(0), y64 - y64.mean(0)
    sx, sy = (xc * xc).sum(0).sqrt(), (yc * yc).sum(0).sqrt()
    cov = (xc * yc).sum(0)
    den = sx * sy + 1e-8
    for reduction in ("mean", "sum"):
        want = tribe_ref.pearson_loss(x64, y64, reduction)
        (grad,) = torch.autograd.grad(want, x64)
        k = 1.0 / V if reduction == "mean" else 1.0
        assert torch.isnan(grad[:, 0]).all() and not torch.isnan(grad[:, 1:]).any()
        grad[:, 0] = -k / den[0] * yc[:, 0]                               # the finite term the kernel keeps (see the docstring)
        if layout == "nv":
            pg = tribe_ref.flatten_bt(pred).contiguous().cuda().requires_grad_()
            got = PearsonLoss(reduction)(pg, tribe_ref.flatten_bt(true).contiguous().cuda())
        else:
            pg = pred.cuda().requires_grad_()
            got = PearsonLoss(reduction).forward_bvt(pg, true.cuda())
        got.backward()
        # f64 statistics, per-voxel f32 rounding of the square roots, the eps add and the quotient: 2e-6 per voxel (x V when summed)
        tol = 2e-6 * (1 if reduction == "mean" else V)
        assert abs(float(got.detach()) - float(want.detach())) <= tol, f"{reduction}: loss {float(got.detach())} vs {float(want.detach())}"
        gk = pg.grad.cpu().double()
        if layout != "nv":
            gk = tribe_ref.flatten_bt(gk)
        # the kernel forms -a (y - my) + c (x - mx) from f32 means and f32 factors a, c: a dozen roundings, each <= u of |a| max|y| or
        # |c| max|x|, on top of rtol 1e-4
        a = k / den
        c = torch.where(sx > 0, k * cov * sy / (sx * den * den), torch.zeros_like(sx))
        floor = 24 * U * (a.abs() * y64.abs().amax(0) + c.abs() * x64.detach().abs().amax(0))
        err = (gk - grad).abs()
        bad = err > 1e-4 * grad.abs() + floor
        first = tuple(bad.nonzero()[0].tolist()) if bad.any() else None
        assert not bad.any(), f"{reduction}: {int(bad.sum())} gradient entries off, first at {first}: {float(gk[first])} vs {float(grad[first])}"
