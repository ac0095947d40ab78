"""The encoder's f32 residual stream as two 16-bit planes (include/tribe_hip.h, enum tribe_c_planes; csrc/gemm_common.h):
hi = bf16(x) rounded to nearest even, lo = the low half of the f32 word, decoded as ((hi - (lo > 0x8000)) << 16) | lo.  Lossless but for the
exact tie that rounded UP (lo == 0x8000 under an odd top half), stored as lo = 0x8001: that element comes back as x + 1 ulp.

 codec     every low half under a handful of high halves through the stand-alone kernels;
 epilogue  the three plane variants of the out-proj / FF2 role kernels against the f32 launch on the same operands: hi and row_sumsq bit-equal,
           the decoded stream bit-equal except at tie-ups (+1 ulp exactly), rows past M and the unused half of every strip untouched; the
           f32 -> planes and planes -> f32 launches also in place on one f32 buffer, as the encoder runs them; ties forced with A = 0;
 encoder   tribe_encoder_fwd with the planes switched on against off in one process, depth 3 and depth 1.

Bound of the encoder comparison.  hi is never altered, so QKV / FF1 see the same operands until a +1 ulp in the stream moves a later sum
across a rounding boundary.  tests/test_residual_planes_host.py restates the stream of THESE inputs on the CPU (NumPy bit operations for
the stream, f32 torch for the branches), once with and once without the tie rule, and measures the relative L2 difference: depth 3 (8
tie-ups in 768 k stored words) 9.3e-10 in x and 1.0e-9 in y; depth 1 (3 tie-ups) 4.4e-10 in x and 5.7e-9 in y, where the + 1 ulp moved one
row's final ScaleNorm factor.  REL_L2_MEASURED = the larger per depth (1.03e-9, 5.71e-9), REL_L2_BOUND = an order of magnitude over it
(1.03e-8, 5.71e-8); at most 1 % of the y elements may differ at all."""

import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_residual_planes_host import B, REL_L2_BOUND, REL_L2_MEASURED, T, encoder_input, make_encoder  # noqa: E402

MAX_DIFFERING_Y = 0.01      # fraction of y elements that may differ at all


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def _u16(x: torch.Tensor) -> torch.Tensor:
    """int16 plane -> its 16 bits as a non-negative int32"""
    return x.to(torch.int32) & 0xFFFF


def _is_tie_up(bits: torch.Tensor) -> torch.Tensor:
    return (bits & 0x1FFFF) == 0x18000


# ---- codec -----------------------------------------------------------------------------------------------------------------------------
# high halves: even / odd significand, both signs, +-0, denormals (smallest, largest), smallest normal, the largest finite top half
# (odd: its tie rounds up to the bf16 infinity), +-inf (NaN for every lo != 0), quiet and all-ones NaN
HIGH_HALVES = [0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4049, 0xC2F6, 0x0000, 0x8000, 0x0001, 0x007F, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x7F7E,
               0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FFF]


def test_codec_every_low_half():
    from tribe_hip import ops

    lo_all = torch.arange(65536, dtype=torch.int64)
    words = torch.cat([(h << 16) | lo_all for h in HIGH_HALVES])
    words = torch.where(words >= 2**31, words - 2**32, words).to(torch.int32).cuda()
    x = words.view(torch.float32)
    hi, lo = ops.f32_to_planes(x)
    back = _bits(ops.planes_to_f32(hi, lo))
    nan = torch.isnan(x)
    tie = _is_tie_up(words) & ~nan
    assert int(tie.sum()) == sum(1 for h in HIGH_HALVES if h & 1 and (h & 0x7F80) != 0x7F80), "one tie-up per odd finite high half"
    # hi is today's f32_to_bf16 (v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN) on every input
    want_hi = x.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(hi[~nan], want_hi[~nan])
    assert bool(torch.isnan(hi[nan].view(torch.bfloat16).float()).all())
    # lossless, except the documented tie-ups: exactly + 1 ulp (the next bit pattern), stored as lo = 0x8001
    plain = ~nan & ~tie
    assert torch.equal(back[plain], words[plain])
    assert torch.equal(back[tie], words[tie] + 1) and bool((_u16(lo[tie]) == 0x8001).all())
    assert torch.equal(_u16(lo[plain]), words[plain] & 0xFFFF)
    # a NaN comes back a NaN, an infinity the same infinity (they are in `plain`: checked bit for bit above; named here for the reader)
    assert bool(torch.isnan(back[nan].view(torch.float32)).all())
    inf = torch.isinf(x)
    assert int(inf.sum()) == 2 and torch.equal(back[inf], words[inf])


def test_codec_random_words():
    from tribe_hip import ops

    g = torch.Generator().manual_seed(5)
    words = torch.randint(-2**31, 2**31 - 1, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    x = words.view(torch.float32)
    ok = ~torch.isnan(x)
    hi, lo = ops.f32_to_planes(x)
    back = _bits(ops.planes_to_f32(hi, lo))
    assert torch.equal(hi[ok], x.to(torch.bfloat16).view(torch.int16)[ok])
    assert torch.equal(back[ok], (words + _is_tie_up(words).to(torch.int32))[ok])


# ---- the role epilogues ------------------------------------------------------------------------------------------------------------------
K = 128
GUARD = 64   # rows behind M that no launch may touch


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _operands(M, N):
    g = torch.Generator().manual_seed(7000 + 10 * M + N)
    t = {"a": bf(torch.randn(M, K, generator=g)).cuda().bfloat16(), "b": bf(torch.randn(N, K, generator=g)).cuda().bfloat16(),
         "bias": torch.randn(N, generator=g).cuda(), "rs": (torch.rand(N, generator=g) + 0.5).cuda(), "res": torch.randn(M, N, generator=g).cuda()}
    t["zero_a"], t["zero_bias"] = torch.zeros_like(t["a"]), torch.zeros_like(t["bias"])
    return t


def _launch(role, M, N, t, *, c_dtype, res, C_buf, hi_buf, rs, a="a", bias="bias", want_ssq=True):
    """One tribe_gemm_bf16 launch on the 256 x 256 role kernel (tile_hint 2).  Returns the row_sumsq slots (or None)."""
    from tribe_hip import _lib

    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = t[a].data_ptr(), K, t["b"].data_ptr(), K
    d.alpha, d.tile_hint, d.role = 1.0, 2, _lib.ROLE[role]
    # a lo row is 2 N 16-bit slots wide (see _lo_buf); an f32 row N words
    lo_out, lo_in = c_dtype in (_lib.F32_PLANES_OUT, _lib.F32_PLANES_INOUT), c_dtype in (_lib.F32_PLANES_INOUT, _lib.F32_PLANES_IN)
    d.C, d.ldc, d.c_dtype = C_buf.data_ptr(), 2 * N if lo_out else N, c_dtype
    d.res, d.ldres = res.data_ptr(), 2 * N if lo_in else N
    if role == "ff2":
        d.bias, d.bias_mode = t[bias].data_ptr(), _lib.BIAS_COL
    if rs:
        d.res_scale = t["rs"].data_ptr()
    ssq = None
    if hi_buf is not None:
        d.c_bf16, d.ld_c_bf16 = hi_buf.data_ptr(), N
    if want_ssq:
        ssq = torch.full((M + GUARD, N // 64), float("nan"), device="cuda")
        d.row_sumsq, d.ld_row_sumsq = ssq.data_ptr(), N // 64
        assert _lib.lib().tribe_gemm_sumsq_slots(C.byref(d)) == N // 64
    assert _lib.lib().tribe_gemm_epilogue_path(C.byref(d)) == 1
    _lib.check(_lib.lib().tribe_gemm_bf16(C.byref(d), torch.cuda.current_stream().cuda_stream), "gemm")
    return ssq


def _guarded(M, N, dtype, fill):
    return torch.full((M + GUARD, N), fill, dtype=dtype, device="cuda")


def _lo_buf(M, N):
    """A lo plane as the epilogues lay it out: column c of a row at 16-bit slot 2 (c & ~63) + (c & 63) of 2 N -- the first 128 bytes of the
    256 that the f32 words of a 64-column strip take, so that the plane can live inside the f32 buffer it stands for."""
    return torch.full((M + GUARD, 2 * N), 0x4321, dtype=torch.int16, device="cuda")


def _lo_get(raw):
    """the plane, compact [rows, N]"""
    return raw.view(raw.shape[0], -1, 2, 64)[:, :, 0, :].reshape(raw.shape[0], -1)


def _lo_set(raw, M, values):
    raw.view(raw.shape[0], -1, 2, 64)[:M, :, 0, :] = values.view(M, -1, 64) if isinstance(values, torch.Tensor) else values


def _lo_gaps_untouched(raw):
    return bool((raw.view(raw.shape[0], -1, 2, 64)[:, :, 1, :] == 0x4321).all())


def _f32_mode(role, M, N, t, res, rs, **kw):
    """today's launch: f32 stream in place + bf16 copy + row_sumsq"""
    x = _guarded(M, N, torch.float32, -7.0)
    x[:M] = res
    hi = _guarded(M, N, torch.int16, 0x1234)
    ssq = _launch(role, M, N, t, c_dtype=0, res=x, C_buf=x, hi_buf=hi, rs=rs, **kw)
    return x, hi, ssq


def _check_planes(M, x, hi, ssq, got_hi, got_lo, got_ssq):
    from tribe_hip import ops

    assert torch.equal(got_hi[:M], hi[:M]), "hi must be the f32 mode's c_bf16 bit for bit"
    assert torch.equal(_bits(got_ssq[:M]), _bits(ssq[:M])), "row_sumsq comes from the f32 value before the split"
    xb = _bits(x[:M])
    tie = _is_tie_up(xb)
    lo = _lo_get(got_lo)
    back = _bits(ops.planes_to_f32(got_hi[:M].contiguous(), lo[:M].contiguous()))
    assert torch.equal(back, xb + tie.to(torch.int32)), "the decoded stream: bit-equal, tie-ups exactly + 1 ulp"
    assert bool((_u16(lo[:M][tie]) == 0x8001).all())
    # rows past M: neither plane nor the slots were touched
    assert bool((got_hi[M:] == 0x1234).all()) and bool((lo[M:] == 0x4321).all()) and bool(torch.isnan(got_ssq[M:]).all())
    return int(tie.sum())


@pytest.mark.parametrize("rs", [False, True], ids=["plain", "res_scale"])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [256, 300])
@pytest.mark.parametrize("role", ["out_proj", "ff2"])
def test_plane_epilogues_match_the_f32_mode(role, M, N, rs):
    from tribe_hip import _lib, ops

    t = _operands(M, N)
    # ---- f32 -> planes (layer-0 out-proj) ----
    x, hi, ssq = _f32_mode(role, M, N, t, t["res"], rs)
    got_hi, got_lo = _guarded(M, N, torch.int16, 0x1234), _lo_buf(M, N)
    res_in = _guarded(M, N, torch.float32, -7.0)
    res_in[:M] = t["res"]
    got_ssq = _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_OUT, res=res_in, C_buf=got_lo, hi_buf=got_hi, rs=rs)
    _check_planes(M, x, hi, ssq, got_hi, got_lo, got_ssq)
    assert _lo_gaps_untouched(got_lo)
    assert torch.equal(res_in[:M], t["res"]) and bool((res_in[M:] == -7.0).all()), "the f32 residual is read only"
    # the same IN PLACE, as the encoder runs it: the lo plane goes into the f32 buffer it was read from (x viewed as 16-bit slots) ...
    xin = _guarded(M, N, torch.float32, -7.0)
    xin[:M] = t["res"]
    got_hi2 = _guarded(M, N, torch.int16, 0x1234)
    got_ssq2 = _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_OUT, res=xin, C_buf=xin.view(torch.int16), hi_buf=got_hi2, rs=rs)
    assert torch.equal(got_hi2, got_hi) and torch.equal(_lo_get(xin.view(torch.int16))[:M], _lo_get(got_lo)[:M])
    assert torch.equal(_bits(got_ssq2[:M]), _bits(ssq[:M])) and bool((xin[M:] == -7.0).all())
    # ... and back to f32 in the same buffer, with A = 0 and no bias / scale: x comes back, + 1 ulp at the tie-ups
    if not rs:
        _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_IN, res=xin.view(torch.int16), C_buf=xin, hi_buf=got_hi2, rs=False, a="zero_a", bias="zero_bias",
                want_ssq=False)
        assert torch.equal(_bits(xin[:M]), _bits(x[:M]) + _is_tie_up(_bits(x[:M])).to(torch.int32)) and bool((xin[M:] == -7.0).all())
    # ---- planes -> planes, in place (middle launches): the residual is what the planes hold ----
    in_hi, in_lo = ops.f32_to_planes(t["res"])
    res_dec = ops.planes_to_f32(in_hi, in_lo)
    x, hi, ssq = _f32_mode(role, M, N, t, res_dec, rs)
    got_hi, got_lo = _guarded(M, N, torch.int16, 0x1234), _lo_buf(M, N)
    got_hi[:M] = in_hi
    _lo_set(got_lo, M, in_lo)
    got_ssq = _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_INOUT, res=got_lo, C_buf=got_lo, hi_buf=got_hi, rs=rs)
    _check_planes(M, x, hi, ssq, got_hi, got_lo, got_ssq)
    # ---- planes -> f32 (last FF2): no tie rule on the way out, the hi plane is read only ----
    got_hi, got_lo = _guarded(M, N, torch.int16, 0x1234), _lo_buf(M, N)
    got_hi[:M] = in_hi
    _lo_set(got_lo, M, in_lo)
    out = _guarded(M, N, torch.float32, -7.0)
    got_ssq = _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_IN, res=got_lo, C_buf=out, hi_buf=got_hi, rs=rs)
    assert torch.equal(_bits(out[:M]), _bits(x[:M])) and bool((out[M:] == -7.0).all())
    assert torch.equal(_bits(got_ssq[:M]), _bits(ssq[:M])) and bool(torch.isnan(got_ssq[M:]).all())
    assert torch.equal(got_hi[:M], in_hi) and torch.equal(_lo_get(got_lo)[:M], in_lo) and bool((got_hi[M:] == 0x1234).all())
    # and without the optional slots (the encoder's last FF2 asks for none)
    out2 = _guarded(M, N, torch.float32, -7.0)
    _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_IN, res=got_lo, C_buf=out2, hi_buf=got_hi, rs=rs, want_ssq=False)
    assert torch.equal(_bits(out2), _bits(out))


@pytest.mark.parametrize("M", [256, 300])
@pytest.mark.parametrize("role", ["out_proj", "ff2"])
def test_forced_ties(role, M):
    """A = 0 (and a zero FF2 bias, no res_scale): the output is the residual itself.  Every residual word ends in 0x8000, under odd and even
    top halves of both signs: odd ones round up and must come out as (top + 1, 0x8001) = r + 1 ulp, even ones as (top, 0x8000) = r."""
    from tribe_hip import _lib, ops

    N = 256
    t = _operands(M, N)
    g = torch.Generator().manual_seed(11)
    top = torch.randint(0x3000, 0x4800, (M, N), generator=g, dtype=torch.int32)   # normal magnitudes 2^-31 .. 2^17, either parity
    top[:, 0] = 0x7F7F   # the largest finite top half: its tie rounds up to the bf16 infinity, and still decodes
    top = top | (torch.randint(0, 2, (M, N), generator=g, dtype=torch.int32) << 15)
    words = (top.to(torch.int64) << 16) | 0x8000
    words = torch.where(words >= 2**31, words - 2**32, words).to(torch.int32).cuda()
    top = top.cuda()
    odd = (top & 1) == 1
    assert int(odd.sum()) > M * N // 4 and int((~odd).sum()) > M * N // 4
    want_hi = (top + odd.to(torch.int32)).to(torch.int16)
    want_lo = torch.where(odd, 0x8001, 0x8000).to(torch.int32)
    kw = dict(rs=False, a="zero_a", bias="zero_bias")
    # f32 -> planes
    res_in = words.view(torch.float32).contiguous()
    got_hi, got_lo = _guarded(M, N, torch.int16, 0x1234), _lo_buf(M, N)
    _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_OUT, res=res_in, C_buf=got_lo, hi_buf=got_hi, **kw)
    assert torch.equal(got_hi[:M], want_hi) and torch.equal(_u16(_lo_get(got_lo)[:M]), want_lo)
    assert torch.equal(_bits(ops.planes_to_f32(got_hi[:M].contiguous(), _lo_get(got_lo)[:M].contiguous())), words + odd.to(torch.int32))
    # planes -> planes: (top, 0x8000) decodes to the same words -- under an odd top no encoder writes that pair, the decoder takes it all the same
    got_hi, got_lo = _guarded(M, N, torch.int16, 0x1234), _lo_buf(M, N)
    got_hi[:M] = top.to(torch.int16)
    _lo_set(got_lo, M, -0x8000)
    _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_INOUT, res=got_lo, C_buf=got_lo, hi_buf=got_hi, **kw)
    assert torch.equal(got_hi[:M], want_hi) and torch.equal(_u16(_lo_get(got_lo)[:M]), want_lo)
    assert bool((got_hi[M:] == 0x1234).all()) and bool((_lo_get(got_lo)[M:] == 0x4321).all()) and _lo_gaps_untouched(got_lo)
    # planes -> f32: the words themselves
    got_hi[:M] = top.to(torch.int16)
    _lo_set(got_lo, M, -0x8000)
    out = _guarded(M, N, torch.float32, -7.0)
    _launch(role, M, N, t, c_dtype=_lib.F32_PLANES_IN, res=got_lo, C_buf=out, hi_buf=got_hi, want_ssq=False, **kw)
    assert torch.equal(_bits(out[:M]), words) and bool((out[M:] == -7.0).all())


# ---- the encoder, planes on against off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 1])
def test_encoder_planes_against_f32_stream(depth):
    from tribe_hip import ops

    # B = 3, T = 200: M = 600 is above the split-K limit and leaves an edge tile of 88 rows
    enc = make_encoder(depth).cuda()
    x0 = encoder_input().cuda()
    # dim 256 plans 128 x 128 tiles on its own: both runs ask for the 256 x 256 role kernels, so that they differ in the stream format alone
    ops.encoder_set_residual_tile_hint(2)
    try:
        runs = {}
        for on in (0, 1):
            ops.encoder_set_residual_planes(bool(on))
            x = x0.clone()
            y = enc.forward_tokens(x, B, T, torch.float32)
            runs[on] = (x, y)
    finally:
        ops.encoder_set_residual_planes(True)
        ops.encoder_set_residual_tile_hint(0)
    (x_f, y_f), (x_p, y_p) = runs[0], runs[1]
    assert bool(torch.isfinite(x_p).all()) and bool(torch.isfinite(y_p).all())
    rel_x = float((x_p.double() - x_f.double()).norm() / x_f.double().norm())
    rel_y = float((y_p.double() - y_f.double()).norm() / y_f.double().norm())
    differing = float((y_p != y_f).float().mean())
    print(f"depth {depth}: rel L2 x {rel_x:.3e}, y {rel_y:.3e}; y elements that differ {differing:.3e}; x elements {float((x_p != x_f).float().mean()):.3e}")
    print(f"  CPU restatement {REL_L2_MEASURED[depth]:.3e}, bound {REL_L2_BOUND[depth]:.3e}")
    assert rel_x <= REL_L2_BOUND[depth] and rel_y <= REL_L2_BOUND[depth]
    assert differing <= MAX_DIFFERING_Y


def test_encoder_default_switch_is_the_f32_path_where_the_role_kernels_do_not_apply():
    """dim 256 plans 128 x 128 tiles: with the switch on and no tile hint the forward is today's, bit for bit."""
    from tribe_hip import ops

    enc = make_encoder(1).cuda()
    x0 = encoder_input().cuda()
    out = []
    try:
        for on in (False, True):
            ops.encoder_set_residual_planes(on)
            x = x0.clone()
            out.append((x, enc.forward_tokens(x, B, T, torch.float32)))
    finally:
        ops.encoder_set_residual_planes(True)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
