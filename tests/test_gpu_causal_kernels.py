"""GPU: the causal softmax row kernels (ops.softmax_causal_fwd / _bwd, csrc/attn_softmax.hip).

Main handle: on the columns j <= i the results -- lse included -- must have the BITS of ops.softmax_dropout_fwd / _bwd run on the same scores
with -inf (forward) or zeros (backward) above the diagonal, since the causal kernels keep their kernel selection, lane ownership and summation
order and a masked element adds an exact zero.  Everything else in the output is +0.0 bits.  The inputs the causal kernels get carry NaN / inf
above the diagonal: nothing of it may reach the output.

Slabs (rows, T, row0): the diagonal i = (row0 + r) % T falls at every position inside a quad, at a row's first and last column, across a
64-column lane stride and across the wrap i = T - 1 -> 0, on every launch path (elem walk, vec walk, reg NV = 1 and 4, vec walk past 1024).

Per-element bounds are those of tests/test_gpu_attn_dropout.py: a kept Pd element within one bf16 step (2^-8 relative) of float64; dS within
2^-8 |float64| + 2^-21 P (|scale m dPd| + |scale D|).  lse2: 1e-5, relative to max(1, |lse2|) -- a short row's log-sum-exp may cancel to near
zero, where a relative figure says nothing about an f32 fma of operands of size ~10."""

import functools

import pytest
import torch

from tests.causal_restatement import tril_mask
from tests.dropout_restatement import keep_mask, multiplier, scale as keep_scale

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SITE = (4 << 56) | 1
SLABS = [(33, 33, 0), (140, 70, 35), (64, 64, 0), (200, 192, 100), (300, 298, 290), (8, 256, 252), (8, 512, 508), (8, 1024, 1020),
         (8, 2048, 2044), (5, 1500, 1497)]
SPLITS = {33: 13, 140: 51, 64: 6, 200: 101, 300: 151, 8: 3, 5: 1}                    # rows -> a first-slab size, never % 4 == 0
PS = [0.0, 0.1, 0.5]
SCALE = 0.125


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pad(T):
    return (T + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _case(rows, T, row0):
    """Scores, the lower-triangle mask, the float64 causal softmax / base-2 log-sum-exp and the backward's operands: computed once per slab,
    never modified."""
    g = torch.Generator().manual_seed(rows * 10007 + T)
    S = torch.randn(rows, T, generator=g) * 2.0
    tril = tril_mask(rows, T, row0)
    S_inf = S.masked_fill(~tril, float("-inf"))
    soft = S_inf.double().softmax(-1)
    lse2 = torch.logsumexp(S_inf.double(), -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))
    P = torch.zeros(rows, _pad(T), dtype=torch.bfloat16)
    P[:, :T] = soft.to(torch.bfloat16)
    dPd = torch.randn(rows, T, generator=g).masked_fill(~tril, 0.0)
    assert bool(tril[:, 0].all()) and int(tril.sum(1).min()) <= 4 and int(tril.sum(1).max()) >= T - 3   # short and (nearly) full rows
    return S, tril, S_inf, soft, lse2, P, dPd


def _on_gpu(S):
    """f32 [rows, T] as the leading T columns of a [rows, T_pad] buffer (the pitch the score GEMM writes with), NaN behind them."""
    rows, T = S.shape
    buf = torch.full((rows, _pad(T)), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :T] = S.cuda()
    return buf[:, :T]


def _mask(rows, T, row0, p):
    keep = torch.from_numpy(keep_mask(row0 + rows, T, p, SEED, SITE)[row0:])
    return keep, multiplier(row0 + rows, T, p, SEED, SITE)[row0:]


def _poison(tril):
    """f32 [rows, T]: 0 where visible, NaN / +inf / -inf in turn above the diagonal."""
    rows, T = tril.shape
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(T) % 3].expand(rows, T)
    return torch.where(tril, torch.zeros(()), bad)


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,T,row0", SLABS)
def test_forward_kernel(rows, T, row0, p):
    from tribe_hip import ops

    S, tril, S_inf, soft, lse2, _, _ = _case(rows, T, row0)
    Tp = _pad(T)
    out = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    Pd, lse = ops.softmax_causal_fwd(_on_gpu(S + _poison(tril)), p, SEED, SITE, row0=row0, out=out)
    assert Pd.data_ptr() == out.data_ptr()
    ref, ref_lse = ops.softmax_dropout_fwd(_on_gpu(S_inf), p, SEED, SITE, row0=row0)
    Pd, lse, ref, ref_lse = Pd.cpu(), lse.cpu(), ref.cpu(), ref_lse.cpu()
    # the bits of the non-causal kernel on the lower triangle, lse included; +0.0 bits everywhere else
    assert torch.equal(_bits(Pd[:, :T])[tril], _bits(ref[:, :T])[tril])
    assert torch.equal(_bits(lse), _bits(ref_lse))
    assert not bool(_bits(Pd[:, :T])[~tril].any()) and not bool(_bits(Pd[:, T:]).any())
    keep, _ = _mask(rows, T, row0, p)
    assert torch.equal(Pd[:, :T] != 0, keep & tril)                                  # the non-zero pattern IS mask AND triangle
    want = soft * float(keep_scale(p))
    sel = keep & tril
    err = ((Pd[:, :T].double() - want).abs() / want)[sel].max()
    lse_err = ((lse.double() - lse2).abs() / lse2.abs().clamp(min=1.0)).max()
    print(f"[{rows}, {T}] row0={row0} p={p}: kept max rel err {float(err):.2e} (bound {2**-8:.2e}), lse2 err {float(lse_err):.2e}")
    assert err <= 2.0**-8 and lse_err < 1e-5


# ---- backward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,T,row0", SLABS)
def test_backward_kernel(rows, T, row0, p):
    from tribe_hip import ops

    _, tril, _, _, _, P, dPd = _case(rows, T, row0)
    Tp = _pad(T)
    keep, m = _mask(rows, T, row0, p)
    P64 = P[:, :T].double()
    D = (m * P64 * dPd.double()).sum(-1, keepdim=True)                               # rowsum(Pd * dPd) over the visible keys
    want = SCALE * P64 * (m * dPd.double() - D)
    negD = (-SCALE * D[:, 0]).float().cuda()
    # what the mask-unaware producers leave above the diagonal: inf / NaN in P (the ACT_EXP2 epilogue) and in dPd
    poison = _poison(tril)
    P_bad = P.clone()
    P_bad[:, :T] = torch.where(tril, P[:, :T], poison.to(torch.bfloat16))
    Pg, dg = P_bad.cuda(), (dPd + poison).cuda()
    dS = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    Pd = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    P_in = Pg.clone()
    ops.softmax_causal_bwd(P_in, dg, negD, SCALE, p, SEED, SITE, row0=row0, dS=dS, Pd=Pd)
    assert torch.equal(_bits(P_in), _bits(Pg))                                       # out of place: P stays
    P_io = Pg.clone()
    dS_io, Pd_io = ops.softmax_causal_bwd(P_io, dg, negD, SCALE, p, SEED, SITE, row0=row0)
    assert Pd_io.data_ptr() == P_io.data_ptr()
    assert torch.equal(_bits(dS_io), _bits(dS)) and torch.equal(_bits(Pd_io), _bits(Pd))
    ref_dS, ref_Pd = ops.softmax_dropout_bwd(P.cuda(), dPd.cuda(), negD, SCALE, p, SEED, SITE, row0=row0)
    got, got_pd, ref_dS, ref_Pd = dS.cpu(), Pd.cpu(), ref_dS.cpu(), ref_Pd.cpu()
    for name, a, b in (("dS", got, ref_dS), ("Pd", got_pd, ref_Pd)):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(_bits(a[:, :T])[tril], _bits(b[:, :T])[tril]), name
        assert not bool(_bits(a[:, :T])[~tril].any()) and not bool(_bits(a[:, T:]).any()), name
    slack = 2.0**-21 * P64 * ((SCALE * m * dPd.double()).abs() + (SCALE * D).abs())
    excess = ((got[:, :T].double() - want).abs() - 2.0**-8 * want.abs() - slack)[tril].max()
    print(f"[{rows}, {T}] row0={row0} p={p}: worst |dS err| - bound {float(excess):.2e} (<= 0 passes)")
    assert excess <= 0


# ---- slabs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,row0", SLABS)
def test_one_call_equals_two_calls_with_row0_moved(rows, T, row0):
    from tribe_hip import ops

    S, _, _, _, _, P, dPd = _case(rows, T, row0)
    cut, p = SPLITS[rows], 0.1
    assert 0 < cut < rows and cut % 4
    Sg = _on_gpu(S)
    whole, lse = ops.softmax_causal_fwd(Sg, p, SEED, SITE, row0=row0)
    parts, lse_parts = torch.empty_like(whole), torch.empty_like(lse)
    ops.softmax_causal_fwd(Sg[:cut], p, SEED, SITE, row0=row0, out=parts[:cut], lse=lse_parts[:cut])
    ops.softmax_causal_fwd(Sg[cut:], p, SEED, SITE, row0=row0 + cut, out=parts[cut:], lse=lse_parts[cut:])
    assert torch.equal(_bits(whole), _bits(parts)) and torch.equal(_bits(lse), _bits(lse_parts))
    negD = torch.randn(rows, generator=torch.Generator().manual_seed(1)).cuda()
    Pg, dg = P.cuda(), dPd.cuda()
    dS, Pd = ops.softmax_causal_bwd(Pg.clone(), dg, negD, SCALE, p, SEED, SITE, row0=row0)
    dS2, Pd2 = torch.empty_like(dS), Pg.clone()
    ops.softmax_causal_bwd(Pd2[:cut], dg[:cut], negD[:cut], SCALE, p, SEED, SITE, row0=row0, dS=dS2[:cut])
    ops.softmax_causal_bwd(Pd2[cut:], dg[cut:], negD[cut:], SCALE, p, SEED, SITE, row0=row0 + cut, dS=dS2[cut:])
    assert torch.equal(_bits(dS), _bits(dS2)) and torch.equal(_bits(Pd), _bits(Pd2))
