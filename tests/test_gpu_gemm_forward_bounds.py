"""GPU: the forward operators of the generic epilogue (csrc/gemm_common.h: epilogue_fast, epilogue_tile16 -> epilogue_row4) on the four
NT tile kernels of the bf16 GEMM (csrc/gemm.hip), per element against the float64 reference of oracle/gemm_ref.py -- the part the encode
path runs outside the role-compiled epilogues: projector (bias + pos_embed row add + subject add), voxel head (alpha + row bias), the
ScaleNorm folding (row_scale; c_bf16 + row_sumsq).  Conventions of test_gpu_gemm_bounds.py, whose helpers are imported: every launch
goes through the C ABI, the test owns every output buffer, every buffer is larger than its matrix (ldc = N + 4 .. 6 or N + 2, rows
M .. M + 8 allocated, ld_c_bf16 > N, ldres > N, lda = ldb = K + 8 with NaN beside the operands, NaN in the pad columns of residual,
rowadd and gadd) and pre-filled with NaN, every element inside and outside [0, M) x [0, N) is compared, and every case is launched
twice and must give the same bits.  An in-place residual fills the window with the residual and only the padding with NaN.

The case table is data in oracle/gemm_ref.py (FWD_CASES); tests/test_gemm_ref_host.py replays the path choice of the kernels on it
(fwd_paths), asserts that every (kernel, path) cell and every operator set on every kernel is reached, that no row can be dropped, that
the library's planner gives each row the kernel it names, and that the inputs tell ten addressing / rounding faults from correct code.

Kernels (tribe_debug_gemm_plan: kind / bn / epilogue_path == 0 asserted per case)
    db128    128 x 128 double-buffered   tile_hint 1          epilogue_fast<NI = 4, NJ = 4, TACC = 0>
    ring128  128 x 128 ring              tile_hint 3          epilogue_fast<NI = 2, NJ = 4, TACC = 0>
    w8_256   256 x 256 8-wave            tile_hint 2 and 6    epilogue_fast<NI = 8, NJ = 4, TACC = 1>: permuted columns, bf16 stores in pairs
    w8_192   256 x 192 8-wave            tile_hint 4 (6 at N = 384)   NJ = 3: the last sub-tile stored unpaired, 48-column row_sumsq slots
    tile_hint 0: (70, 136, 128) -> db128, (70, 136, 256) -> ring128, (12076, 384, 64) -> w8_192: the smallest shapes plan_tiles sends
    there (rules restated beside the rows in oracle/gemm_ref.py); skipped with a message where the planner of the machine says otherwise

Branches and the case that reaches each (BN = 128, 256, 192; M = 300 = ragged for 128- and 256-row tiles; K = 128)
    P1  epilogue_fast                                      N = 2 BN: every operator set but rowadd + residual and the gadd set;
                                                           M = 70 (one tile row, ends inside a 16-row sub-tile and inside a quad of
                                                           lanes) for none / the in-place set, M = 200 for the in-place set
        LDS-slot route of the periodic row add             bias_rowadd7 (wraps inside a sub-tile), bias_rowadd32 at N = 2 BN
        c_bf16 + row_sumsq, row_scale                      (300, 768, 128) / N = 2 BN: the launcher admits them on P1 only
    P2  epilogue_row4, vector branch   (a) tile crossing N N = BN + 8: a full tile (P1) beside an 8-column one
                                       (b) a gadd          projector (alpha + row bias + rowadd 7 + gadd / 32, 5-row table, index
                                                           (3, 0, 3, 4, 1, 1, 2, 0, 4, 3)) at N = BN + 8
                                       (c) rowadd + res    rowadd_res at N = BN + 8
    P3  epilogue_row4, scalar branch   (a) ldc = N + 2     every set P2 takes, at N = BN + 8
                                       (b) a pointer       C offset by one element (res); the column bias offset by one float, beside
                                                           the aligned case
                                       (c) N % 4 == 2      N = BN + 6 with ldc % 4 == 0 (res): the last quad of a row beside vector quads
    refusal                                                fused-norm operands at N = 776 on every hint: non-zero, nothing written

Operator sets (oracle.gemm_ref.FWD_OPS): none; col_bias (aligned / + 1 float); voxel_head = alpha 1/2 + row bias; res (ldres > N);
out_proj = residual * res_scale + column bias in place (f32; bf16 output reads the residual from a buffer of its own); bias_rowadd7,
bias_rowadd32; rowadd_res; projector; row_scale and row_scale_bias_gelu (bf16); bias_gelu (erf form for f32, gelu_poly2 for bf16);
fused_norm = f32 C in place = product + bias + residual * res_scale with c_bf16 and row_sumsq, slots packed and at a pitch of slots + 3.

Criteria (no constant of this file's own)
  EXACT inputs: f32 bit-equal to the float64 reference, bf16 and c_bf16 bit-equal to oracle.layout_ref.bf16_bits of it, every row_sumsq
  slot bit-equal to the float64 sum of squares of its own N / slots columns of the row the kernel stored (integers below 2^24:
  oracle.gemm_ref.is_exact_sumsq).  The GELU sets are bounded as in test_gpu_gemm_bounds.py: B from [-1, 1], 8.3e-5 on an exact
  pre-activation, bf16 store 2^-8.
  RANDOM inputs (300, 768, 128), one per kernel: bias + scaled residual + c_bf16 + row_sumsq; output within K u S + u per f32
  operation, slots within N_slot u sum(x^2) of the float64 sum of squares of the stored row.
  MEASURED on an MI355X (max err / bound; for the record, the bounds are not tuned to these):
    EXACT   all 277 cases bit for bit over every element, c_bf16, slot and all padding: 0
    GELU    f32 (gelu_erf) 0.0046 at worst;  bf16 (gelu_poly2, its rounding included) 0.995 (bias_gelu) and 0.996 (row_scale_bias_gelu):
            an output just above a power of two, where round-to-nearest alone uses the whole 2^-8 |y|
    RANDOM  output 0.0131 (tile_hint 1, 3, 4) and 0.0167 (2);  slots 0.0376 (1, 3), 0.039 (2), 0.0542 (4: 48-column slots)
  No case exposed a fault in csrc/.  That the cases can: with four mistakes planted in a scratch copy of gemm_common.h (the LDS-slot
  rowadd row taken at r + 1; the slot index of row_sumsq ^ 1; res_scale[(n + k) ^ 1] in the scalar branch; two words of the paired
  bf16 store exchanged) 98 of the 317 tests failed -- the rowadd P1 cases on every kernel, the fused-norm and RANDOM slots on every
  kernel, out_proj at ldc = N + 2 on every kernel in both dtypes, every bf16 case of the two 8-wave kernels with a tile on P1 -- and
  no other.
  Wall time on the MI355X, the same machine and session: this module 3.8 s (317 tests), tests/test_gpu_gemm_bounds.py 4.6 s (372 tests).
"""

import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from oracle import gemm_ref as ref
from test_gpu_gemm_bounds import U, Buf, _act_bound, _bf16_in_wider, _dev, _L, _launch, _stream, assert_bounded, assert_exact, same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _wide(x: np.ndarray, ld: int) -> torch.Tensor:
    """The f32 device copy of x [rows, cols] in rows of ld elements, NaN in the pad columns."""
    t = torch.full((x.shape[0], ld), NAN, dtype=torch.float32)
    t[:, : x.shape[1]] = torch.from_numpy(np.array(x))
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _device(M, N, K, bmax):
    """The operands of every case at one shape on the device, laid out with the pitches of ref.fwd_layout (they depend on N alone)."""
    lay = ref.fwd_layout(ref.FwdCase(1, M, N, K, "res", "pad", "bf16", "db128"))
    t = {k: np.array(v) for k, v in ref.fwd_inputs(M, N, K, bmax).items()}          # (copies: the shared arrays are read-only)
    dv = {k: _dev(t[k]) for k in ("cb", "icb", "rb", "rs", "irs", "row_scale", "gidx")}
    dv["a"], dv["b"] = _bf16_in_wider(t["a"], lay["lda"] - K), _bf16_in_wider(t["b"], lay["ldb"] - K)
    dv["res"], dv["ires"] = _wide(t["res"], lay["ldres"]), _wide(t["ires"], lay["ldres"])
    dv["rowadd7"], dv["rowadd32"], dv["gadd"] = _wide(t["rowadd7"], lay["ld_rowadd"]), _wide(t["rowadd32"], lay["ld_rowadd"]), _wide(t["gadd"], lay["ld_gadd"])
    return dv


def _plan(d):
    out = (C.c_int64 * 19)()
    rc = _L().lib().tribe_debug_gemm_plan(C.byref(d), 0, out, 19)
    return rc, list(out)


def _descriptor(case, dv):
    """Fresh NaN-filled outputs (the residual preloaded where the case runs in place) and the descriptor over them."""
    L = _L()
    spec, lay = ref.FWD_OPS[case.ops], ref.fwd_layout(case)
    M, N = case.M, case.N
    c = Buf(lay["lead"] + (M + 8) * lay["ldc"], case.out)
    c.region(lay["lead"], M, N, lay["ldc"])
    if lay["inplace"]:
        c.preload(0, dv["ires" if spec.get("fused") else "res"][:, :N])
    ptr = {k: v.data_ptr() for k, v in dv.items()}
    ptr["c"] = c.ptr()
    bufs = [c]
    if spec.get("fused"):
        cbf = Buf((M + 8) * lay["ld_c_bf16"], "bf16")
        cbf.region(0, M, N, lay["ld_c_bf16"])
        ssq = Buf((M + 8) * lay["ld_row_sumsq"], "f32")
        ssq.region(0, M, lay["slots"], lay["ld_row_sumsq"])
        ptr["c_bf16"], ptr["row_sumsq"] = cbf.ptr(), ssq.ptr()
        bufs += [cbf, ssq]
    return ref.fwd_fill_desc(L.GemmDesc(), L, case, ptr), bufs


def _run(case):
    dv = _device(case.M, case.N, case.K, ref.FWD_OPS[case.ops].get("bmax", ref.A_MAX))
    d, bufs = _descriptor(case, dv)
    _launch(d)
    r = types.SimpleNamespace(bufs=bufs, mats=[], untouched=True)
    for b in bufs:
        (m,), ok = b.read()
        r.mats.append(m)
        r.untouched = r.untouched and ok
    return r


def _check_plan(case):
    """The launch gets the kernel the table names, with the generic epilogue.  tile_hint 0: the plan is read, not assumed."""
    dv = _device(case.M, case.N, case.K, ref.FWD_OPS[case.ops].get("bmax", ref.A_MAX))
    d, _ = _descriptor(case, dv)
    rc, out = _plan(d)
    assert rc == 0, _L().lib().tribe_last_error()
    kind, _, bn, cols, _ = ref.FWD_KERNELS[case.kernel]
    got, want = (out[1], out[3], out[7], out[5]), (kind, bn, 0, 1)
    if case.hint == 0 and got != want:
        pytest.skip(f"the planner of this machine sends {case.M} x {case.N} x {case.K} to kind {out[1]} with {out[3]}-wide tiles, not to {case.kernel}")
    assert got == want, (case.id, got)
    if ref.FWD_OPS[case.ops].get("fused"):
        assert out[4] == cols and int(_L().lib().tribe_gemm_sumsq_slots(C.byref(d))) == ref.fwd_layout(case)["slots"]


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=[c.id for c in ref.FWD_CASES])
def test_forward_operators(case):
    spec, lay = ref.FWD_OPS[case.ops], ref.fwd_layout(case)
    _check_plan(case)
    want, v = ref.fwd_reference(case.M, case.N, case.K, case.ops, lay["bias_lead"])
    r = _run(case)
    got = r.mats[0]
    if ref.fwd_exact(case.ops):
        assert_exact(got, want, case.id)
        print(f"{case.id}: bit-exact over {got.numel()} outputs (max err / bound 0)")
    else:
        assert np.abs(v).std() > 1, "pre-activations are meant to lie where the activation bends"
        assert_bounded(got, want, _act_bound("gelu", types.SimpleNamespace(v=v, want=want), case.out), case.id)
    if spec.get("fused"):
        cbf, slots = r.mats[1], r.mats[2]
        assert_exact(cbf, want, f"{case.id} c_bf16")
        assert_exact(slots, ref.fwd_slots(got.double().numpy(), case.N // lay["slots"]), f"{case.id} row_sumsq")
    assert r.untouched, f"{case.id}: a write outside [0, M) x [0, N) of C, c_bf16 or the slots"
    again = _run(case)
    assert all(same_bits(x.buf, y.buf) for x, y in zip(r.bufs, again.bufs)), f"{case.id}: two launches differ"


@pytest.mark.parametrize("hint", [1, 3, 2, 4, 6])
def test_fused_norm_operands_are_refused_when_a_tile_would_cross_n(hint):
    """N = 776 is a multiple of no tile width: the launcher returns an error and leaves C (the residual), c_bf16 and the slots as they were."""
    kernel = {1: "db128", 3: "ring128", 2: "w8_256", 4: "w8_192", 6: "w8_256"}[hint]
    case = ref.FwdCase(hint, 300, 776, 128, "fused_norm", "pad", "f32", kernel)
    d, bufs = _descriptor(case, _device(300, 776, 128, 1))
    before = [b.buf.clone() for b in bufs]
    assert _plan(d)[0] != 0
    rc = _L().lib().tribe_gemm_bf16(C.byref(d), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and _L().lib().tribe_last_error(), "fused-norm operands with N = 776: accepted"
    assert all(same_bits(b.buf, x) for b, x in zip(bufs, before)), "refused, yet an output was written"
    assert bool(torch.isnan(bufs[1].buf).all()) and bool(torch.isnan(bufs[2].buf).all())


@functools.lru_cache(maxsize=None)
def _random():
    M, N, K = ref.FWD_SUMSQ_SHAPE
    t = ref.random_inputs(M, N, K)
    t["rs"] = (torch.rand(N, generator=torch.Generator().manual_seed(N)) + 0.5).numpy()
    t["dev"] = {"a": _dev(t["a"], torch.bfloat16), "b": _dev(t["b"], torch.bfloat16), "bias": _dev(t["bias"]), "rs": _dev(t["rs"]),
                "res": _wide(t["res"], N + 8)}
    return t


def _run_random(hint):
    L = _L()
    M, N, K = ref.FWD_SUMSQ_SHAPE
    dv = _random()["dev"]
    c, cbf = Buf((M + 8) * (N + 4), "f32"), Buf((M + 8) * (N + 8), "bf16")
    c.region(0, M, N, N + 4)
    cbf.region(0, M, N, N + 8)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = dv["a"].data_ptr(), K, dv["b"].data_ptr(), K
    d.C, d.ldc, d.c_dtype, d.alpha, d.tile_hint = c.ptr(), N + 4, L.F32, 1.0, hint
    d.bias, d.bias_mode, d.res, d.ldres, d.res_scale = dv["bias"].data_ptr(), L.BIAS_COL, dv["res"].data_ptr(), N + 8, dv["rs"].data_ptr()
    d.c_bf16, d.ld_c_bf16 = cbf.ptr(), N + 8
    nslots = int(L.lib().tribe_gemm_sumsq_slots(C.byref(d)))
    assert nslots == N // ref.FWD_KERNELS[{1: "db128", 3: "ring128", 2: "w8_256", 4: "w8_192"}[hint]][3]
    ssq = Buf((M + 8) * (nslots + 1), "f32")
    ssq.region(0, M, nslots, nslots + 1)
    d.row_sumsq, d.ld_row_sumsq = ssq.ptr(), nslots + 1
    rc, out = _plan(d)
    assert rc == 0 and out[7] == 0 and out[3] == {1: 128, 3: 128, 2: 256, 4: 192}[hint]
    _launch(d)
    return [c, cbf, ssq]


@pytest.mark.parametrize("hint", ref.FWD_RANDOM_HINTS)
def test_random_bias_scaled_residual_and_row_sums_of_squares(hint):
    M, N, K = ref.FWD_SUMSQ_SHAPE
    t = _random()
    bufs = _run_random(hint)
    ((got,), ok_c), ((gbf,), ok_bf), ((slots,), ok_s) = (b.read() for b in bufs)
    a = np.abs
    y = t["base"]
    bound = K * U * t["S"] + U * a(y)                      # accumulation; alpha = 1
    y = y + t["bias"].astype(np.float64)
    bound = bound + U * a(y)                               # + bias
    p = t["res"].astype(np.float64) * t["rs"].astype(np.float64)
    y = y + p
    bound = bound + U * a(p) + U * a(y)                    # the scaled residual: a product and a sum (one rounding less where they fuse)
    assert_bounded(got, y, bound, f"random hint {hint} bias + scaled residual")
    assert np.array_equal(gbf.contiguous().view(torch.int16).numpy().view(np.uint16), ref.fwd_bf16_bits(got.numpy())), "c_bf16 must be the bf16 of the stored f32"
    cols = N // slots.shape[1]
    x2 = ref.fwd_slots(got.double().numpy(), cols)
    assert_bounded(slots, x2, cols * U * x2, f"random hint {hint} row_sumsq, {cols}-column slots")
    assert ok_c and ok_bf and ok_s, "a write outside C, c_bf16 or the slots"
    assert all(same_bits(x.buf, y.buf) for x, y in zip(bufs, _run_random(hint))), "two launches differ"
