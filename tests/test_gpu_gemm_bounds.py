"""GPU: the training and extended branches of the bf16 GEMM (csrc/gemm.hip: the transposed-operand kernel, stream-K, split-K, the EXT
epilogue operators, batching / gathering and the K-loop edges of the NT kernels) per element against the float64 reference of
oracle/gemm_ref.py.  Everything is called through the C ABI (`_lib.GemmDesc`, tribe_gemm_bf16): the test owns every output buffer and
fills it with NaN (f32) or a NaN pattern (bf16) first, so an element the kernel skipped, a write into the row padding, into a pad column
or between batches shows.  Every element of every output is compared.  The four role-compiled epilogues, tile_hint 5 and the fp8 GEMM
have tests of this kind already (test_gpu_gemm_role_epilogues.py, test_gpu_fp8_bounds.py) and are left to them.

Branches and the case that reaches each
  (a) gemm_nt_256x256x64<.., TN = 1> (desc.trans_ab: At [K, M], Bt [K, N])
    K loop (nk = K / 64 K-tiles, two LDS buffers)         K = 64 prologue without K-tile 1; 128 with it; 192 the `t + 1 < nk` tail; 256 the
                                                          `t + 2 < nk` branch; 512 the steady state                 (all at 256 x 256)
    K rotation krot = ((tn & 7) + (tm & 3)) % nk          (1024, 2048): tm & 3 = 0..3, tn & 7 = 0..7; nk = 3 and nk = 5: every value, wraps
    clamp of the last 8-wide chunk, masked stores         (8, 16), (264, 520), (1000, 296), (256, 264: a full tile beside an 8-column one),
                                                          operands are column slices of wider matrices (lda > M, ldb > N, NaN beside them)
    epilogue_tile16 -> epilogue_row4, vector branch       every operator at (264, 520, 128): edge tiles
    epilogue_fast<NI = 8, TACC = 0>                       every operator at (512, 512, 128) (its only caller in the bf16 library)
    epilogue_row4, scalar branch                          ldc = N + 2; C offset by one element
    operators                                             none, column bias, row bias, residual (ldres > N), residual * res_scale,
                                                          residual in place, rowadd of period 7 without and with a residual, gadd with a
                                                          divisor of 5, alpha = 1/2 on top of bias + residual; GELU + column bias (bounded)
    batches, strided head slices                          batch1 = 2 x batch0 = 3 as attention backward launches dV / dK: one operand is the
                                                          [T, Tp] probability block (lda = Tp > M), the other a head slice of a [T, h d]
                                                          buffer (batch stride d, row pitch h d), C a bf16 slice of a [T, 3 h d] buffer
                                                          (sC0 = d, ldc = 3 h d); T = 128, 192, d = 64, 384, either operand in either role;
                                                          gather_bias with gather1 = [1, 0]
  (b) stream-K (trans_ab + stream_k; SkSched, second_worker[], streamk_reduce_kernel), f32, alpha = 1/2
    8 x 16 x 131072       one ragged tile in 256 parts of 8 K-steps; the reduce sums 256 slots; the store mask
    264 x 520 x 22016     6 ragged tiles, q = 9: 5 runs cross a tile boundary (second parts), 26 idle workers, 39 - 40 parts per tile
    1024 x 1280 x 8192    20 tiles, q = 10: 16 second parts, no idle worker
    4096 x 6144 x 1088    384 tiles: a whole round stored directly (tiles_dp = 256) beside 128 stream-K tiles; q = 9 against nk = 17:
                          113 second parts, 14 idle workers, 2 - 3 parts per tile
    512 x 512 x 128, 3072 x 3072 x 256    left whole (too few K-steps; a remainder above half a round): workspace bytes 0
    NOT REACHABLE: with 256 workers and a remainder of at most half a round q = ceil(rem nk / 256) stays below nk, so a run never holds a
    whole tile: `partial == false` inside the stream-K region of the GEMM kernel and `w_lo == w_hi` in streamk_reduce_kernel
    (tests/test_gemm_ref_host.py::test_stream_k_with_half_a_round_never_hands_a_run_a_whole_tile).  The refusals (bf16 output, a bias,
    a batch, the workspace) are held by test_gpu_kernels.py / test_abi_and_host.py where they were, and by
    test_split_launch_refuses_and_leaves_c_untouched for the rest (bf16, a batch, an activation, a short or misaligned workspace).
  (c) split-K (gemm_nt_ring128 with splits > 1 + splitk_epilogue_kernel; tile_hint 3, stream_k)
    share counts          2 at K = 1024, 8 at K = 4096, 9 + 10 K-steps at K = 1216, 8 + 8 + 9 at K = 1600     (all at 128 x 128)
    shapes                (77, 200, 4096): ragged M, a tile that crosses N; (128, 1024, 4096): 8 tiles
    the second launch     alpha, row_scale, row bias, column bias, GELU (erf for f32, the packed polynomial for bf16), residual,
                          residual * res_scale in place, rowadd, c_bf16 + row_sumsq -- against the reference AND the un-split launch
    fallback              gadd, aux, SiLU, residual with rowadd, N % 4 != 0, a column bias offset by one float: workspace bytes 0 and
                          the un-split result
  (d) EXT operators (SiLU, SwiGLU, GLU, GELU + pre-activation store, GELU_BWD, EXP2, MUL_AUX) on tile_hint 1, 2, 3, 4
    epilogue_fast                                         (257, 256, 256); (257, 384, 256) for tile_hint 4 (192-wide tiles).  tile_hint 2 / 4
                                                          store through TACC = 1: a lane's columns are permuted there, and the SwiGLU / GLU
                                                          pairs are checked per element under that permutation
    epilogue_tile16 -> epilogue_row4, vector branch       (100, 260, 128); the pair activations need ldc % 4 == 0 for it: ldc = N / 2 + 6
    epilogue_row4, scalar branch                          (100, 260, 128) with ldc = N + 2 (N / 2 + 1 for the pairs) on tile_hint 1 and 2; the
                                                          pair activations also at ldc = N / 2 and N / 2 + 4 (130, 134: no vector stores)
    batched EXP2 / MUL_AUX                                batch1 = 2 x batch0 = 3 with sBias1, sBias0; T = 70 in rows of Tp = 128, T = 256
  (e) batches and gather on the NT kernels (tile_hint 1, 2)   batch1 = 3 x batch0 = 2, every stride larger than its matrix, a residual with
                                                          sRes1 / sRes0; gather1 = [2, 0, 2] with gather_a, gather_b, gather_bias in turn
  (f) K loops of the NT kernels, plain f32                tile_hint 1: K = 64 .. 256 at (129, 129); tile_hint 3: K = 64 .. 512 at (129, 129);
                                                          tile_hint 2 / 4: K = 64 .. 512 at (300, 512) / (300, 384) and the K rotation at
                                                          (1024, 2048, 320)

Two kinds of input (oracle/gemm_ref.py)
  EXACT: integer operands in [-3, 3], alpha / row_scale / res_scale in {1/2, 1, 2}, addends multiples of 1/64 in [-2, 2].  Every partial
  sum is an integer below 9 K < 2^24, so the f32 result does not depend on the order of the additions, on the split of K over workgroups
  or on the matrix unit's internals; the f32 output is compared BIT FOR BIT with the float64 reference, the bf16 output with
  round-to-nearest-even of it (oracle.layout_ref.bf16_bits), and a second launch must give the same bits.  A stale LDS buffer, a dropped
  or doubled K-step, a part summed into the wrong tile, a wrong swizzle, clamp or column pairing changes an integer.
  For the activations B is drawn from [-1, 1] and K <= 256: the pre-activation v is exact and lies where the activations bend, so the
  error seen is the activation's alone.  (The GELU case of split-K needs K >= 1024 by the planner's rule: B from [-1, 1] at K = 4096.)
  RANDOM: randn operands rounded to bf16, one case per kernel family, f32.  The stream-K case is the plain product: the launcher
  refuses a bias or a residual on a stream-K launch (test_gpu_kernels.py holds that refusal), so none can ride along there.

Bounds (u = 2^-24; S = sum_k |a_k b_k|; y the float64 value after each step)
    accumulation           K u S |alpha|
    each f32 operation     u |its result|
    GELU                   1.13 bound + 8.3e-5
    SiLU                   1.1 bound + (2 |v| + 8) u |y| + (1 + |v|) 2^-126
    sigmoid                0.25 bound + (2 |v| + 8) u |s| + 2^-126
    SwiGLU silu(g) * w     |w| e_silu(g) + |silu(g)| e(w) + u |y|;   GLU g * sigmoid(w): |g| e_sigmoid(w) + |sigmoid(w)| e(g) + u |y|
    GELU_BWD v * gelu'(p)  |v| 1e-4 + u |y|       (test_gpu_training.py::test_gelu_backward_epilogue pins |gelu' error| <= 1e-4 on [-6, 6])
    MUL_AUX                u |y|                  (one rounded product)
    EXP2                   (2 |x| + 8) u |y| + 2^-126      (v_exp_f32 of an exact argument x)
    bf16 store             2^-8 (|y| + bound)
    row_sumsq              N u sum(x^2) against the float64 sum of squares of the row the kernel stored
  MEASURED on an MI355X (max err / bound; every test prints its own):
    RANDOM  TN (1000, 296, 192) bias + residual 0.0097;  split-K (77, 200, 4096) bias + residual 8.5e-5;
            stream-K (264, 520, 22016) plain 9.0e-6
    EXP2    exact arguments against float64 exp2: 0.115 (f32 output) and 0.779 (bf16 output, its rounding included) at worst over
            every tile kernel and shape: the bound stands as it is
    GELU    the bf16 form (gelu_poly2) missed its bound by up to 24x on pre-activations below -15 (TN and EXT cases 4 - 5.7x at
            |v| < 80, split-K 19 - 24x at |v| < 450): v times a Phi clamped at -4.1e-6 instead of 0.  Fixed in csrc/gemm_common.h by
            moving the lower clamp onto the fit's zero; test_gelu_far_from_zero holds it down to v = -8192
"""

import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from oracle import gemm_ref as ref
from oracle.layout_ref import bf16_bits

pytestmark = pytest.mark.gpu

U = 2.0**-24
BF_U = 2.0**-8
TINY = 2.0**-126
DTYPES = ["f32", "bf16"]
PAIR = ref.PAIR_ACTS


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
def _L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import _lib

    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _esz(out):
    return 4 if out == "f32" else 2


class Buf:
    """An owned, NaN-filled flat buffer with 64 guard elements behind.  The matrices a launch may write are registered as regions;
    read() returns them and whether every element outside them still holds the fill."""

    def __init__(self, n, out):
        self.out, self.n, self.regions = out, n, []
        self.buf = torch.full((n + 64,), float("nan"), dtype=torch.float32 if out == "f32" else torch.bfloat16, device="cuda")

    def ptr(self, off=0):
        return self.buf.data_ptr() + off * _esz(self.out)

    def region(self, off, rows, cols, ld):
        assert off >= 0 and off + (rows - 1) * ld + cols <= self.n, "a region outside its buffer"
        self.regions.append((off, rows, cols, ld))
        return len(self.regions) - 1

    def preload(self, r, values: torch.Tensor):
        off, rows, cols, ld = self.regions[r]
        idx = off + torch.arange(rows, device="cuda")[:, None] * ld + torch.arange(cols, device="cuda")[None, :]
        self.buf[idx] = values.to(self.buf.dtype)

    def read(self):
        flat = self.buf.cpu()
        nan = torch.isnan(flat).numpy()
        if len(self.regions) == 1 and self.regions[0][2] == self.regions[0][3]:      # one contiguous matrix: no index arrays
            off, rows, cols, _ = self.regions[0]
            end = off + rows * cols
            return [flat[off:end].view(rows, cols)], bool(nan[:off].all() and nan[end:].all())
        mask = np.zeros(flat.numel(), dtype=bool)
        mats = []
        for off, rows, cols, ld in self.regions:
            idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
            assert not mask[idx.ravel()].any(), "overlapping regions"
            mask[idx.ravel()] = True
            mats.append(flat[torch.from_numpy(idx)])
        return mats, bool(nan[~mask].all())


def same_bits(x: torch.Tensor, y: torch.Tensor) -> bool:
    """Two device buffers hold the same bit patterns (fill included)."""
    it = torch.int32 if x.dtype == torch.float32 else torch.int16
    return x.dtype == y.dtype and torch.equal(x.view(it), y.view(it))


_WS = {}


def _workspace(nbytes):
    """A 16-byte aligned workspace, NaN-filled before every use: a part read from a slot nobody wrote shows."""
    if _WS.get("n", 0) < nbytes:
        _WS["t"], _WS["n"] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device="cuda"), nbytes
    _WS["t"].fill_(float("nan"))
    return _WS["t"]


def _launch(d):
    L = _L()
    L.check(L.lib().tribe_gemm_bf16(C.byref(d), _stream()), "tribe_gemm_bf16")
    torch.cuda.synchronize()


def _ws_bytes(d):
    return int(_L().lib().tribe_gemm_stream_k_workspace_bytes(C.byref(d)))


def _split(d):
    """desc.stream_k = 1 with the workspace the planner asks for; returns the bytes (0 = the launch stays whole)."""
    d.stream_k = 1
    nbytes = _ws_bytes(d)
    if nbytes:
        ws = _workspace(nbytes)
        d.stream_k_ws, d.stream_k_ws_bytes = ws.data_ptr(), nbytes
    return nbytes


def assert_exact(got: torch.Tensor, want64: np.ndarray, what: str):
    """f32: bit-identical to the float64 value cast to f32; bf16: to round-to-nearest-even of it.  (want64 is f32-exact: asserted.)"""
    assert tuple(got.shape) == want64.shape, f"{what}: shape {tuple(got.shape)} vs {want64.shape}"
    w32 = want64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want64), f"{what}: the reference itself is not exact in f32"
    if got.dtype == torch.float32:
        g, w = got.contiguous().view(torch.int32).numpy(), w32.view(np.int32)
    else:
        g, w = got.contiguous().view(torch.int16).numpy().view(np.uint16), bf16_bits(w32).reshape(want64.shape)
    bad = g != w
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from the exact result; first at {at}: "
                             f"got {float(got[at]):.9g}, want {float(want64[at]):.9g}")


def assert_bounded(got: torch.Tensor, want64: np.ndarray, bound: np.ndarray, what: str) -> float:
    assert tuple(got.shape) == want64.shape, f"{what}: shape {tuple(got.shape)} vs {want64.shape}"
    g = got.double().numpy()
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} outputs are not finite (skipped elements keep the NaN fill)"
    err = np.abs(g - want64)
    zero = bound == 0                                   # an exact 0 by construction: nothing but 0 will do
    assert not err[zero].any(), f"{what}: a non-zero result where the exact value is 0 by construction"
    worst = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, max err / bound {worst:.3g}")
    assert worst <= 1.0, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------
# exact inputs
# ------------------------------------------------------------------------------------------------
def _bf16_in_wider(a: np.ndarray, pad: int) -> torch.Tensor:
    """The bf16 device copy of a [rows, cols], as the left column slice of a [rows, cols + pad] matrix whose other columns hold NaN."""
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.bfloat16)
    t[:, : a.shape[1]] = torch.from_numpy(a).to(torch.bfloat16)
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _exact(M, N, K, tn=False, bmax=3, pad=0):
    """Integer operands on the device (trans_ab: At [K, M], Bt [K, N]; pad: the row pitch exceeds the row by `pad` NaN columns) and
    the exact product in float64."""
    a, b = ref.exact_operands((K, M) if tn else (M, K), (K, N) if tn else (N, K), seed=100003 * M + 101 * N + K + 7 * bmax + tn, bmax=bmax)
    return {"acc": ref.product64(a, b, tn), "da": _bf16_in_wider(a, pad), "db": _bf16_in_wider(b, pad), "lda": a.shape[1] + pad,
            "ldb": b.shape[1] + pad}


@functools.lru_cache(maxsize=None)
def _operands(M, N):
    """Epilogue operands that keep the exact cases exact (oracle/gemm_ref.py)."""
    g = np.random.default_rng(7 * M + N)
    t = {"cb": ref.sixty_fourths(g, N + 1), "rb": ref.sixty_fourths(g, M), "rb_exp": ref.sixty_fourths(g, M, lo=-24.0, hi=0.0),
         "res": ref.sixty_fourths(g, M, N + 4), "rs": ref.power_of_two(g, N), "row_scale": ref.power_of_two(g, M),
         "rowadd": ref.sixty_fourths(g, 7, N + 4), "gadd": ref.sixty_fourths(g, 3, N + 4),
         "gidx": np.resize(np.array([2, 0, 2, 1, 1, 0, 2], dtype=np.int64), (M + 4) // 5),
         # a saved GELU pre-activation spread over [-6, 6] and a probability-like factor, both bf16 values
         "pre": torch.from_numpy(g.uniform(-6.0, 6.0, (M, N + 4)).astype(np.float32)).bfloat16().float().numpy(),
         "p": torch.from_numpy(g.uniform(0.0, 1.0, (M, N + 4)).astype(np.float32)).bfloat16().float().numpy()}
    t["dev"] = {k: _dev(v) for k, v in t.items()}
    return t


ACT_CODE = {"gelu": "ACT_GELU", "gelu_aux": "ACT_GELU", "silu": "ACT_SILU", "swiglu": "ACT_SWIGLU", "glu": "ACT_GLU", "gelu_bwd": "ACT_GELU_BWD",
            "exp2": "ACT_EXP2", "mul_aux": "ACT_MUL_AUX"}


def _run(M, N, K, out="f32", op="none", *, tn=False, hint=0, act=None, ldc=None, lead=0, bias_lead=0, bmax=3, pad=0, split=False,
         fused=False):
    """One launch on exact inputs.  op: the plain operator set; act: the activation (with the bias it goes with).  Returns a namespace:
    got [M, n_out] (CPU), untouched (padding and guard keep the fill), want / v (float64 reference, pre-activation), buf (the device
    buffer, for bit comparisons between launches), nbytes (the workspace a split launch took), aux_got / aux_untouched (GELU's
    pre-activation store), cbf / slots (c_bf16, row_sumsq)."""
    L = _L()
    x, o = _exact(M, N, K, tn, bmax, pad), _operands(M, N)
    dv = o["dev"]
    pair = act in PAIR
    n_out = N // 2 if pair else N
    ldc = ldc or n_out
    c = Buf(lead + M * ldc, out)
    c.region(lead, M, n_out, ldc)
    alpha = {"alpha_half": 0.5, "alpha2": 2.0}.get(op, 0.5 if act == "exp2" else 1.0)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = x["da"].data_ptr(), x["lda"], x["db"].data_ptr(), x["ldb"]
    d.C, d.ldc, d.c_dtype = c.ptr(lead), ldc, L.F32 if out == "f32" else L.BF16
    d.alpha, d.trans_ab, d.tile_hint = alpha, int(tn), hint
    kw = {"alpha": alpha}
    if op in ("col_bias", "alpha_half", "gelu") or bias_lead or act in ("silu", "swiglu", "glu", "gelu_aux"):
        d.bias, d.bias_mode = dv["cb"].data_ptr() + 4 * bias_lead, L.BIAS_COL
        kw["col_bias"] = o["cb"][bias_lead: bias_lead + N]
    if op == "row_bias" or act in ("exp2", "mul_aux"):
        which = "rb_exp" if act == "exp2" else "rb"
        d.bias, d.bias_mode = dv[which].data_ptr(), L.BIAS_ROW
        kw["row_bias"] = o[which]
    if op == "row_scale":
        d.row_scale = dv["row_scale"].data_ptr()
        kw["row_scale"] = o["row_scale"]
    if op in ("res_ldres", "res_scale", "rowadd_res", "alpha_half"):
        d.res, d.ldres = dv["res"].data_ptr(), N + 4
        kw["res"] = o["res"][:, :N]
    if op in ("res_scale", "res_scale_inplace"):
        d.res_scale = dv["rs"].data_ptr()
        kw["res_scale"] = o["rs"]
    if op in ("res_inplace", "res_scale_inplace"):               # x += gemm(...): the residual is C itself (f32)
        assert out == "f32"
        c.preload(0, dv["res"][:, :N])
        d.res, d.ldres = c.ptr(lead), ldc
        kw["res"] = o["res"][:, :N]
    if op in ("rowadd", "rowadd_res"):
        d.rowadd, d.ld_rowadd, d.rowadd_period = dv["rowadd"].data_ptr(), N + 4, 7
        kw.update(rowadd=o["rowadd"][:, :N], rowadd_period=7)
    if op == "gadd":
        d.gadd, d.gadd_index, d.gadd_div, d.ld_gadd = dv["gadd"].data_ptr(), dv["gidx"].data_ptr(), 5, N + 4
        kw.update(gadd=o["gadd"][:, :N], gadd_index=o["gidx"], gadd_div=5)
    if op == "gelu":
        act = "gelu"
    aux = None
    if act:
        d.act = getattr(L, ACT_CODE[act])
        kw["act"] = "gelu" if act == "gelu_aux" else act
    if act == "gelu_aux":
        aux = Buf(M * (N + 4), "bf16")
        aux.region(0, M, N, N + 4)
        d.aux, d.ld_aux = aux.ptr(), N + 4
    if act == "gelu_bwd":
        daux = dv["pre"].to(torch.bfloat16)
        d.aux, d.ld_aux = daux.data_ptr(), N + 4
        kw["aux"] = o["pre"][:, :N]
    if act == "mul_aux":                                          # laid out like C: ld_aux == ldc, the same element offset
        p = np.resize(o["p"], (M, ldc))
        daux = torch.cat([torch.zeros(lead), torch.from_numpy(p).flatten()]).to(torch.bfloat16).cuda()
        d.aux, d.ld_aux = daux.data_ptr() + 2 * lead, ldc
        kw["aux"] = p[:, :N]
    cbf = ssq = None
    if fused:                                                     # the fused-norm producer outputs: a bf16 copy and row sums of squares
        assert out == "f32"
        cbf = Buf(M * (N + 4), "bf16")
        cbf.region(0, M, N, N + 4)
        d.c_bf16, d.ld_c_bf16 = cbf.ptr(), N + 4
        nslots = int(L.lib().tribe_gemm_sumsq_slots(C.byref(d)))
        assert nslots == N // 64
        ssq = Buf(M * (nslots + 1), "f32")
        ssq.region(0, M, nslots, nslots + 1)
        d.row_sumsq, d.ld_row_sumsq = ssq.ptr(), nslots + 1
    nbytes = _split(d) if split else 0
    _launch(d)
    (got,), untouched = c.read()
    want, v = ref.epilogue64(x["acc"], want_preact=True, **kw)
    r = types.SimpleNamespace(got=got, untouched=untouched, want=want, v=v, buf=c.buf, nbytes=nbytes, kw=kw)
    if aux is not None:
        (r.aux_got,), r.aux_untouched = aux.read()
    if fused:
        (r.cbf,), cbf_ok = cbf.read()
        (r.slots,), ssq_ok = ssq.read()
        r.untouched = untouched and cbf_ok and ssq_ok
    return r


def _check_exact_twice(what, *args, **kw):
    """The launch equals the reference bit for bit, leaves the padding alone, and a second launch gives the same bits."""
    r = _run(*args, **kw)
    assert_exact(r.got, r.want, what)
    assert r.untouched, f"{what}: a write outside C"
    assert same_bits(r.buf, _run(*args, **kw).buf), f"{what}: two launches differ"
    return r


def _act_bound(act, r, out):
    """The activation's own error on an exact pre-activation v (module docstring)."""
    a = np.abs
    v, y = r.v, r.want
    e_silu = lambda t: (2 * a(t) + 8) * U * a(ref.silu64(t)) + (1 + a(t)) * TINY          # noqa: E731
    e_sig = lambda t: (2 * a(t) + 8) * U * ref.sigmoid64(t) + TINY                        # noqa: E731
    if act in ("gelu", "gelu_aux"):
        bound = np.full_like(y, 8.3e-5)
    elif act == "silu":
        bound = e_silu(v)
    elif act == "swiglu":
        bound = a(v[:, 1::2]) * e_silu(v[:, 0::2]) + U * a(y)
    elif act == "glu":
        bound = a(v[:, 0::2]) * e_sig(v[:, 1::2]) + U * a(y)
    elif act == "gelu_bwd":
        bound = a(v) * 1e-4 + U * a(y)
    elif act == "mul_aux":
        bound = U * a(y)
    elif act == "exp2":
        bound = (2 * a(v) + 8) * U * a(y) + TINY
    else:
        raise ValueError(act)
    return bound + (BF_U * (a(y) + bound) if out == "bf16" else 0.0)


# ------------------------------------------------------------------------------------------------
# (a) the transposed-operand kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 512])
def test_tn_k_loop(K, out):
    _check_exact_twice(f"tn 256x256x{K} {out}", 256, 256, K, out, tn=True)


@pytest.mark.parametrize("K", [192, 320])
def test_tn_k_rotation(K):
    """4 x 8 tiles: krot = ((tn & 7) + (tm & 3)) % nk takes every value mod nk = 3 and mod 5, and wraps."""
    _check_exact_twice(f"tn 1024x2048x{K}", 1024, 2048, K, tn=True)


TN_EDGES = [(8, 16), (264, 520), (1000, 296), (256, 264)]


@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("M,N", TN_EDGES, ids=[f"{m}x{n}" for m, n in TN_EDGES])
def test_tn_edge_clamp_and_masked_stores(M, N, out):
    """The staging clamps a chunk past M / N to the last whole 8-wide chunk and the stores are masked; the operands are column slices
    of wider matrices (lda = M + 24, ldb = N + 24) whose other columns hold NaN, and C has ldc = N + 4."""
    _check_exact_twice(f"tn edge {M}x{N} {out}", M, N, 192, out, tn=True, pad=24, ldc=N + 4)


TN_OPS = ["none", "col_bias", "row_bias", "res_ldres", "res_scale", "res_inplace", "rowadd", "rowadd_res", "gadd", "alpha_half"]
TN_SHAPES = {"edge": (264, 520, 128), "fast": (512, 512, 128)}
TN_OP_CASES = [(op, s, out) for op in TN_OPS for s in TN_SHAPES for out in DTYPES if not (op == "res_inplace" and out == "bf16")]


@pytest.mark.parametrize("op,shape,out", TN_OP_CASES, ids=[f"{o}-{s}-{t}" for o, s, t in TN_OP_CASES])
def test_tn_operators(op, shape, out):
    M, N, K = TN_SHAPES[shape]
    _check_exact_twice(f"tn {op} {shape} {out}", M, N, K, out, op, tn=True, ldc=N + 4 if op == "res_inplace" else None)


@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("shape", list(TN_SHAPES))
def test_tn_gelu_with_column_bias(shape, out):
    M, N, K = TN_SHAPES[shape]
    r = _run(M, N, K, out, "gelu", tn=True, bmax=1)
    assert np.abs(r.v).std() > 1, "pre-activations are meant to lie where the activation bends"
    assert_bounded(r.got, r.want, _act_bound("gelu", r, out), f"tn gelu {shape} {out}")
    assert r.untouched


@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("name,kw", [("ldc_plus_2", dict(ldc=522)), ("c_plus_one", dict(ldc=524, lead=1))])
def test_tn_scalar_epilogue(name, kw, out):
    """An ldc or a C that 16-byte accesses cannot take: the element-wise branch of epilogue_row4, with column bias and residual riding
    along so that its scalar loads are checked too."""
    for op in ("col_bias", "alpha_half"):
        _check_exact_twice(f"tn {name} {op} {out}", 264, 520, 128, out, op, tn=True, **kw)


def _flat(g, n, bmax):
    return g.integers(-bmax, bmax + 1, n).astype(np.float32)


def _mat(flat, off, rows, cols, ld):
    return flat[off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]]


def _run_batched(M, N, K, b1n, b0n, a, b, c, out, *, tn=False, hint=0, bias=None, res=None, act=None, aux=None, alpha=1.0, gather=None,
                 flag=None):
    """A batched launch from flat host arrays.  a, b: (flat f32 array of bf16-exact values, offset, ld, s1, s0); c: (elements, offset, ld,
    s1, s0); bias: (flat, mode, s1, s0); res: (flat, ld, s1, s0); aux: flat bf16 values laid out like C (MUL_AUX).  Every batch is
    compared with the reference of the same slices; returns the worst err / bound of a bounded activation (else 0)."""
    L = _L()
    (fa, oa, lda, sa1, sa0), (fb, ob, ldb, sb1, sb0), (cn, oc, ldc, sc1, sc0) = a, b, c
    dA, dB = _dev(fa, torch.bfloat16), _dev(fb, torch.bfloat16)
    cb = Buf(cn, out)
    for b1 in range(b1n):
        for b0 in range(b0n):
            cb.region(oc + b1 * sc1 + b0 * sc0, M, N, ldc)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, b1n, b0n
    d.A, d.lda, d.sA1, d.sA0 = dA.data_ptr() + 2 * oa, lda, sa1, sa0
    d.B, d.ldb, d.sB1, d.sB0 = dB.data_ptr() + 2 * ob, ldb, sb1, sb0
    d.C, d.ldc, d.sC1, d.sC0, d.c_dtype = cb.ptr(oc), ldc, sc1, sc0, L.F32 if out == "f32" else L.BF16
    d.alpha, d.trans_ab, d.tile_hint = alpha, int(tn), hint
    keep = [dA, dB]
    if bias is not None:
        fbias, mode, sbi1, sbi0 = bias
        keep.append(_dev(fbias))
        d.bias, d.bias_mode, d.sBias1, d.sBias0 = keep[-1].data_ptr(), L.BIAS_COL if mode == "col" else L.BIAS_ROW, sbi1, sbi0
    if res is not None:
        fres, ldres, sr1, sr0 = res
        keep.append(_dev(fres))
        d.res, d.ldres, d.sRes1, d.sRes0 = keep[-1].data_ptr(), ldres, sr1, sr0
    if aux is not None:
        keep.append(_dev(aux, torch.bfloat16))
        d.aux, d.ld_aux = keep[-1].data_ptr() + 2 * oc, ldc
    if act:
        d.act = getattr(L, ACT_CODE[act])
    if gather is not None:
        keep.append(_dev(np.asarray(gather, dtype=np.int64)))
        d.gather1 = keep[-1].data_ptr()
        setattr(d, flag, 1)
    _launch(d)
    mats, untouched = cb.read()
    worst = 0.0
    for b1 in range(b1n):
        ga, gb, gbias = ((int(gather[b1]) if flag == f else b1) for f in ("gather_a", "gather_b", "gather_bias"))
        for b0 in range(b0n):
            am = _mat(fa, oa + ga * sa1 + b0 * sa0, K if tn else M, M if tn else K, lda)
            bm = _mat(fb, ob + gb * sb1 + b0 * sb0, K if tn else N, N if tn else K, ldb)
            kw = {"alpha": alpha, "act": act}
            if bias is not None:
                n_bias = N if mode == "col" else M
                kw["col_bias" if mode == "col" else "row_bias"] = fbias[gbias * sbi1 + b0 * sbi0: gbias * sbi1 + b0 * sbi0 + n_bias]
            if res is not None:
                kw["res"] = _mat(fres, b1 * sr1 + b0 * sr0, M, N, ldres)
            if aux is not None:
                kw["aux"] = _mat(aux, oc + b1 * sc1 + b0 * sc0, M, N, ldc)
            want, v = ref.epilogue64(ref.product64(am, bm, tn), want_preact=True, **kw)
            got, what = mats[b1 * b0n + b0], f"batch ({b1}, {b0}) {out}"
            if act:
                worst = max(worst, assert_bounded(got, want, _act_bound(act, types.SimpleNamespace(v=v, want=want), out), what))
            else:
                assert_exact(got, want, what)
    assert untouched, "a write outside the batches of C (padding, pad columns, the rest of the big buffer)"
    return worst


@pytest.mark.parametrize("heads_on", ["B", "A"])
@pytest.mark.parametrize("T,dh", [(128, 64), (192, 64), (128, 384), (192, 384)])
def test_tn_batched_head_slices_as_attention_backward(T, dh, heads_on):
    """dV = P^T dO / dK = dS^T Q of modeling_utils/autograd.py: batch1 = 2 sequences x batch0 = 3 heads, the reduction over the T query
    rows.  heads_on B (the launch autograd makes): At = a [T, Tp] block (lda = Tp > M = T), Bt = a head slice of a [T, h d] buffer
    (sB0 = d, ldb = h d), C = a bf16 slice of the [T, 3 h d] qkv gradient (sC0 = d, ldc = 3 h d).  heads_on A: the roles swapped
    (sA0 = d, lda = h d; C [d, T] blocks in rows of Tp).  Everything else in the big buffers keeps its fill."""
    nb, h, Tp = 2, 3, T + 64
    g = np.random.default_rng(T + dh)
    blocks = (_flat(g, nb * h * T * Tp, 3), 0, Tp, h * T * Tp, T * Tp)            # [nb, h, T, Tp]
    heads = (_flat(g, nb * T * h * dh, 3), 0, h * dh, T * h * dh, dh)              # [nb T, h d], head b0 = columns b0 d ..
    if heads_on == "B":
        c = (nb * T * 3 * h * dh, 2 * h * dh, 3 * h * dh, T * 3 * h * dh, dh)      # the V third of [nb T, 3 h d]
        _run_batched(T, dh, T, nb, h, blocks, heads, c, "bf16", tn=True)
    else:
        c = (nb * h * dh * Tp, 0, Tp, h * dh * Tp, dh * Tp)                        # [nb, h, d, Tp], T columns written
        _run_batched(dh, T, T, nb, h, heads, blocks, c, "bf16", tn=True)


def test_tn_gather_bias():
    """gather1 = [1, 0] with gather_bias: the column bias of batch b1 comes from gather1[b1], A, B and C keep the plain index."""
    M, N, K = 264, 296, 128
    g = np.random.default_rng(11)
    a = (_flat(g, 2 * K * (M + 8), 3), 0, M + 8, K * (M + 8), 0)
    b = (_flat(g, 2 * K * (N + 8), 3), 0, N + 8, K * (N + 8), 0)
    bias = (ref.sixty_fourths(g, 2 * (N + 4)), "col", N + 4, 0)
    _run_batched(M, N, K, 2, 1, a, b, (2 * M * (N + 4) + 8, 0, N + 4, M * (N + 4) + 8, 0), "f32", tn=True, bias=bias, gather=[1, 0],
                 flag="gather_bias")


# ------------------------------------------------------------------------------------------------
# (b) stream-K
# ------------------------------------------------------------------------------------------------
def _plan(tiles, nk):
    out = (C.c_int32 * 260)()
    grid = _L().lib().tribe_gemm_stream_k_plan(tiles, nk, out)
    return grid, list(out)


def _run_stream_k(M, N, K, split, ldc):
    L = _L()
    x = _exact(M, N, K, True)
    c = Buf(M * ldc, "f32")
    c.region(0, M, N, ldc)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = x["da"].data_ptr(), x["lda"], x["db"].data_ptr(), x["ldb"]
    d.C, d.ldc, d.c_dtype, d.alpha, d.trans_ab = c.ptr(), ldc, L.F32, ref.STREAM_K_ALPHA, 1
    nbytes = _split(d) if split else 0
    _launch(d)
    return c, nbytes


STREAM_K = list(ref.STREAM_K_CASES)


@pytest.mark.parametrize("M,N,K", STREAM_K, ids=["x".join(map(str, s)) for s in STREAM_K])
def test_stream_k_equals_the_reference_and_the_whole_launch(M, N, K):
    claim = ref.STREAM_K_CASES[(M, N, K)]
    tiles, nk = ref.tiles256(M, N), K // ref.BK
    grid, out = _plan(tiles, nk)
    replay = ref.plan_stream_k(tiles, nk)
    ldc = N + 4 if N % 256 else N                       # ragged cases: the row padding is watched too
    if claim is None:
        assert grid == tiles and replay is None
    else:                                               # the case reaches the branch it is there for
        assert out[3] == 256 and (grid, out[0], out[1], out[2]) == (replay["grid"], replay["tiles_dp"], replay["rem_units"], replay["q"])
        assert out[4: 4 + replay["second"]] == replay["second_worker"]
        assert {k: replay[k] for k in ("tiles_dp", "q", "second", "idle", "parts")} == {k: claim[k] for k in ("tiles_dp", "q", "second", "idle", "parts")}
    c, nbytes = _run_stream_k(M, N, K, True, ldc)
    assert nbytes == (0 if claim is None else 2 * 256 * 256 * 256 * 4)
    (got,), untouched = c.read()
    assert_exact(got, _exact(M, N, K, True)["acc"] * ref.STREAM_K_ALPHA, f"stream-K {M}x{N}x{K}")
    assert untouched, "a write outside C"
    whole, _ = _run_stream_k(M, N, K, False, ldc)
    assert same_bits(c.buf, whole.buf), "the split launch differs from the whole one"
    again, _ = _run_stream_k(M, N, K, True, ldc)
    assert same_bits(c.buf, again.buf), "two split launches differ"


REFUSALS = {
    "bf16 output": lambda d, L: setattr(d, "c_dtype", L.BF16),
    "a batch": lambda d, L: setattr(d, "batch0", 2),
    "an activation": lambda d, L: setattr(d, "act", L.ACT_GELU),
    "no workspace": lambda d, L: setattr(d, "stream_k_ws", None),
    "a workspace 4 bytes short": lambda d, L: setattr(d, "stream_k_ws_bytes", d.stream_k_ws_bytes - 4),
    "a misaligned workspace": lambda d, L: setattr(d, "stream_k_ws", d.stream_k_ws + 4),
}


# split-K serves bf16 and GELU, and a batched NT launch is simply not split: those three are stream-K's alone
REFUSAL_CASES = [("stream-K", n) for n in REFUSALS] + [("split-K", n) for n in REFUSALS if "workspace" in n]


@pytest.mark.parametrize("kind,name", REFUSAL_CASES, ids=[f"{k}-{n.replace(' ', '_')}" for k, n in REFUSAL_CASES])
def test_split_launch_refuses_and_leaves_c_untouched(kind, name):
    """What test_gpu_kernels.py does not already hold: a stream-K launch with a bf16 C, a batch or an activation, and either split
    launch with a workspace that is missing, too small or not 16-byte aligned, returns an error before anything is launched."""
    L = _L()
    tn = kind == "stream-K"
    M, N, K = (264, 520, 22016) if tn else (77, 200, 4096)
    x = _exact(M, N, K, tn)
    c = Buf(2 * M * N, "f32")
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = x["da"].data_ptr(), x["lda"], x["db"].data_ptr(), x["ldb"]
    d.C, d.ldc, d.c_dtype, d.alpha, d.trans_ab, d.tile_hint = c.ptr(), N, L.F32, 1.0, int(tn), 0 if tn else 3
    assert _split(d) > 0
    REFUSALS[name](d, L)
    rc = L.lib().tribe_gemm_bf16(C.byref(d), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and L.lib().tribe_last_error(), f"{kind} with {name}: accepted"
    assert bool(torch.isnan(c.buf).all()), f"{kind} with {name}: refused, yet C was written"


# ------------------------------------------------------------------------------------------------
# (c) split-K
# ------------------------------------------------------------------------------------------------
def _check_split(what, M, N, K, out, op="none", *, bounded=None, hint=3, **kw):
    """The split launch takes the workspace of the planned share count, equals the reference (bit for bit, or within `bounded`'s bound)
    and equals the un-split launch bit for bit."""
    shares = ref.split_k_shares(M, N, K)
    r = _run(M, N, K, out, op, hint=hint, split=True, **kw)
    assert r.nbytes == len(shares) * M * N * 4 and len(shares) >= 2, f"{what}: {r.nbytes} bytes for {len(shares)} shares"
    if bounded:
        assert_bounded(r.got, r.want, _act_bound(bounded, r, out), what)
    else:
        assert_exact(r.got, r.want, what)
    assert r.untouched, f"{what}: a write outside C"
    whole = _run(M, N, K, out, op, hint=hint, **kw)
    assert whole.nbytes == 0 and same_bits(r.buf, whole.buf), f"{what}: the split launch differs from the whole one"
    assert same_bits(r.buf, _run(M, N, K, out, op, hint=hint, split=True, **kw).buf), f"{what}: two split launches differ"
    return r, whole


@pytest.mark.parametrize("hint", [0, 3])
@pytest.mark.parametrize("K", [1024, 4096, 1216, 1600])
def test_split_k_share_counts(K, hint):
    assert ref.split_k_shares(128, 128, K) == ref.SPLIT_K_CASES[(128, 128, K)]
    _check_split(f"split-K 128x128x{K} hint {hint}", 128, 128, K, "f32", hint=hint)


SPLIT_SHAPES = {"ragged": (77, 200, 4096), "tiles8": (128, 1024, 4096)}
SPLIT_OPS = ["none", "alpha2", "row_scale", "row_bias", "col_bias", "res_ldres", "res_scale_inplace", "rowadd"]
SPLIT_CASES = [(op, s, out) for op in SPLIT_OPS for s in SPLIT_SHAPES for out in DTYPES if not (op == "row_scale" and s == "ragged")]


@pytest.mark.parametrize("op,shape,out", SPLIT_CASES, ids=[f"{o}-{s}-{t}" for o, s, t in SPLIT_CASES])
def test_split_k_operators(op, shape, out):
    """Every operator set splitk_epilogue_kernel re-implements.  row_scale needs N % 128 == 0 (the launcher's rule): the 8-tile shape.
    The residual * res_scale case runs in place for f32 (res == C) and from its own buffer for bf16 (the residual is f32)."""
    M, N, K = SPLIT_SHAPES[shape]
    kw = {}
    if op == "res_scale_inplace":
        op, kw = ("res_scale_inplace", {"ldc": N + 4}) if out == "f32" else ("res_scale", {})
    _check_split(f"split-K {op} {shape} {out}", M, N, K, out, op, bmax=1, **kw)


@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("shape", list(SPLIT_SHAPES))
def test_split_k_gelu(shape, out):
    """gelu_erf for f32, gelu_poly2 for bf16, on an exact pre-activation."""
    M, N, K = SPLIT_SHAPES[shape]
    r, _ = _check_split(f"split-K gelu {shape} {out}", M, N, K, out, "gelu", bounded="gelu", bmax=1)
    assert (np.abs(r.v) < 4).mean() > 0.01, "some pre-activations must lie where GELU bends"


def test_split_k_bf16_copy_and_row_sums_of_squares():
    M, N, K = SPLIT_SHAPES["tiles8"]
    for op in ("col_bias", "res_scale"):
        r, whole = _check_split(f"split-K fused-norm outputs {op}", M, N, K, "f32", op, bmax=1, fused=True)
        for x in (r, whole):
            assert np.array_equal(x.cbf.contiguous().view(torch.int16).numpy().view(np.uint16), bf16_bits(x.got).reshape(M, N)), \
                "c_bf16 must be the bf16 of the stored f32"
            x2 = (x.got.double().numpy() ** 2).sum(1)
            worst = float((np.abs(x.slots.double().numpy().sum(1) - x2) / (N * U * x2)).max())
            print(f"row_sumsq {op}: max err / (N u sum x^2) {worst:.3f}")
            assert worst <= 1.0


FALLBACK = {"gadd": dict(op="gadd"), "aux": dict(act="gelu_aux", bounded="gelu_aux"), "silu": dict(act="silu", bounded="silu"),
            "res_and_rowadd": dict(op="rowadd_res"), "N % 4": dict(N=202, op="col_bias"), "bias_plus_one": dict(op="col_bias", bias_lead=1)}


@pytest.mark.parametrize("name", list(FALLBACK))
def test_split_k_fallback(name):
    """A descriptor the second launch cannot serve is not split: workspace bytes 0, and stream_k changes nothing."""
    kw = dict(FALLBACK[name])
    M, N, K = 77, kw.pop("N", 200), 4096
    bounded, op = kw.pop("bounded", None), kw.pop("op", "none")
    r = _run(M, N, K, "f32", op, hint=3, split=True, bmax=1, **kw)
    assert r.nbytes == 0, f"{name}: the planner split a launch its second kernel cannot finish"
    if bounded:
        assert_bounded(r.got, r.want, _act_bound(bounded, r, "f32"), name)
    else:
        assert_exact(r.got, r.want, name)
    assert r.untouched and same_bits(r.buf, _run(M, N, K, "f32", op, hint=3, bmax=1, **kw).buf)


# ------------------------------------------------------------------------------------------------
# (d) EXT operators on every tile kernel
# ------------------------------------------------------------------------------------------------
def _ext_cases():
    cases = []
    for hint in (1, 2, 3, 4):
        for shape, (M, N, K) in (("fast", (257, 384 if hint == 4 else 256, 256)), ("edge", (100, 260, 128))):
            for act in ("silu", "gelu_aux", "gelu_bwd", "exp2", "mul_aux"):
                cases.append((hint, shape, M, N, K, act, None))
            for act in PAIR:
                # fast: both 16-byte accessible.  edge: 130 and 134 are not (scalar branch), 136 is (the vector branch of epilogue_row4)
                for ldc in ((N // 2, N // 2 + 4) if shape == "fast" else (N // 2, N // 2 + 4, N // 2 + 6)):
                    cases.append((hint, shape, M, N, K, act, ldc))
    for hint in (1, 2):                                 # the scalar branch of every operator
        for act in ("silu", "gelu_aux", "gelu_bwd", "exp2", "mul_aux"):
            cases.append((hint, "scalar", 100, 260, 128, act, 262))
        for act in PAIR:
            cases.append((hint, "scalar", 100, 260, 128, act, 131))
    return cases


EXT_CASES = _ext_cases()
EXP2_WORST = {"f32": 0.0, "bf16": 0.0}


@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("hint,shape,M,N,K,act,ldc", EXT_CASES, ids=[f"hint{h}-{s}-{a}-ldc{l}" for h, s, _, _, _, a, l in EXT_CASES])
def test_ext_operators(hint, shape, M, N, K, act, ldc, out):
    """The pre-activation is exact, so the error seen is the activation's alone; the padding of C (and of aux) keeps its fill."""
    r = _run(M, N, K, out, hint=hint, act=act, ldc=ldc, bmax=1)
    assert r.got.shape[1] == (N // 2 if act in PAIR else N)
    assert np.abs(r.v).std() > 1, "pre-activations are meant to lie where the activation bends"
    worst = assert_bounded(r.got, r.want, _act_bound(act, r, out), f"{act} hint {hint} {shape} ldc {ldc} {out}")
    assert r.untouched, "a write outside C"
    if act == "exp2":
        EXP2_WORST[out] = max(EXP2_WORST[out], worst)
        print(f"EXP2 {out}: worst max err / bound so far {EXP2_WORST[out]:.3f}")
    if act == "gelu_aux":
        assert np.array_equal(r.aux_got.contiguous().view(torch.int16).numpy().view(np.uint16), bf16_bits(r.v.astype(np.float32)).reshape(M, N)), \
            "the stored pre-activation must be the bf16 of the exact value"
        assert r.aux_untouched, "a write into the padding of aux"
    assert same_bits(r.buf, _run(M, N, K, out, hint=hint, act=act, ldc=ldc, bmax=1).buf), "two launches differ"


@pytest.mark.parametrize("hint", [0, 2])
@pytest.mark.parametrize("T,Tp", [(70, 128), (256, 256)])
@pytest.mark.parametrize("act", ["exp2", "mul_aux"])
def test_ext_exp2_and_mul_aux_batched(act, T, Tp, hint):
    """The score GEMMs of the fused attention backward: batch1 = 2 x batch0 = 3 head slices of a [T, 3 h d] buffer, a ROW bias per
    (b1, b0) batch through sBias1 / sBias0, C (and MUL_AUX's factor) in rows of Tp: the pad columns T .. Tp stay untouched."""
    nb, h, dh = 2, 3, 64
    ld = 3 * h * dh
    g = np.random.default_rng(T + hint)
    qkv = _flat(g, nb * T * ld, 1)
    qkv[::3] *= 3                                                   # the A side up to 3, products stay integers
    a = (qkv, 0, ld, T * ld, dh)
    b = (qkv, h * dh, ld, T * ld, dh)
    rb = ref.sixty_fourths(g, nb * h * T + 8, lo=-24.0, hi=0.0) if act == "exp2" else ref.sixty_fourths(g, nb * h * T + 8)
    aux = torch.from_numpy(g.uniform(0.0, 1.0, nb * h * T * Tp).astype(np.float32)).bfloat16().float().numpy() if act == "mul_aux" else None
    for out in DTYPES:
        _run_batched(T, T, dh, nb, h, a, b, (nb * h * T * Tp, 0, Tp, h * T * Tp, T * Tp), out, hint=hint, bias=(rb, "row", h * T, T), act=act,
                     aux=aux, alpha=0.5)


@pytest.mark.parametrize("hint", [1, 2])
def test_gelu_far_from_zero(hint):
    """Column biases of -16 .. -8192 and +16 .. +8192 on an exact product: GELU is 0 (to 1e-57 and better) on the far negative side and
    v on the far positive one.  The packed polynomial of the bf16 form clamps its argument; v times the clamped Phi must go to 0 with
    it (it grew like 4e-6 |v| before the lower clamp moved onto the fit's zero: csrc/gemm_common.h, gelu_poly2)."""
    M, N, K = 100, 260, 64
    g = np.random.default_rng(hint)
    bias = np.resize(np.array([-16, -128, -1024, -8192, 0, 16, 128, 1024, 8192], dtype=np.float32), N)
    for out in DTYPES:
        _run_batched(M, N, K, 1, 1, (_flat(g, M * K, 3), 0, K, 0, 0), (_flat(g, N * K, 1), 0, K, 0, 0), (M * N, 0, N, 0, 0), out, hint=hint,
                     bias=(bias, "col", 0, 0), act="gelu")


# ------------------------------------------------------------------------------------------------
# (e) batches and gather on the NT kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", DTYPES)
@pytest.mark.parametrize("hint", [1, 2])
def test_nt_batches_with_padded_strides(hint, out):
    """batch1 = 3 x batch0 = 2, every stride larger than its matrix; a column bias per batch1 and a residual with sRes1 / sRes0."""
    M, N, K, b1n, b0n = 100, 260, 128, 3, 2
    g = np.random.default_rng(5 + hint)
    lda, ldb, ldc, ldres = K + 16, K + 32, N + 4, N + 8
    sA0, sB0, sC0, sR0 = M * lda + 32, N * ldb + 16, M * ldc + 12, M * ldres + 4
    sA1, sB1, sC1, sR1, sBi1 = 2 * sA0 + 64, 2 * sB0 + 48, 2 * sC0 + 4, 2 * sR0 + 8, N + 4
    _run_batched(M, N, K, b1n, b0n, (_flat(g, 3 * sA1, 3), 0, lda, sA1, sA0), (_flat(g, 3 * sB1, 3), 0, ldb, sB1, sB0),
                 (3 * sC1, 0, ldc, sC1, sC0), out, hint=hint, bias=(ref.sixty_fourths(g, 3 * sBi1), "col", sBi1, 0),
                 res=(ref.sixty_fourths(g, 3 * sR1), ldres, sR1, sR0))


@pytest.mark.parametrize("hint", [1, 2])
@pytest.mark.parametrize("flag", ["gather_a", "gather_b", "gather_bias"])
def test_nt_gather(flag, hint):
    """gather1 = [2, 0, 2] replaces the batch index of A, of B or of the bias; C (and only C) always follows the plain index."""
    M, N, K = 100, 260, 128
    g = np.random.default_rng(9 + hint)
    _run_batched(M, N, K, 3, 1, (_flat(g, 3 * M * K, 3), 0, K, M * K, 0), (_flat(g, 3 * N * K, 3), 0, K, N * K, 0), (3 * M * N, 0, N, M * N, 0),
                 "f32", hint=hint, bias=(ref.sixty_fourths(g, 3 * (N + 4)), "col", N + 4, 0), gather=[2, 0, 2], flag=flag)


# ------------------------------------------------------------------------------------------------
# (f) K-loop edges of the NT kernels
# ------------------------------------------------------------------------------------------------
NT_K = ([(1, 129, 129, K) for K in (64, 128, 192, 256)] + [(3, 129, 129, K) for K in (64, 128, 192, 256, 320, 512)]
        + [(2, 300, 512, K) for K in (64, 128, 192, 256, 512)] + [(4, 300, 384, K) for K in (64, 128, 192, 256, 512)]
        + [(2, 1024, 2048, 320), (4, 1024, 2048, 320)])


@pytest.mark.parametrize("hint,M,N,K", NT_K, ids=[f"hint{h}-{m}x{n}x{k}" for h, m, n, k in NT_K])
def test_nt_k_loop(hint, M, N, K):
    """Prologue, steady state and tail of the double-buffered (1), ring (3) and 8-wave (2, 4) loops; the 8-wave K rotation at nk = 5."""
    _check_exact_twice(f"nt hint {hint} {M}x{N}x{K}", M, N, K, hint=hint)


# ------------------------------------------------------------------------------------------------
# RANDOM inputs: one case per kernel family, per-element bound
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(M, N, K, tn):
    t = ref.random_inputs(M, N, K, trans_ab=tn)
    t["dev"] = {"a": _dev(t["a"], torch.bfloat16), "b": _dev(t["b"], torch.bfloat16), "bias": _dev(t["bias"]), "res": _dev(t["res"])}
    return t


def _run_random(M, N, K, *, tn, hint=0, split=False, addends=True, alpha=1.0):
    L = _L()
    t = _random(M, N, K, tn)
    c = Buf(M * N, "f32")
    c.region(0, M, N, N)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = t["dev"]["a"].data_ptr(), (M if tn else K), t["dev"]["b"].data_ptr(), (N if tn else K)
    d.C, d.ldc, d.c_dtype, d.alpha, d.trans_ab, d.tile_hint = c.ptr(), N, L.F32, alpha, int(tn), hint
    if addends:
        d.bias, d.bias_mode, d.res, d.ldres = t["dev"]["bias"].data_ptr(), L.BIAS_COL, t["dev"]["res"].data_ptr(), N
    nbytes = _split(d) if split else 0
    _launch(d)
    (got,), untouched = c.read()
    a = np.abs
    y = t["base"] * alpha
    bound = K * U * t["S"] * abs(alpha) + U * a(y)
    if addends:
        y = y + t["bias"].astype(np.float64)
        bound = bound + U * a(y)
        y = y + t["res"].astype(np.float64)
        bound = bound + U * a(y)
    assert untouched
    return got, y, bound, nbytes, c.buf


def test_random_transposed_operands():
    got, y, bound, _, _ = _run_random(1000, 296, 192, tn=True)
    assert_bounded(got, y, bound, "random TN 1000x296x192 bias + residual")


def test_random_split_k():
    got, y, bound, nbytes, buf = _run_random(77, 200, 4096, tn=False, hint=3, split=True)
    assert nbytes == 8 * 77 * 200 * 4
    assert_bounded(got, y, bound, "random split-K 77x200x4096 bias + residual")
    assert same_bits(buf, _run_random(77, 200, 4096, tn=False, hint=3, split=True)[4]), "two split launches differ"


def test_random_stream_k():
    """The plain product: the launcher refuses a bias or a residual on a stream-K launch."""
    got, y, bound, nbytes, buf = _run_random(264, 520, 22016, tn=True, split=True, addends=False, alpha=0.5)
    assert nbytes == 2 * 256 * 256 * 256 * 4
    assert_bounded(got, y, bound, "random stream-K 264x520x22016")
    assert same_bits(buf, _run_random(264, 520, 22016, tn=True, split=True, addends=False, alpha=0.5)[4]), "two split launches differ"
