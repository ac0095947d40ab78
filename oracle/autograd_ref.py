"""Float64 statements of the forward and of every gradient of the autograd functions of modeling_utils/autograd.py, the case tables
of tests/test_gpu_autograd_bounds.py and the per-element criteria both that test and tests/test_autograd_ref_host.py apply.  CPU only:
numpy and torch float64, no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Every reference is written from the mathematics of the function (y = x W^T + b,
its adjoints, the quotient rule of a normalisation, the softmax of a cross entropy), not from autograd.py; the host test pins each
of them to torch.autograd on a float64 graph.

A family is (CASES, inputs(case), reference / check(case, inputs, got)).  `got` is a dict of numpy arrays as the device returned
them: f32 arrays, and uint16 bit patterns for bf16 tensors.  check() returns [(name, ratio, where)]: for an EXACT quantity the ratio is
0 (same bits) or inf, for a BOUNDED one worst |err| / bound.  emulate(case, inputs) is the reference rounded the way the device
rounds (one rounding per stored tensor): what check() must pass, and what the faults of FAULTS perturb.

EXACT inputs (oracle.gemm_ref): activations, incoming gradients and weights are integers in [-3, 3], biases and residuals multiples
of 1/64 in [-2, 2], res_scale in {1/2, 1, 2}.  Every f32 result is then an integer or a multiple of 2^-7 that 24 bits hold, in any
summation order.  reductions(case) lists (what, length, is_exact(...)) per gradient: dx reduces over N, dw over M, db and drs over M.
"""

from __future__ import annotations

import math
import zlib

import numpy as np
import torch

from oracle.attention_ref import ratio_report
from oracle.gemm_ref import (bf16_value, exact_operands, gelu64, gelu_grad64, is_exact, plan_stream_k, power_of_two, product64,
                             sixty_fourths, tiles256)
from oracle.layout_ref import adaptive_avg_pool_adjoint, adaptive_pool_matrix, bf16_bits

U = 2.0**-24
BF_U = 2.0**-8
TINY = 2.0**-126
GELU_ABS = 8.3e-5        # test_gpu_gemm_bounds.py: GELU 1.13 bound + 8.3e-5
GELU_BWD_REL = 1e-4      # test_gpu_gemm_bounds.py: GELU_BWD |v| 1e-4 + u |y|
ROW_REL = 1e-5           # test_gpu_reductions.py: f32 results of f32 row reductions, relative to the row's largest magnitude


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def _ints(g, *shape, hi=3) -> np.ndarray:
    return g.integers(-hi, hi + 1, shape).astype(np.float32)


def values(a) -> np.ndarray:
    """float64 values of a device result: uint16 arrays are bf16 bit patterns."""
    a = np.asarray(a)
    return bf16_value(a) if a.dtype == np.uint16 else a.astype(np.float64)


def bf16r(x) -> np.ndarray:
    """float64 -> the float64 value of its bf16 rounding (through f32, as the device stores)."""
    return bf16_value(bf16_bits(np.asarray(x, dtype=np.float64).astype(np.float32)))


def f32r(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def as_stored(x64, like) -> np.ndarray:
    """The float64 reference as a device tensor of `like`'s kind would hold it: bf16 bits or f32."""
    f = np.asarray(x64, dtype=np.float64).astype(np.float32)
    return bf16_bits(f).reshape(f.shape) if like == "bf16" else f


# ------------------------------------------------------------------------------------------------
# the two criteria
# ------------------------------------------------------------------------------------------------
def exact(name: str, got, want64):
    """BIT equality of an f32 result with the float64 reference (which f32 must hold exactly), of a bf16 result with its
    round-to-nearest-even.  +0 and -0 count as equal.  (name, 0.0 or inf, first mismatch)."""
    got, want64 = np.asarray(got), np.asarray(want64, dtype=np.float64)
    if got.shape != want64.shape:
        return name, math.inf, ("shape", got.shape, want64.shape)
    w32 = want64.astype(np.float32)
    if got.dtype == np.uint16:
        same = got == bf16_bits(w32).reshape(w32.shape)
        same |= (bf16_value(got) == 0) & (w32 == 0)
    else:
        assert got.dtype == np.float32, f"{name}: {got.dtype}"
        assert (w32.astype(np.float64) == want64).all(), f"{name}: the reference is not an f32 value: the case is not EXACT"
        same = got.view(np.uint32) == w32.view(np.uint32)
        same |= (got == 0) & (w32 == 0)
    if same.all():
        return name, 0.0, ()
    return name, math.inf, tuple(int(i) for i in np.argwhere(~same)[0])


def bounded(name: str, got, want64, bound):
    """(name, worst |got - want| / bound, where) over ALL elements (oracle.attention_ref.ratio_report)."""
    g, w = values(got), np.asarray(want64, dtype=np.float64)
    if g.shape != w.shape:
        return name, math.inf, ("shape", g.shape, w.shape)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), w.shape) + TINY
    r, where = ratio_report(torch.from_numpy(np.ascontiguousarray(g)), torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(b.copy()))
    return name, r, where


def worst(results):
    return max(results, key=lambda r: r[1])


# ------------------------------------------------------------------------------------------------
# branch predicates, each stated once beside the line of autograd.py it mirrors
# ------------------------------------------------------------------------------------------------
def wgrad_reads_transposed(M, N, K, ld_dy, ld_x) -> bool:
    """autograd.wgrad_reads_transposed (the host test holds the two equal over a grid of shapes)."""
    return M % 64 == 0 and N % 8 == 0 and K % 8 == 0 and N >= 128 and K >= 128 and ld_dy % 8 == 0 and ld_x % 8 == 0


def fused_sums(dy_f32: bool, N: int) -> bool:
    """autograd.grad_sums_and_cast: `if dy.dtype != torch.float32 or N % 4:` takes the colsum / cast_bf16 fallback."""
    return dy_f32 and N % 4 == 0


def cast_takes_row_kernel(numel: int) -> bool:
    """autograd.cast_bf16: `if x.numel() % 4 and x.ndim == 2 and x.dtype == torch.float32:`."""
    return numel % 4 != 0


def voxel_batched(Cc: int, V: int) -> bool:
    """autograd.VoxelHead.backward: `if (Cc * V) % 4 == 0:` one batched GEMM + slab scatter sum, else the per-sample chain."""
    return (Cc * V) % 4 == 0


def scalenorm_bwd_register_kernel(D: int) -> bool:
    """csrc/backward.hip scalenorm_bwd_launch: first_nv<12, 3> with dim == 256 * nv (16-byte aligned rows), else the walk kernel."""
    return D in (3072, 768)


def stream_k_engages(M, N, K) -> bool:
    """Whether dw [N, K] = dy^T x with the reduction M is cut by the stream-K planner (oracle.gemm_ref.plan_stream_k)."""
    return plan_stream_k(tiles256(N, K), M // 64) is not None


def smallest_stream_k_M(N, K) -> int:
    M = 64
    while not stream_k_engages(M, N, K):
        M += 64
    return M


# ================================================================================================
# EXACT families
# ================================================================================================
# ---- Linear: y = x W^T + b + res * res_scale ---------------------------------------------------
def _lin(name, M, N, K, Kx=None, out_f32=True, bias=True, res="scaled", raw=False, dy_view="contig"):
    return {"name": name, "M": M, "N": N, "K": K, "Kx": Kx or K, "out_f32": out_f32, "bias": bias, "res": res, "raw": raw, "dy_view": dy_view}


STREAM_K_NK = (264, 576)                       # a ragged 6-tile dw: 2 x 3 tiles of 256^2
STREAM_K_M = smallest_stream_k_M(*STREAM_K_NK)   # 21888: 6 tiles x 342 K-steps >= 256 workers x 8

LINEAR_CASES = [
    _lin("trans_ab-64x128x128", 64, 128, 128),                                  # wgrad: the smallest transposed-operand shape; fused sums, both on
    _lin("M70", 70, 128, 128, bias=False),                                      # explicit transposes: M pad columns; fused sums: res only
    _lin("N100", 64, 100, 128, res=None),                                       # N % 8 != 0; Np = 128 != N; fused sums: want_sum only
    _lin("N120", 64, 120, 128, bias=False, res=None),                           # N < 128; Np = 128; fused sums: neither
    _lin("K64", 64, 128, 64),                                                   # K < 128
    _lin("N136", 64, 136, 128),                                                 # Np = 192 = ld_dy: transposed operands behind dense_bwd's pad
    _lin("N102-M65", 65, 102, 128),                                             # N % 4 != 0: colsum fallback; numel % 4 != 0: cast row kernel
    _lin("bf16-out", 64, 128, 128, out_f32=False, res=None),                    # bf16 dy: colsum fallback, cast hands it on
    _lin("K-padded", 64, 128, 100, Kx=128, res=None),                           # w [N, 100] behind x [M, 128]: dw[:, :100]
    _lin("raw-res-grad", 70, 128, 128, raw=True),                               # dres is dy itself
    _lin("res-unscaled", 64, 128, 128, res="plain"),                            # res without res_scale
    _lin("dy-columns-view", 64, 128, 128, dy_view="cols"),                      # incoming gradient: every second column of a wider tensor
    _lin("dy-transposed-view", 70, 100, 128, dy_view="t"),                      # incoming gradient: a transposed view
    _lin("stream-K-whole-M256", 256, *STREAM_K_NK, bias=False, res=None),       # same N, K: left whole
    _lin("stream-K", STREAM_K_M, *STREAM_K_NK, bias=False, res=None),           # the one large case
]


def linear_inputs(c):
    g = _rng("linear" + c["name"])
    M, N, K, Kx = c["M"], c["N"], c["K"], c["Kx"]
    x, w = exact_operands((M, Kx), (N, K), seed=int(g.integers(1 << 30)))
    x[:, K:] = 0
    t = {"x": x, "w": w, "dy": _ints(g, M, N)}
    if c["bias"]:
        t["b"] = sixty_fourths(g, N)
    if c["res"]:
        t["res"] = sixty_fourths(g, M, N)
    if c["res"] == "scaled":
        t["rs"] = power_of_two(g, N)
    return t


def linear_reference(c, t):
    K = c["K"]
    x, w, dy = (t[k].astype(np.float64) for k in ("x", "w", "dy"))
    y = product64(x[:, :K], w)
    if "b" in t:
        y = y + t["b"].astype(np.float64)[None, :]
    if "res" in t:
        y = y + t["res"].astype(np.float64) * (t["rs"].astype(np.float64)[None, :] if "rs" in t else 1.0)
    r = {"y": y, "dx": np.zeros((c["M"], c["Kx"])), "dw": dy.T @ x[:, :K]}
    r["dx"][:, :K] = dy @ w
    if "b" in t:
        r["db"] = dy.sum(0)
    if "res" in t:
        r["dres"] = dy * t["rs"].astype(np.float64)[None, :] if ("rs" in t and not c["raw"]) else dy
    if "rs" in t:
        r["drs"] = (dy * t["res"].astype(np.float64)).sum(0)
    return r


def linear_kinds(c):
    return {"y": "f32" if c["out_f32"] else "bf16", "dx": "bf16"}


def linear_route(c):
    """What the recorded launches of a Linear backward must show."""
    M, N, Kx = c["M"], c["N"], c["Kx"]
    Np = round_up(N, 64)
    trans = wgrad_reads_transposed(M, N, Kx, Np, Kx)
    fused = fused_sums(c["out_f32"], N)
    return {"Np": Np, "trans_ab": trans, "transposes": 0 if trans else 2, "fused_sums": fused,
            "colsums": 0 if fused else int(c["bias"]) + int(c["res"] == "scaled"), "casts": 0 if fused else 1,
            "cast_row_kernel": (not fused) and c["out_f32"] and cast_takes_row_kernel(M * N),
            "stream_k": trans and stream_k_engages(M, N, Kx)}


def linear_reductions(c):
    return [("y over K", c["K"], is_exact(c["K"], addends=True)), ("dx over Np", round_up(c["N"], 64), is_exact(round_up(c["N"], 64))),
            ("dw over M", round_up(c["M"], 64), is_exact(round_up(c["M"], 64))), ("db, drs over M", c["M"], sums_exact(c["M"], 6.0, 64))]


def sums_exact(n: int, top: float, per_unit: int) -> bool:
    """A sum of n multiples of 1 / per_unit of magnitude <= top: exact in f32, in any order, while n top per_unit < 2^24."""
    return n * top * per_unit < 2**24


def check_exact(ref, kinds, got):
    """Every key of the reference, bit for bit; a key the device did not return is a failure."""
    out = []
    for k, want in ref.items():
        if k not in got:
            out.append((k, math.inf, ("missing",)))
        else:
            out.append(exact(k, got[k], want))
    extra = set(got) - set(ref)
    assert not extra, f"the device returned gradients the reference has none for: {sorted(extra)}"
    return out


def emulate_exact(ref, kinds):
    return {k: as_stored(v, kinds.get(k, "f32")) for k, v in ref.items()}


# ---- QKVLinear: qkv = x [Wq; Wk; Wv]^T ---------------------------------------------------------
QKV_CASES = [{"name": "3N192-M128", "M": 128, "N": 64, "K": 128},       # 3N % 64 == 0; wgrad: transposed operands
             {"name": "3N96-M70", "M": 70, "N": 32, "K": 64},           # 3N = 96: the dgrad operand padded to 128; explicit transposes
             {"name": "3N96-M64", "M": 64, "N": 32, "K": 128}]
QKV_WEIGHT_MAX = {"wq": 3, "wk": 2, "wv": 1}      # three ranges: a permuted slice shows in the magnitudes, too


def qkv_inputs(c):
    g = _rng("qkv" + c["name"])
    M, N, K = c["M"], c["N"], c["K"]
    t = {"x": _ints(g, M, K), "dy": _ints(g, M, 3 * N), "wk2": _ints(g, N, K)}    # wk2: written over wk before the second pass
    for k, hi in QKV_WEIGHT_MAX.items():
        t[k] = _ints(g, N, K, hi=hi)
    return t


def qkv_reference(c, t, second=False):
    N = c["N"]
    x, dy = t["x"].astype(np.float64), t["dy"].astype(np.float64)
    ws = [t["wq"], t["wk2"] if second else t["wk"], t["wv"]]
    W = np.concatenate(ws).astype(np.float64)
    r = {"y": product64(x, W), "dx": dy @ W}
    for i, k in enumerate(("dwq", "dwk", "dwv")):
        r[k] = dy[:, i * N:(i + 1) * N].T @ x
    return r


QKV_KINDS = {"y": "bf16", "dx": "bf16"}


def qkv_route(c):
    N3 = 3 * c["N"]
    Np = round_up(N3, 64)
    trans = wgrad_reads_transposed(c["M"], N3, c["K"], Np, c["K"])
    return {"Np": Np, "trans_ab": trans, "transposes": 0 if trans else 2}


def qkv_reductions(c):
    Np = round_up(3 * c["N"], 64)
    Mp = round_up(c["M"], 64)
    return [("y over K", c["K"], is_exact(c["K"])), ("dx over 3N", Np, is_exact(Np)), ("dw over M", Mp, is_exact(Mp))]


# ---- ProjectorFuse: y = feat W^T + b -----------------------------------------------------------
PROJECTOR_CASES = [{"name": "K100-M70-bias", "M": 70, "N": 128, "K": 100, "bias": True},
                   {"name": "K128-M128", "M": 128, "N": 128, "K": 128, "bias": False},
                   {"name": "K100-M128-bias", "M": 128, "N": 128, "K": 100, "bias": True},
                   {"name": "K128-M70", "M": 70, "N": 128, "K": 128, "bias": False}]


def projector_inputs(c):
    g = _rng("projector" + c["name"])
    M, N, K = c["M"], c["N"], c["K"]
    feat = _ints(g, M, round_up(K, 64))
    feat[:, K:] = 0
    t = {"feat": feat, "w": _ints(g, N, K), "dy": _ints(g, M, N)}
    if c["bias"]:
        t["b"] = sixty_fourths(g, N)
    return t


def projector_reference(c, t):
    K = c["K"]
    f, w, dy = (t[k].astype(np.float64) for k in ("feat", "w", "dy"))
    r = {"y": product64(f[:, :K], w) + (t["b"].astype(np.float64)[None, :] if "b" in t else 0.0), "dw": dy.T @ f[:, :K]}
    if "b" in t:
        r["db"] = dy.sum(0)
    return r


def projector_route(c):
    Kp = round_up(c["K"], 64)
    trans = wgrad_reads_transposed(c["M"], c["N"], Kp, c["N"], Kp)
    return {"trans_ab": trans, "transposes": 0 if trans else 2, "colsums": int(c["bias"]), "casts": 1}


def projector_reductions(c):
    return [("y over K", c["K"], is_exact(c["K"], addends=True)), ("dw over M", round_up(c["M"], 64), is_exact(round_up(c["M"], 64))),
            ("db over M", c["M"], sums_exact(c["M"], 3.0, 1))]


# ---- VoxelHead followed by AdaptivePool --------------------------------------------------------
def _vox(name, T, Tout, Cc, Cp, V, S, subjects, bias=True):
    return {"name": name, "B": len(subjects), "T": T, "Tout": Tout, "Cc": Cc, "Cp": Cp, "V": V, "S": S, "subjects": subjects, "bias": bias}


# T_out is chosen so that every pool window holds two inputs (40 -> 32, 64 -> 48: T_out does not divide T_in, the windows overlap):
# the adjoint of an integer gradient is then a multiple of 1/2 that bf16 holds, and the case stays EXACT
VOXEL_CASES = [
    _vox("T40-C100in128-V20", 40, 32, 100, 128, 20, 3, (2, 0, 2)),                 # batched; Cp != Cc; a repeat; subject 1 unused
    _vox("T64-C64-V23-nobias", 64, 48, 64, 64, 23, 3, (1, 1, 0), bias=False),      # batched; Cp == Cc; subject 2 unused
    _vox("T40-C99in128-V23-chain", 40, 32, 99, 128, 23, 3, (0, 2, 0, 2)),          # (Cc V) % 4 != 0: the per-sample chain
    _vox("T64-C101in128-V65-chain", 64, 48, 101, 128, 65, 2, (1, 1, 1)),           # the chain; V > 64; subject 0 unused
    _vox("T40-C100in128-V65", 40, 32, 100, 128, 65, 4, (3, 0, 3, 1)),              # batched; V > 64
]


def voxel_inputs(c):
    g = _rng("voxel" + c["name"])
    B, T, Cc, Cp, V, S = (c[k] for k in ("B", "T", "Cc", "Cp", "V", "S"))
    x = _ints(g, B, T, Cp)
    x[:, :, Cc:] = 0
    t = {"x": x, "w": _ints(g, S, Cc, V), "subjects": np.array(c["subjects"], dtype=np.int64), "g": _ints(g, B, V, c["Tout"])}
    if c["bias"]:
        t["bias"] = sixty_fourths(g, S, V)
    return t


def voxel_reference(c, t):
    """y[b, v, t] = sum_c x[b, t, c] W[s_b, c, v] + bias[s_b, v]; pooled = y P^T; the gradients of <pooled, g>."""
    Cc, S = c["Cc"], c["S"]
    x, w, g = (t[k].astype(np.float64) for k in ("x", "w", "g"))
    s = t["subjects"]
    y = np.einsum("btc,bcv->bvt", x[:, :, :Cc], w[s])
    if "bias" in t:
        y = y + t["bias"].astype(np.float64)[s][:, :, None]
    P = adaptive_pool_matrix(c["T"], c["Tout"]).numpy()
    dy = adaptive_avg_pool_adjoint(torch.from_numpy(g), c["T"]).numpy()
    dx = np.zeros(x.shape)
    dx[:, :, :Cc] = np.einsum("bvt,bcv->btc", dy, w[s])
    dwb = np.einsum("btc,bvt->bcv", x[:, :, :Cc], dy)
    dw = np.zeros(w.shape)
    r = {"y": y, "pooled": y @ P.T, "dx": dx, "dw": dw}
    for b, sb in enumerate(s):
        dw[sb] += dwb[b]
    if "bias" in t:
        r["db"] = np.zeros((S, c["V"]))
        for b, sb in enumerate(s):
            r["db"][sb] += dy[b].sum(1)
    return r


def voxel_route(c):
    return {"batched": voxel_batched(c["Cc"], c["V"]), "gemms": 2 if voxel_batched(c["Cc"], c["V"]) else 1 + c["B"], "transposes": 1}


def voxel_reductions(c):
    Vp, Tp = round_up(c["V"], 64), round_up(c["T"], 64)
    P = adaptive_pool_matrix(c["T"], c["Tout"]).numpy()
    halves = bool(np.isin(P, (0.0, 0.5)).all()) and c["Tout"] and c["T"] % c["Tout"] != 0
    return [("every pool window holds two inputs", 2, halves), ("y over C", c["Cp"], is_exact(c["Cp"], addends=True)),
            ("dx over V", Vp, is_exact(Vp)), ("dW over T, then over the samples", Tp * c["B"], is_exact(Tp * c["B"])),
            ("db over T and samples", c["T"] * c["B"], sums_exact(c["T"] * c["B"], 3.0, 2))]


# ---- PackRows ----------------------------------------------------------------------------------
PACKROWS_CASES = [{"name": "f32-K100", "M": 37, "K": 100, "dtype": "f32"},          # tribe_pack_weight_bf16: cast + zero pad
                  {"name": "bf16-K128", "M": 37, "K": 128, "dtype": "bf16"},        # handed on as it lies
                  {"name": "bf16-K100", "M": 37, "K": 100, "dtype": "bf16"}]        # tribe_pack_features with T = 1


def packrows_inputs(c):
    g = _rng("packrows" + c["name"])
    M, K = c["M"], c["K"]
    x = g.standard_normal((M, K)).astype(np.float32)
    if c["dtype"] == "bf16":
        x = bf16r(x).astype(np.float32)
    return {"x": x, "dy": bf16r(g.standard_normal((M, round_up(K, 64)))).astype(np.float32)}


def packrows_reference(c, t):
    """The operand: x rounded to bf16 with zero pad columns; the gradient: the leading K columns, in x's type (f32 holds a bf16 exactly)."""
    y = np.zeros((c["M"], round_up(c["K"], 64)))
    y[:, :c["K"]] = bf16r(t["x"])
    return {"y": y, "dx": t["dy"][:, :c["K"]].astype(np.float64)}


def packrows_kinds(c):
    return {"y": "bf16", "dx": c["dtype"]}


# ================================================================================================
# BOUNDED families
# ================================================================================================
# ---- FeedForward: out = gelu(x W1^T + b1) W2^T + b2 + res * res_scale --------------------------
def _ff(name, M, raw, rs, dense=False):
    return {"name": name, "M": M, "D": 128, "Fh": 256, "raw": raw, "rs": rs, "dense": dense}


FF_CASES = [_ff("M70-raw-rs", 70, True, True), _ff("M128-rs", 128, False, True), _ff("M70-no-rs", 70, False, False),
            _ff("M128-raw-no-rs", 128, True, False), _ff("M70-pre-within-6", 70, False, True, dense=True)]


def ff_inputs(c):
    """x, dout integers; W1 in [-1, 1] and K = D <= 256: pre = x W1^T + b1 is exact in f32.  W2 integers: dout W2 is an exact integer.
    dense: W1 keeps 2 entries per row, so that pre (a sum of 2 products and a bias) lies within [-6, 6] mostly, where gelu' bends."""
    g = _rng("ff" + c["name"])
    M, D, Fh = c["M"], c["D"], c["Fh"]
    w1 = _ints(g, Fh, D, hi=1)
    if c["dense"]:
        keep = np.zeros((Fh, D), dtype=bool)
        for r in range(Fh):
            keep[r, g.choice(D, 2, replace=False)] = True
        w1 = np.where(keep, np.where(w1 == 0, 1.0, w1), 0.0).astype(np.float32)
    t = {"x": _ints(g, M, D), "w1": w1, "b1": sixty_fourths(g, Fh), "w2": _ints(g, D, Fh), "b2": sixty_fourths(g, D),
         "res": sixty_fourths(g, M, D), "dout": _ints(g, M, D)}
    if c["rs"]:
        t["rs"] = power_of_two(g, D)
    return t


def ff_stages(c, t, pre_dev=None, h_dev=None, fault=None):
    """float64 of every stage.  pre_dev / h_dev: the values the device stored (None: the float64 ones, for the full reference)."""
    x, w1, b1, w2, b2, res, dout = (t[k].astype(np.float64) for k in ("x", "w1", "b1", "w2", "b2", "res", "dout"))
    rs = t["rs"].astype(np.float64)[None, :] if "rs" in t else 1.0
    v = x @ w1.T + b1[None, :]                       # exact
    pre = v if pre_dev is None else pre_dev
    h = gelu64(v) if h_dev is None else h_dev
    s = {"v": v, "gelu": gelu64(v), "out": h @ w2.T + b2[None, :] + res * rs,
         "S_out": np.abs(h) @ np.abs(w2).T + np.abs(b2)[None, :] + np.abs(res * rs)}
    dh = dout @ w2                                   # exact integers
    s["dh"] = dh
    s["dpre"] = dh * gelu_grad64(h if fault == "gelu_grad_at_h" else pre)
    s["dw2"], s["S_dw2"] = dout.T @ h, np.abs(dout).T @ np.abs(h)
    s["db2"] = dout.sum(0)
    s["dres"] = dout if (c["raw"] or "rs" not in t) else dout * rs
    if "rs" in t:
        s["drs"] = (dout * res).sum(0)
    s["db1"], s["dx"], s["dw1"] = s["dpre"].sum(0), s["dpre"] @ w1, s["dpre"].T @ x
    return s


def ff_emulate(c, t, fault=None):
    v = ff_stages(c, t)["v"]
    pre, h = bf16r(v), bf16r(gelu64(v))
    s = ff_stages(c, t, pre, h, fault=fault)
    dpre = bf16r(s["dpre"])
    x, w1 = t["x"].astype(np.float64), t["w1"].astype(np.float64)
    got = {"pre": bf16_bits(pre.astype(np.float32)), "h": bf16_bits(h.astype(np.float32)), "out": f32r(s["out"]).astype(np.float32),
           "dx": bf16_bits((dpre @ w1).astype(np.float32)), "dw1": (dpre.T @ x).astype(np.float32), "db1": dpre.sum(0).astype(np.float32),
           "dw2": s["dw2"].astype(np.float32), "db2": s["db2"].astype(np.float32), "dres": s["dres"].astype(np.float32)}
    if "drs" in s:
        got["drs"] = s["drs"].astype(np.float32)
    return got


def ff_check(c, t, got):
    """Stage by stage from the device's own pre and h.
      pre   EXACT: the f32 pre-activation is exact, its bf16 store one round-to-nearest-even
      h     GELU of an exact argument: 8.3e-5, then the bf16 store 2^-8 (|y| + 8.3e-5)
      out   h_dev W2^T + b2 + res rs: accumulation Fh u S, three more f32 operations u S each (S includes |b2| and |res rs|)
      dres, db2, drs   EXACT (integers times powers of two; sums of multiples of 1/64)
      dw2   dout^T h_dev: accumulation M_pad u S
      dpre  (not observable) = dh gelu'(pre_dev), dh an exact integer: E = |dh| 1e-4 + u |y|, then the bf16 store 2^-8 (|y| + that)
      db1   column sums of dpre_dev: sum_m E + M u sum_m (|dpre| + E)
      dx    dpre_dev W1 (bf16): E |W1| + Fh u (|dpre| + E) |W1|, then the bf16 store 2^-8 (|dx| + that)
      dw1   dpre_dev^T x: E^T |x| + M_pad u (|dpre| + E)^T |x|"""
    M, Fh = c["M"], c["Fh"]
    Mp = round_up(M, 64)
    s0 = ff_stages(c, t)
    out = [exact("pre", got["pre"], s0["v"])]
    e_g = GELU_ABS
    out.append(bounded("h", got["h"], s0["gelu"], e_g + BF_U * (np.abs(s0["gelu"]) + e_g)))
    s = ff_stages(c, t, values(got["pre"]), values(got["h"]))
    out.append(bounded("out", got["out"], s["out"], (Fh + 3) * U * s["S_out"]))
    out += [exact("dres", got["dres"], s["dres"]), exact("db2", got["db2"], s["db2"])]
    if "drs" in s:
        out.append(exact("drs", got["drs"], s["drs"]) if "drs" in got else ("drs", math.inf, ("missing",)))
    out.append(bounded("dw2", got["dw2"], s["dw2"], (Mp + 1) * U * s["S_dw2"]))
    a = np.abs(s["dpre"])
    e0 = np.abs(s["dh"]) * GELU_BWD_REL + U * a
    E = e0 + BF_U * (a + e0)
    w1a, xa = np.abs(t["w1"].astype(np.float64)), np.abs(t["x"].astype(np.float64))
    out.append(bounded("db1", got["db1"], s["db1"], E.sum(0) + (M + 1) * U * (a + E).sum(0)))
    bx = E @ w1a + (Fh + 1) * U * ((a + E) @ w1a)
    out.append(bounded("dx", got["dx"], s["dx"], bx + BF_U * (np.abs(s["dx"]) + bx)))
    out.append(bounded("dw1", got["dw1"], s["dw1"], E.T @ xa + (Mp + 1) * U * ((a + E).T @ xa)))
    return out


def ff_pre_coverage(c, t) -> float:
    """Fraction of the pre-activations within [-6, 6]."""
    return float((np.abs(ff_stages(c, t)["v"]) <= 6).mean())


# ---- ScaleNorm / ScaleNormFork -----------------------------------------------------------------
SN_ROWS = 37
SN_EPS = 1e-5
# D on either side of the switch of scalenorm_bwd_launch: 768 takes the register kernel, 512 the walk kernel
SCALENORM_CASES = [{"name": f"{fn}-D{D}-{'f32' if f32 else 'bf16'}{'-' + use if fn == 'fork' else ''}{'-rs' if rs else ''}", "fn": fn, "D": D,
                    "out_f32": f32, "use": use, "rs": rs}
                   for fn, D, f32, use, rs in [
                       ("norm", 768, False, "norm", False), ("norm", 768, True, "norm", False), ("norm", 512, False, "norm", False),
                       ("norm", 512, True, "norm", False),
                       ("fork", 768, False, "both", True), ("fork", 512, False, "both", True), ("fork", 768, False, "both", False),
                       ("fork", 512, False, "norm", True),            # dxr is None: the residual branch unused
                       ("fork", 768, False, "res", True), ("fork", 512, False, "res", False)]]   # dy is None: the normed branch unused


def scalenorm_inputs(c):
    g = _rng("scalenorm" + c["name"])
    D = c["D"]
    x = (g.standard_normal((SN_ROWS, D)) * np.logspace(-1, 1, SN_ROWS)[:, None]).astype(np.float32)
    dy = g.standard_normal((SN_ROWS, D)).astype(np.float32)
    t = {"x": x, "g": np.array([1.3], dtype=np.float32), "gs": float(np.float32(D**0.5)), "eps": float(np.float32(SN_EPS)),
         "dy": dy if c["out_f32"] else bf16r(dy).astype(np.float32), "dxr": (2 * g.standard_normal((SN_ROWS, D))).astype(np.float32)}
    if c["rs"]:
        t["rs"] = (0.5 + g.random(D)).astype(np.float32)
    return t


def scalenorm_fwd64(x, g, gs, eps):
    """y = x / max(|x|, eps) * gs * g."""
    inv = 1.0 / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), eps)
    return x * inv * (gs * g)


def scalenorm_bwd64(x, dy, g, gs, eps):
    """(dx, dg, per-row dot magnitudes) of y = x s / |x|, s = gs g: dx = s / |x| (dy - x <x, dy> / |x|^2) (the projection drops
    below eps, where y = x s / eps is linear); dg = gs sum_rows <x, dy> / max(|x|, eps)."""
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    inv = 1.0 / np.maximum(n, eps)
    dot = (x * dy).sum(-1, keepdims=True)
    proj = np.where(n < eps, 0.0, dot * inv * inv)
    return gs * g * inv * (dy - x * proj), float((gs * dot * inv).sum()), np.abs(x * dy).sum(-1, keepdims=True), inv


def scalenorm_reference(c, t):
    x, g = t["x"].astype(np.float64), float(t["g"][0])
    dy = t["dy"].astype(np.float64) if c["use"] != "res" else np.zeros_like(x)
    r = {"y": scalenorm_fwd64(x, g, t["gs"], t["eps"])}
    dx, dg, absdot, inv = scalenorm_bwd64(x, dy, g, t["gs"], t["eps"])
    if c["fn"] == "fork" and c["use"] != "norm":
        dx = dx + t["dxr"].astype(np.float64) * (t["rs"].astype(np.float64)[None, :] if "rs" in t else 1.0)
    r.update(dx=dx, dg=np.array([dg]), _absdot=absdot, _inv=inv)
    return r


def scalenorm_check(c, t, got):
    """y    the f32 value within 1e-5 of the row's largest magnitude (test_gpu_reductions.py), the bf16 store 2^-8 |y| more
       dx   1e-5 of the row's largest magnitude, plus the error of the f32 dot <x, dy> (chains of k = ceil(D / 64) + 9 adds):
            s / |x| |x_i| k u sum|x dy| / |x|^2 (test_gpu_reductions.py::test_scalenorm_bwd)
       dg   a fixed-order f32 sum over the rows of gs <x, dy> / |x|: (k + rows + 2) u sum over rows and columns of gs |x_i dy_i| / |x|"""
    r = scalenorm_reference(c, t)
    D = c["D"]
    k = -(-D // 64) + 9
    s = float(t["g"][0]) * t["gs"]
    rowmax = lambda a: np.abs(a).max(-1, keepdims=True)       # noqa: E731
    by = ROW_REL * rowmax(r["y"]) + (0.0 if c["out_f32"] else BF_U * np.abs(r["y"]))
    floor = s * r["_inv"] * np.abs(t["x"].astype(np.float64)) * (k * U * r["_absdot"] * r["_inv"] ** 2)
    out = [bounded("y", got["y"], r["y"], by), bounded("dx", got["dx"], r["dx"], ROW_REL * rowmax(r["dx"]) + floor)]
    if "dg" in got or c["use"] != "res":
        terms = float((t["gs"] * r["_absdot"] * r["_inv"]).sum())
        out.append(bounded("dg", got["dg"], r["dg"], np.array([(k + SN_ROWS + 2) * U * terms])))
    return out


def scalenorm_emulate(c, t):
    r = scalenorm_reference(c, t)
    return {"y": as_stored(r["y"], "f32" if c["out_f32"] else "bf16"), "dx": r["dx"].astype(np.float32), "dg": r["dg"].astype(np.float32)}


# ---- InfoNCE -----------------------------------------------------------------------------------
INFONCE_TAU = 0.07                                   # not a power of two
INFONCE_CASES = [{"name": f"N{N}-H{H}", "N": N, "H": H} for N, H in [(64, 64), (70, 128), (64, 128), (70, 64)]]
INFONCE_G = 1.5                                      # upstream gradient


def infonce_inputs(c):
    g = _rng("infonce" + c["name"])
    q = g.standard_normal((c["N"], c["H"])).astype(np.float32)
    k = (0.6 * q + g.standard_normal((c["N"], c["H"]))).astype(np.float32)      # matched pairs correlate: the diagonal stands out
    return {"q": q, "k": k, "alpha": float(np.float32(1.0 / INFONCE_TAU)), "gs": float(np.float32(np.float32(INFONCE_G) / np.float32(INFONCE_TAU)))}


def _lse(S, axis):
    m = S.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(S - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def infonce_loss64(S, lse_r, lse_c):
    d = np.diagonal(S)
    return 0.5 * ((lse_r - d).mean() + (lse_c - d).mean())


def infonce_dlogits64(S, lse_r, lse_c, gs):
    """d loss / d (qn . kn) times the upstream gradient: gs / (2 N) (softmax over rows + softmax over columns - 2 I), gs = g / tau."""
    N = S.shape[0]
    return gs * 0.5 / N * (np.exp(S - lse_r[:, None]) + np.exp(S - lse_c[None, :]) - 2 * np.eye(N))


def normalize_bwd64(x, dy):
    """The gradient of x / |x|: (dy - xn <xn, dy>) / |x|."""
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    xn = x / n
    return (dy - xn * (xn * dy).sum(-1, keepdims=True)) / n


def infonce_full64(t, tau_twice=False):
    """The whole function in float64 from q and k (no intermediate rounded)."""
    q, k = t["q"].astype(np.float64), t["k"].astype(np.float64)
    qn, kn = q / np.linalg.norm(q, axis=-1, keepdims=True), k / np.linalg.norm(k, axis=-1, keepdims=True)
    S = qn @ kn.T * t["alpha"]
    lr, lc = _lse(S, 1), _lse(S, 0)
    dL = infonce_dlogits64(S, lr, lc, t["gs"] * (t["alpha"] if tau_twice else 1.0))
    return {"qn": qn, "kn": kn, "S": S, "lse_r": lr, "lse_c": lc, "loss": infonce_loss64(S, lr, lc), "dq": normalize_bwd64(q, dL @ kn),
            "dk": normalize_bwd64(k, dL.T @ qn)}


def infonce_emulate(c, t, tau_twice=False):
    q, k = t["q"].astype(np.float64), t["k"].astype(np.float64)
    qn, kn = bf16r(q / np.linalg.norm(q, axis=-1, keepdims=True)), bf16r(k / np.linalg.norm(k, axis=-1, keepdims=True))
    S = f32r(qn @ kn.T * t["alpha"])
    lr, lc = f32r(_lse(S, 1)), f32r(_lse(S, 0))
    dL = bf16r(infonce_dlogits64(S, lr, lc, t["gs"] * (t["alpha"] if tau_twice else 1.0)))
    return {"qn": bf16_bits(qn.astype(np.float32)), "kn": bf16_bits(kn.astype(np.float32)), "S": S.astype(np.float32), "lse_r": lr.astype(np.float32),
            "lse_c": lc.astype(np.float32), "loss": np.array(infonce_loss64(S, lr, lc), dtype=np.float32).reshape(1),
            "dq": normalize_bwd64(q, f32r(dL @ kn)).astype(np.float32), "dk": normalize_bwd64(k, f32r(dL.T @ qn)).astype(np.float32)}


def infonce_check(c, t, got):
    """Stage by stage from the device's own qn, kn, S, lse_r, lse_c.
      qn, kn   ScaleNorm forward to bf16: 1e-5 of the row's largest magnitude + 2^-8 |y|
      S        alpha qn_dev kn_dev^T: accumulation H u sum|.|, then alpha and the store, u each
      lse_r    1e-5 max(|lse|, the row's largest |S|) (test_gpu_reductions.py)
      lse_c    the same over the columns, plus the difference between S^T as the second GEMM computed it and the stored S: the bound of S
      loss     f32 host glue over N terms: (N + 4) u (mean|lse_r| + mean|lse_c| + 2 mean|diag|)
      dL       (not observable) exp of an f32 argument a: (2 |a| + 6) u relative, the cancellation on the diagonal 4 u (test_gpu_reductions.py),
               then the bf16 store: E_L = floor + 2^-8 (|dL| + floor)
      dqn      dL_dev kn_dev (not observable): E_q = E_L |kn| + (Np + 1) u (|dL| + E_L) |kn|
      dq       the normalisation's backward, linear in dqn: (E_q + |qn| <|qn|, E_q>) / |q| carried through, plus the kernel's own
               1e-5 of the row's largest magnitude and its dot term (k = ceil(H / 64) + 9)"""
    N, H = c["N"], c["H"]
    Np = round_up(N, 64)
    q, k = t["q"].astype(np.float64), t["k"].astype(np.float64)
    f = infonce_full64(t)
    rowmax = lambda a: np.abs(a).max(-1, keepdims=True)       # noqa: E731
    out = [bounded(n, got[n], f[n], ROW_REL * rowmax(f[n]) + BF_U * np.abs(f[n])) for n in ("qn", "kn")]
    qn, kn, S, lr, lc = (values(got[n]) for n in ("qn", "kn", "S", "lse_r", "lse_c"))
    a = t["alpha"]
    bS = (H + 2) * U * a * (np.abs(qn) @ np.abs(kn).T)
    out.append(bounded("S", got["S"], qn @ kn.T * a, bS))
    out.append(bounded("lse_r", got["lse_r"], _lse(S, 1), ROW_REL * np.maximum(np.abs(_lse(S, 1)), np.abs(S).max(1))))
    out.append(bounded("lse_c", got["lse_c"], _lse(S, 0), ROW_REL * np.maximum(np.abs(_lse(S, 0)), np.abs(S).max(0)) + bS.max(0)))
    d = np.abs(np.diagonal(S))
    out.append(bounded("loss", got["loss"], np.array([infonce_loss64(S, lr, lc)]),
                       np.array([(N + 4) * U * (np.abs(lr).mean() + np.abs(lc).mean() + 2 * d.mean())])))
    kk = t["gs"] * 0.5 / N
    ar, ac = S - lr[:, None], S - lc[None, :]
    pr, pc = np.exp(ar), np.exp(ac)
    dL = kk * (pr + pc - 2 * np.eye(N))
    floor = kk * U * (pr * (2 * np.abs(ar) + 6) + pc * (2 * np.abs(ac) + 6) + 4 * np.eye(N))
    EL = floor + BF_U * (np.abs(dL) + floor)
    kdot = -(-H // 64) + 9
    for name, x, xn, dLm, ELm in (("dq", q, kn, dL, EL), ("dk", k, qn, dL.T, EL.T)):
        dn = dLm @ xn
        Eq = ELm @ np.abs(xn) + (Np + 1) * U * ((np.abs(dLm) + ELm) @ np.abs(xn))
        n = np.linalg.norm(x, axis=-1, keepdims=True)
        xh = np.abs(x) / n
        want = normalize_bwd64(x, dn)
        carried = (Eq + xh * (xh * Eq).sum(-1, keepdims=True)) / n
        own = ROW_REL * rowmax(want) + xh / n * kdot * U * (np.abs(x * dn).sum(-1, keepdims=True) / n)
        out.append(bounded(name, got[name], want, carried + own))
    return out


# ---- PearsonLossFn -----------------------------------------------------------------------------
PEARSON_G = 0.75
PEARSON_CASES = [{"name": f"B{B}-V{V}-T{T}-{layout}-{red}", "B": B, "V": V, "T": T, "layout": layout, "reduction": red}
                 for B, V, T, layout, red in [(3, 37, 20, "bvt", "mean"), (3, 37, 20, "bvt", "sum"), (3, 37, 20, "view", "mean"),
                                              (3, 37, 20, "view", "sum"), (2, 1, 30, "bvt", "mean"), (2, 1, 30, "view", "sum")]]
# layout "view": the [1, V, B T] transposed view of a '(b t) v' matrix that pl_module passes (strides (., 1, V))


def pearson_inputs(c):
    g = _rng("pearson" + c["name"])
    B, V, T = c["B"], c["V"], c["T"]
    pred = g.standard_normal((B, V, T)).astype(np.float32)
    true = (0.5 * pred + g.standard_normal((B, V, T))).astype(np.float32)
    if V > 1:
        pred[:, 0] = 1.7                              # one voxel constant in pred
    return {"pred": pred, "true": true}


def pearson_reference(c, t):
    """loss = g * reduce_v (1 - r_v), r_v = cov / (sx sy + 1e-8) over the (b, t) samples of voxel v, and its gradient
    d/dx = -k / den (yc - cov sy / (sx den) xc), k = g (1 / V for the mean).  Convention for a voxel constant in pred (sx = 0):
    cov = 0, r = 0 and the gradient keeps the finite term -k / den yc alone (modeling_utils/losses/losses.py, PearsonLoss)."""
    V = c["V"]
    x = t["pred"].astype(np.float64).transpose(1, 0, 2).reshape(V, -1)
    y = t["true"].astype(np.float64).transpose(1, 0, 2).reshape(V, -1)
    xc, yc = x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)
    sx, sy = np.sqrt((xc * xc).sum(1)), np.sqrt((yc * yc).sum(1))
    const = np.ptp(x, axis=1) == 0
    sx = np.where(const, 0.0, sx)
    cov = np.where(const, 0.0, (xc * yc).sum(1))
    den = sx * sy + 1e-8
    k = PEARSON_G * (1.0 / V if c["reduction"] == "mean" else 1.0)
    a = k / den
    cc = np.where(sx > 0, k * cov * sy / (np.where(sx > 0, sx, 1.0) * den * den), 0.0)
    grad = -a[:, None] * yc + cc[:, None] * xc
    loss = (1 - cov / den)
    loss = loss.mean() if c["reduction"] == "mean" else loss.sum()
    B, T = c["B"], c["T"]
    bound = 1e-4 * np.abs(grad) + (24 * U * (np.abs(a) * np.abs(y).max(1) + np.abs(cc) * np.abs(x).max(1)))[:, None]
    back = lambda m: m.reshape(V, B, T).transpose(1, 0, 2)    # noqa: E731
    return {"loss": np.array([loss]), "grad": back(grad), "_grad_bound": back(bound)}


def pearson_check(c, t, got):
    """loss   f64 statistics, per-voxel f32 roundings of the roots, the eps add and the quotient: 2e-6 per voxel (x V when summed)
       grad   1e-4 relative + 24 u (|a| max|y| + |c| max|x|) (test_gpu_reductions.py::test_pearson_loss_fwd_bwd), times the upstream g"""
    r = pearson_reference(c, t)
    tol = 2e-6 * (1 if c["reduction"] == "mean" else c["V"])
    return [bounded("loss", got["loss"], r["loss"], np.array([tol])), bounded("grad", got["grad"], r["grad"], r["_grad_bound"])]


def pearson_emulate(c, t, mean_for_sum=False):
    r = pearson_reference(dict(c, reduction="mean") if mean_for_sum else c, t)
    return {"loss": r["loss"].astype(np.float32), "grad": r["grad"].astype(np.float32)}


# ---- ElemLoss ----------------------------------------------------------------------------------
ELEM_G = 3.0
ELEM_SHAPE = (3, 7, 11)                              # 231 elements: numel % 4 != 0
ELEM_PARAM = {"l1": 0.0, "smooth_l1": 0.7, "huber": 1.3, "mse": 0.0}
ELEM_CASES = [{"name": f"{kind}-{red}", "kind": kind, "reduction": red} for kind in ELEM_PARAM for red in ("mean", "sum")]


def elem_inputs(c):
    g = _rng("elem" + c["name"])
    pred = (2 * g.standard_normal(ELEM_SHAPE)).astype(np.float32)
    true = g.standard_normal(ELEM_SHAPE).astype(np.float32)
    pred[0, 0, :3] = true[0, 0, :3]                  # equal elements: the sign of 0
    return {"pred": pred, "true": true}


def elem_reference(c, t):
    """l1 |d|;  smooth_l1 d^2 / (2 beta) below beta, |d| - beta / 2 above;  huber d^2 / 2 below delta, delta (|d| - delta / 2) above;
    mse d^2.  Gradients by the piece; times g, over n for the mean."""
    d = t["pred"].astype(np.float64) - t["true"].astype(np.float64)
    a, p, kind = np.abs(d), ELEM_PARAM[c["kind"]], c["kind"]
    if kind == "l1":
        v, dv = a, np.sign(d)
    elif kind == "mse":
        v, dv = d * d, 2 * d
    elif kind == "smooth_l1":
        v, dv = np.where(a < p, 0.5 * d * d / p, a - 0.5 * p), np.where(a < p, d / p, np.sign(d))
    else:
        v, dv = np.where(a <= p, 0.5 * d * d, p * (a - 0.5 * p)), np.where(a <= p, d, p * np.sign(d))
    k = 1.0 / d.size if c["reduction"] == "mean" else 1.0
    return {"loss": np.array([v.sum() * k]), "grad": ELEM_G * k * dv, "_abs": np.array([v.sum() * k])}


def elem_check(c, t, got):
    """loss   f32 terms in f32 chains, then f64: the project's standing 1e-5 relative (test_gpu_robust_loss.py)
       grad   rtol 1e-4, atol 0: an exact zero of the reference is an exact zero here (test_gpu_robust_loss.py)"""
    r = elem_reference(c, t)
    return [bounded("loss", got["loss"], r["loss"], 1e-5 * np.abs(r["loss"])), bounded("grad", got["grad"], r["grad"], 1e-4 * np.abs(r["grad"]))]


def elem_emulate(c, t, mean_for_sum=False):
    r = elem_reference(dict(c, reduction="mean") if mean_for_sum else c, t)
    return {"loss": r["loss"].astype(np.float32), "grad": r["grad"].astype(np.float32)}


# ================================================================================================
# faults: the reference's output perturbed the way a wrong launch would (tests/test_autograd_ref_host.py: each must fail a case)
# ================================================================================================
def _copy(got):
    return {k: np.array(v, copy=True) for k, v in got.items()}


def _linear_got(c):
    t = linear_inputs(c)
    return t, emulate_exact(linear_reference(c, t), linear_kinds(c))


def _fault_linear(mutate, needs=()):
    def run(c):
        if c["M"] > 1024 or any(not n(c) for n in needs):
            return None
        t, got = _linear_got(c)
        mutate(c, t, got)
        return check_exact(linear_reference(c, t), linear_kinds(c), got)
    return "linear", run


def _dw_last_row(c, t, got):
    got["dw"][-1] = got["dw"][-2]


def _db_short(c, t, got):
    got["db"] = (t["dy"].astype(np.float64)[:-1].sum(0)).astype(np.float32)


def _drs_from_dy(c, t, got):
    got["drs"] = t["dy"].astype(np.float64).sum(0).astype(np.float32)


def _dres_scaled(c, t, got):
    got["dres"] = (t["dy"] * t["rs"][None, :]).astype(np.float32)


def _fault_qkv(c):
    t = qkv_inputs(c)
    ref = qkv_reference(c, t)
    got = emulate_exact(ref, QKV_KINDS)
    got["dwq"], got["dwk"] = got["dwk"], got["dwq"]
    return check_exact(ref, QKV_KINDS, got)


def _fault_voxel_slab(c):
    s = c["subjects"]
    rep = [b for b in range(len(s)) if s.index(s[b]) != b]
    if not rep:
        return None
    t = voxel_inputs(c)
    ref = voxel_reference(c, t)
    got = emulate_exact(ref, {})
    dy = adaptive_avg_pool_adjoint(torch.from_numpy(t["g"].astype(np.float64)), c["T"]).numpy()
    b = rep[0]
    got["dw"][s[b]] += np.einsum("tc,vt->cv", t["x"][b, :, :c["Cc"]].astype(np.float64), dy[b]).astype(np.float32)
    return check_exact(ref, {}, got)


def _fault_voxel_pad(c):
    if c["Cp"] == c["Cc"]:
        return None
    t = voxel_inputs(c)
    ref = voxel_reference(c, t)
    got = emulate_exact(ref, {})
    got["dx"][:, :, c["Cc"]] = got["dx"][:, :, c["Cc"] - 1]
    return check_exact(ref, {}, got)


def _fault_ff(c):
    t = ff_inputs(c)
    return ff_check(c, t, ff_emulate(c, t, fault="gelu_grad_at_h"))


def _fault_tau(c):
    t = infonce_inputs(c)
    return infonce_check(c, t, infonce_emulate(c, t, tau_twice=True))


def _fault_mean_for_sum(c):
    if c["reduction"] != "sum" or c["V"] == 1:
        return None
    t = pearson_inputs(c)
    return pearson_check(c, t, pearson_emulate(c, t, mean_for_sum=True))


FAULTS = {
    "the last row of dw left from the previous tile": _fault_linear(_dw_last_row),
    "db summed over M - 1 rows": _fault_linear(_db_short, [lambda c: c["bias"]]),
    "drs computed from dy instead of dy * res": _fault_linear(_drs_from_dy, [lambda c: c["res"] == "scaled"]),
    "dres scaled when raw_res_grad is set": _fault_linear(_dres_scaled, [lambda c: c["raw"]]),
    "the q and k slices of dw swapped": ("qkv", _fault_qkv),
    "one repeated subject's slab added twice": ("voxel", _fault_voxel_slab),
    "a pad column of dx equal to its neighbour": ("voxel", _fault_voxel_pad),
    "gelu' taken at h instead of pre": ("ff", _fault_ff),
    "1/tau applied twice": ("infonce", _fault_tau),
    "mean taken for sum": ("pearson", _fault_mean_for_sum),
}

FAMILIES = {"linear": LINEAR_CASES, "qkv": QKV_CASES, "projector": PROJECTOR_CASES, "voxel": VOXEL_CASES, "packrows": PACKROWS_CASES,
            "ff": FF_CASES, "scalenorm": SCALENORM_CASES, "infonce": INFONCE_CASES, "pearson": PEARSON_CASES, "elem": ELEM_CASES}
