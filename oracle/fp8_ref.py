"""Float64 / integer references for the fp8 path (csrc/gemm_fp8.hip): the OCP e4m3 format, the quantiser's rounding and the GEMM
epilogue's operators.  CPU only: numpy, no torch, no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Everything here is written from the format definition and from the kernels'
documented behaviour, not from torch's float8 type: tests/test_fp8_host.py pins the table and the encoder to torch.float8_e4m3fn,
so that a wrong reference cannot bless a wrong kernel; tests/test_gpu_fp8_bounds.py holds the kernels to them.

e4m3 ("fn": finite, no infinities): 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits.
    exponent field 0:      subnormal, value m / 8 * 2^-6           (smallest 2^-9)
    exponent field 1..15:  (1 + m / 8) * 2^(e - 7)                 (largest: e = 15, m = 6 -> 448)
    0x7F / 0xFF (e = 15, m = 7): NaN.  254 finite codes, two of them zeros.
"""

from __future__ import annotations

import math

import numpy as np

E4M3_MAX = 448.0
E4M3_MIN_SUBNORMAL = 2.0**-9
E4M3_MIN_NORMAL = 2.0**-6
E4M3_NAN = 0x7F            # | 0x80 for a NaN with the sign bit set


def _decode(code: int) -> float:
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 0xF, code & 0x7
    if e == 0xF and m == 0x7:
        return math.nan
    if e == 0:
        return sign * (m / 8.0) * 2.0**-6
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


E4M3_VALUES = np.array([_decode(c) for c in range(256)], dtype=np.float64)      # code -> value
FINITE_CODES = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)


def decode_e4m3(codes) -> np.ndarray:
    """uint8 codes -> float64 values (NaN for 0x7F / 0xFF)."""
    return E4M3_VALUES[np.asarray(codes, dtype=np.uint8)]


def scale_f32(x, inv_scale=1.0) -> np.ndarray:
    """The quantiser's scaling step: f32(x) * f32(inv_scale), ONE f32 product (inv_scale is np.float32(1 / scale), the value
    ops.quantize_fp8 hands to the kernel)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(x, dtype=np.float32) * np.float32(inv_scale)).astype(np.float32)


def encode_e4m3(x_f32, inv_scale=1.0) -> np.ndarray:
    """f32 values -> uint8 e4m3 codes as the quantiser kernels define them:
        y = f32(x) * f32(inv_scale)                   one f32 rounding
        NaN            -> 0x7F, with the sign bit of the NaN: 0xFF
        |y| > 448      -> +-448 (0x7E / 0xFE): SATURATING, +-inf included
        otherwise      round to nearest representable, ties to the even mantissa; below half the smallest subnormal (and the
                       tie at exactly 2^-10, whose even neighbour is 0) -> zero.  The sign of y is kept, on zeros too."""
    y = scale_f32(x_f32, inv_scale)
    sign = (np.signbit(y)).astype(np.uint8) << 7
    nan = np.isnan(y)
    a = np.abs(np.where(nan, np.float32(0), y)).astype(np.float64)
    a = np.minimum(a, E4M3_MAX)
    # the spacing of e4m3 at |y|: 2^-9 below the smallest normal, else 2^(floor(log2 a) - 3)
    _, ex = np.frexp(np.maximum(a, E4M3_MIN_NORMAL))        # a = f * 2^ex, f in [0.5, 1): floor(log2 a) = ex - 1
    e = ex.astype(np.int64) - 1
    quantum = np.ldexp(1.0, e - 3)
    q = np.rint(a / quantum).astype(np.int64)               # exact quotient (a power-of-two divisor); rint = ties to even
    sub = a < E4M3_MIN_NORMAL
    # subnormal range: q = 0..8 and the code IS q (q = 8 is 0x08, the smallest normal).  Normal: q = 8 + m, or 16 = the next binade
    carry = q == 16
    field = np.where(carry, e + 8, e + 7)
    mant = np.where(carry, 0, q - 8)
    code = np.where(sub, q, (field << 3) | mant).astype(np.uint8)
    return np.where(nan, np.uint8(E4M3_NAN), code).astype(np.uint8) | sign


def midpoints():
    """(lo codes, hi codes, f32 midpoints) of every pair of neighbouring non-negative finite codes 0x00..0x7E: 126 pairs.  A midpoint
    needs one mantissa bit more than e4m3 has, so it is exact in f32 (and in bf16)."""
    lo = np.arange(0x00, 0x7E, dtype=np.uint8)
    hi = lo + 1
    mid = (E4M3_VALUES[lo] + E4M3_VALUES[hi]) / 2
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    return lo, hi, mid.astype(np.float32)


def interesting_f32() -> dict[str, np.ndarray]:
    """The sets of f32 inputs the quantiser tests walk (tests/test_fp8_host.py pins encode_e4m3 on them, tests/test_gpu_fp8_bounds.py
    the kernel): name -> f32 array.  `ties` and `around` come in both signs."""
    _, _, mid = midpoints()
    below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    pm = lambda v: np.concatenate([v, -v]).astype(np.float32)       # noqa: E731
    tiny = np.float32(2.0**-10)                                     # half the smallest subnormal: the flush-to-zero threshold (a tie, to even = 0)
    sub = np.concatenate([np.arange(0, 9, dtype=np.float32) * np.float32(2.0**-9),                    # 0, the 7 subnormals, the smallest normal
                          np.array([tiny, np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1)), 2.0**-11, 1e-9, 1e-30, 1e-45,
                                    3 * 2.0**-10, 2.0**-6 - 2.0**-10], dtype=np.float32)])
    return {
        "codes": E4M3_VALUES[FINITE_CODES].astype(np.float32),      # every finite code's value (254, -0 among them)
        "ties": pm(mid),
        "around": pm(np.concatenate([below, above])),
        "subnormal": pm(sub),
        "zeros": np.array([0.0, -0.0], dtype=np.float32),
        # 464 is the midpoint between 448 and the 480 that the format gives up for its NaN code: the last value torch's cast keeps finite
        "saturation": pm(np.array([448.0, np.nextafter(np.float32(448), np.float32(np.inf)), 463.99, 464.0,
                                   np.nextafter(np.float32(464), np.float32(np.inf)), 465.0, 480.0, 512.0, 1e4, 1e30, 3.4028234663852886e38, np.inf],
                                  dtype=np.float32)),
    }


def bf16_exact(x: np.ndarray) -> np.ndarray:
    """The subset of f32 values that bf16 holds exactly (low 16 bits zero)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x[(x.view(np.uint32) & 0xFFFF) == 0]


# ------------------------------------------------------------------------------------------------
# the GEMM epilogue in float64, in the kernel's order (csrc/gemm_common.h, epilogue_row4):
#   v = alpha * acc;  + row bias[m] | + column bias[n];  activation;  + res * res_scale[n];  + rowadd[m % period];  + gadd[gadd_index[m // div]]
# ------------------------------------------------------------------------------------------------
def sigmoid64(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(v >= 0, 1.0 / (1.0 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1.0 + np.exp(-np.abs(v))))


def silu64(v):
    return np.asarray(v, dtype=np.float64) * sigmoid64(v)


_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def gelu64(v):
    """GELU with erf: v * Phi(v), Phi(v) = (1 + erf(v / sqrt 2)) / 2.  For v < 0 the sum 1 + erf cancels, so it is taken as
    erfc(-v / sqrt 2), the same function without the cancellation."""
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * _erfc(-v / math.sqrt(2.0))


def preact64(acc, *, alpha=1.0, row_bias=None, col_bias=None) -> np.ndarray:
    """alpha * acc + bias: the value the activation sees.  acc float64 [M, N]; alpha is the f32 the descriptor carries."""
    v = np.asarray(acc, dtype=np.float64) * float(np.float32(alpha))
    if row_bias is not None:
        v = v + np.asarray(row_bias, dtype=np.float64)[:, None]
    if col_bias is not None:
        v = v + np.asarray(col_bias, dtype=np.float64)[None, :]
    return v


def activation64(v, act=None) -> np.ndarray:
    """act: None, 'gelu', 'silu' -> [M, N];  'swiglu' / 'glu' pair the columns (even = gate, odd = up) -> [M, N / 2]:
    SwiGLU silu(gate) * up, GLU gate * sigmoid(up)."""
    if act is None:
        return np.asarray(v, dtype=np.float64)
    if act == "gelu":
        return gelu64(v)
    if act == "silu":
        return silu64(v)
    gate, up = v[:, 0::2], v[:, 1::2]
    if act == "swiglu":
        return silu64(gate) * up
    if act == "glu":
        return gate * sigmoid64(up)
    raise ValueError(f"activation64: {act}")


def epilogue64(acc, *, alpha=1.0, row_bias=None, col_bias=None, act=None, res=None, res_scale=None, rowadd=None, rowadd_period=None,
               gadd=None, gadd_index=None, gadd_div=None) -> np.ndarray:
    """The whole epilogue of one matrix.  res [M, N]; res_scale [N]; rowadd [period, N] added to row m as rowadd[m % period];
    gadd [G, N] added to row m as gadd[gadd_index[m // gadd_div]] (runs of gadd_div consecutive rows share an index entry, and
    entries may repeat)."""
    y = activation64(preact64(acc, alpha=alpha, row_bias=row_bias, col_bias=col_bias), act)
    M = y.shape[0]
    rows = np.arange(M)
    if res is not None:
        r = np.asarray(res, dtype=np.float64)
        y = y + (r * np.asarray(res_scale, dtype=np.float64)[None, :] if res_scale is not None else r)
    if rowadd is not None:
        y = y + np.asarray(rowadd, dtype=np.float64)[rows % int(rowadd_period)]
    if gadd is not None:
        y = y + np.asarray(gadd, dtype=np.float64)[np.asarray(gadd_index, dtype=np.int64)[rows // int(gadd_div)]]
    return y


# ------------------------------------------------------------------------------------------------
# the exactness argument of the GPU tests: operands j / 8, |j| <= 15
# ------------------------------------------------------------------------------------------------
def eighths_codes(j) -> np.ndarray:
    """e4m3 codes of j / 8 for integer j in [-15, 15] (every such value needs at most 4 significant bits: e4m3 holds it exactly;
    0 is +0)."""
    j = np.asarray(j, dtype=np.int64)
    assert np.abs(j).max() <= 15
    codes = encode_e4m3((j / 8.0).astype(np.float32))
    assert np.array_equal(E4M3_VALUES[codes] * 8, j.astype(np.float64))
    return codes


def f32_sum_forward(p: np.ndarray) -> np.float32:
    s = np.float32(0)
    for v in p:
        s = np.float32(s + v)
    return s


def f32_sum_pairwise(p: np.ndarray) -> np.float32:
    p = np.asarray(p, dtype=np.float32)
    while p.size > 1:
        if p.size & 1:
            p = np.concatenate([p, np.zeros(1, dtype=np.float32)])
        p = (p[0::2] + p[1::2]).astype(np.float32)
    return p[0]
