"""Float64 reference, input generators and launch-plan replays for the bf16 GEMM (csrc/gemm.hip, csrc/gemm_common.h).  CPU only: numpy
(torch's CPU generator for the randn operands), no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  tests/test_gemm_ref_host.py pins what is here -- the activations to torch's float64
ones, the exactness argument to three f32 summation orders, the plan replays to the case table below (and, where the library loads, to
its own planner); tests/test_gpu_gemm_bounds.py holds the kernels to it.

The epilogue is the one of oracle.fp8_ref (the two GEMMs share csrc/gemm_common.h); added here are row_scale, EXP2, MUL_AUX, GELU_BWD,
the bf16 pre-activation the GELU forward keeps in `aux`, transposed operands, batches and gather1.

EXACT inputs: operands are integers in [-3, 3] (bf16 holds them), alpha / row_scale / res_scale powers of two in {1/2, 1, 2}, bias,
residual, rowadd and gadd multiples of 1/64 in [-2, 2].  A product is an integer of magnitude <= 9, so every partial sum over K is an
integer below 9 K: exact in f32, in ANY order and under any split of K, while 9 K < 2^24.  With the addends the result is a multiple of
2^-7 (a 1/64 residual times res_scale 1/2) of magnitude below 9 K |alpha| + 8: 24 bits hold it while 9 K |alpha| 2 < 2^18.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle import fp8_ref
from oracle.fp8_ref import activation64, gelu64, preact64, sigmoid64, silu64  # noqa: F401  (re-exported: one epilogue, two GEMMs)

BK = 64                      # K-tile of every bf16 kernel
PAIR_ACTS = ("swiglu", "glu")


# ------------------------------------------------------------------------------------------------
# the epilogue in float64
# ------------------------------------------------------------------------------------------------
def gelu_grad64(v):
    """d/dv [v Phi(v)] = Phi(v) + v phi(v); Phi through erfc on the negative side (no cancellation)."""
    v = np.asarray(v, dtype=np.float64)
    cdf = 0.5 * fp8_ref._erfc(-v / math.sqrt(2.0))
    return cdf + v * np.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def bf16_value(bits) -> np.ndarray:
    """uint16 bf16 patterns -> float64 values."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def act64(v, act=None, aux=None) -> np.ndarray:
    """The activation on a float64 pre-activation v [M, N].  None / 'gelu' / 'silu' / 'swiglu' / 'glu' as oracle.fp8_ref.activation64;
    'exp2': 2^v;  'mul_aux': v * aux;  'gelu_bwd': v * gelu'(aux)  (aux float64 [M, N]: the VALUES of the bf16 operand)."""
    if act == "exp2":
        return np.exp2(np.asarray(v, dtype=np.float64))
    if act == "mul_aux":
        return np.asarray(v, dtype=np.float64) * np.asarray(aux, dtype=np.float64)
    if act == "gelu_bwd":
        return np.asarray(v, dtype=np.float64) * gelu_grad64(aux)
    return activation64(v, act)


def epilogue64(acc, *, alpha=1.0, row_scale=None, row_bias=None, col_bias=None, act=None, aux=None, res=None, res_scale=None, rowadd=None,
               rowadd_period=None, gadd=None, gadd_index=None, gadd_div=None, want_preact=False):
    """One matrix: y = act(alpha * acc * row_scale[m] + bias) + res * res_scale[n] + rowadd[m % period] + gadd[gadd_index[m // div]].
    want_preact: also return the pre-activation (what a GELU forward with `aux` stores there, rounded to bf16)."""
    acc = np.asarray(acc, dtype=np.float64)
    if row_scale is not None:
        acc = acc * np.asarray(row_scale, dtype=np.float64)[:, None]
    v = preact64(acc, alpha=alpha, row_bias=row_bias, col_bias=col_bias)
    y = fp8_ref.epilogue64(act64(v, act, aux), res=res, res_scale=res_scale, rowadd=rowadd, rowadd_period=rowadd_period, gadd=gadd,
                           gadd_index=gadd_index, gadd_div=gadd_div)
    return (y, v) if want_preact else y


def product64(a, b, trans_ab=False) -> np.ndarray:
    """A B^T of A [M, K], B [N, K]; trans_ab: At^T Bt of At [K, M], Bt [K, N]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.T @ b if trans_ab else a @ b.T


def reference64(a, b, *, trans_ab=False, gather1=None, gather_a=False, gather_b=False, gather_bias=False, **epi) -> np.ndarray:
    """The whole descriptor.  Un-batched: a, b 2-D, `epi` as epilogue64 takes it.  Batched: a, b [batch1, batch0, ., .]; every entry of
    `epi` that is batched in the launch (row_bias, col_bias, res, aux) carries the same two leading axes, the rest is shared.  gather1
    replaces the batch1 index of A (gather_a), B (gather_b) and the bias (gather_bias); C, the residual and aux follow the plain index."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 2:
        return epilogue64(product64(a, b, trans_ab), **epi)
    batched = {k: np.asarray(v) for k, v in epi.items() if k in ("row_bias", "col_bias", "res", "aux") and v is not None}
    shared = {k: v for k, v in epi.items() if k not in batched}
    out = []
    for b1 in range(a.shape[0]):
        g = b1 if gather1 is None else int(gather1[b1])
        row = []
        for b0 in range(a.shape[1]):
            kw = {k: v[g if (k.endswith("bias") and gather_bias) else b1, b0] for k, v in batched.items()}
            row.append(epilogue64(product64(a[g if gather_a else b1, b0], b[g if gather_b else b1, b0], trans_ab), **shared, **kw))
        out.append(np.stack(row))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------
# EXACT inputs
# ------------------------------------------------------------------------------------------------
A_MAX = 3


def exact_operands(shape_a, shape_b, seed, bmax=A_MAX):
    """Integer operands: A in [-3, 3], B in [-bmax, bmax] (bmax = 1 for the activation cases: pre-activations stay near 0, where the
    activations bend), as float32 arrays that bf16 holds exactly."""
    g = np.random.default_rng(seed)
    a = g.integers(-A_MAX, A_MAX + 1, shape_a).astype(np.float32)
    b = g.integers(-bmax, bmax + 1, shape_b).astype(np.float32)
    return a, b


def sixty_fourths(g: np.random.Generator, *shape, lo=-2.0, hi=2.0) -> np.ndarray:
    """Multiples of 1/64 in [lo, hi] as f32 (bias, residual, rowadd, gadd; EXP2 row biases with lo = -24, hi = 0)."""
    return (g.integers(int(lo * 64), int(hi * 64) + 1, shape) / 64.0).astype(np.float32)


def power_of_two(g: np.random.Generator, *shape) -> np.ndarray:
    """Powers of two in {1/2, 1, 2} (row_scale, res_scale)."""
    return np.ldexp(1.0, g.integers(-1, 2, shape)).astype(np.float32)


def is_exact(K, alpha=1.0, addends=False, scale=1.0, bmax=A_MAX) -> bool:
    """Whether a case of EXACT inputs is exact in f32 whatever the order of its additions.  `scale`: the largest row_scale.  Without
    addends the result is alpha * scale * (an integer below A_MAX bmax K): 24 bits hold the integer while A_MAX bmax K < 2^24.  With
    addends (multiples of 1/64, a res_scale down to 1/2) the result is a multiple of 2^-7 below A_MAX bmax K |alpha| scale + 8."""
    if not (_is_pow2(alpha) and _is_pow2(scale)):
        return False
    top = A_MAX * bmax * K
    return top * abs(alpha) * scale * 2 < 2**18 if addends else top < 2**24


def _is_pow2(x) -> bool:
    m, _ = math.frexp(abs(float(x)))
    return m == 0.5


def f32_sums(products: np.ndarray):
    """The f32 sum of a vector of products forward, reversed and pairwise."""
    p = np.asarray(products, dtype=np.float32)
    return fp8_ref.f32_sum_forward(p), fp8_ref.f32_sum_forward(p[::-1]), fp8_ref.f32_sum_pairwise(p)


# ------------------------------------------------------------------------------------------------
# RANDOM inputs
# ------------------------------------------------------------------------------------------------
def random_inputs(M, N, K, trans_ab=False):
    """randn operands rounded to bf16 (f32 arrays of bf16-exact values; trans_ab: At [K, M], Bt [K, N]), a column bias, a residual,
    the float64 product and S = |A| |B|^T for the accumulation bound K u S."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    bf = lambda x: x.to(torch.bfloat16).to(torch.float32).numpy()      # noqa: E731
    a, b = bf(torch.randn((K, M) if trans_ab else (M, K), generator=g)), bf(torch.randn((K, N) if trans_ab else (N, K), generator=g))
    t = {"a": a, "b": b, "bias": torch.randn(N, generator=g).numpy(), "res": torch.randn(M, N, generator=g).numpy()}
    t["base"] = product64(a, b, trans_ab)
    t["S"] = product64(np.abs(a), np.abs(b), trans_ab)
    return t


# ------------------------------------------------------------------------------------------------
# launch plans, replayed (csrc/gemm.hip: plan_stream_k, gemm_plan)
# ------------------------------------------------------------------------------------------------
def tiles256(M, N) -> int:
    return -(-M // 256) * -(-N // 256)


def plan_stream_k(tiles, nk, W=256):
    """plan_stream_k of the launcher: the tiles of the last partial round (at most half a round, runs of at least 8 K-steps) are cut
    into W runs of q K-steps.  None when the launch stays whole.  Otherwise tiles_dp / rem_units / q / workers / second_worker (the
    workers whose run crosses a tile boundary, longest second part first) / grid as the library reports them, and what the case table
    claims: second = number of second parts, idle = workers without work, parts = (fewest, most) parts a split tile is summed from."""
    rem = tiles % W
    if rem == 0 or rem * 2 > W or rem * nk < W * 8:
        return None
    units = rem * nk
    q = -(-units // W)
    seconds, idle = [], 0
    for w in range(W):
        u0 = w * q
        if u0 >= units:
            idle += 1
            continue
        run = min(q, units - u0)
        first = min(run, nk - u0 % nk)
        if first < run:
            seconds.append((run - first, w))
    order = [w for _, w in sorted(seconds, key=lambda t: -t[0])]          # stable: equal lengths keep worker order
    parts = [(t * nk + nk - 1) // q - (t * nk) // q + 1 for t in range(rem)]
    return {"tiles_dp": tiles - rem, "rem_units": units, "q": q, "workers": W, "second_worker": order, "grid": tiles - rem + W + len(order),
            "second": len(order), "idle": idle, "parts": (min(parts), max(parts))}


def split_k_shares(M, N, K, batches=1):
    """gemm_plan's split-K rule for a ring-kernel launch of 128 x 128 tiles: sp = min(256 / t128, nk / 8, 8) shares (none below 2), share s
    covering K-steps [s nk / sp, (s + 1) nk / sp).  Returns the share lengths ([nk] when the launch stays whole)."""
    t128 = -(-M // 128) * -(-N // 128) * batches
    nk = K // BK
    sp = min(256 // t128, nk // 8, 8)
    if sp < 2:
        return [nk]
    return [(s + 1) * nk // sp - s * nk // sp for s in range(sp)]


# ------------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_gemm_bounds.py (checked on the host by tests/test_gemm_ref_host.py)
# ------------------------------------------------------------------------------------------------
# stream-K (trans_ab, f32, alpha = 1/2): (M, N, K) -> what the plan must look like; None = left whole
STREAM_K_CASES = {
    (8, 16, 131072): {"tiles": 1, "tiles_dp": 0, "q": 8, "second": 0, "idle": 0, "parts": (256, 256)},
    (264, 520, 22016): {"tiles": 6, "tiles_dp": 0, "q": 9, "second": 5, "idle": 26, "parts": (39, 40)},
    (1024, 1280, 8192): {"tiles": 20, "tiles_dp": 0, "q": 10, "second": 16, "idle": 0, "parts": (13, 14)},
    (4096, 6144, 1088): {"tiles": 384, "tiles_dp": 256, "q": 9, "second": 113, "idle": 14, "parts": (2, 3)},
    (512, 512, 128): None,            # too few K-steps to share out
    (3072, 3072, 256): None,          # 144 tiles: a remainder above half a round
}
STREAM_K_ALPHA = 0.5

# split-K (NT, ring kernel): (M, N, K) -> share lengths in K-steps
SPLIT_K_CASES = {
    (128, 128, 1024): [8, 8],
    (128, 128, 4096): [8] * 8,
    (128, 128, 1216): [9, 10],
    (128, 128, 1600): [8, 8, 9],
    (77, 200, 4096): [8] * 8,
    (128, 1024, 4096): [8] * 8,
}

# every EXACT case family of the GPU test: (name, largest K, largest |alpha|, addends, largest row_scale, bmax)
EXACT_FAMILIES = [
    ("tn K loop / rotation / edges", 512, 1.0, False, 1.0, 3),
    ("tn operators", 128, 1.0, True, 1.0, 3),
    ("tn scalar branch", 128, 0.5, True, 1.0, 3),
    ("tn batched", 192, 1.0, True, 1.0, 3),
    ("stream-K 8x16", 131072, 0.5, False, 1.0, 3),
    ("stream-K 264x520", 22016, 0.5, False, 1.0, 3),
    ("stream-K 1024x1280", 8192, 0.5, False, 1.0, 3),
    ("stream-K 4096x6144", 1088, 0.5, False, 1.0, 3),
    ("stream-K left whole", 256, 0.5, False, 1.0, 3),
    ("split-K share counts", 4096, 1.0, False, 1.0, 3),
    ("split-K operators", 4096, 2.0, True, 2.0, 1),
    ("ext activations", 256, 1.0, True, 1.0, 1),
    ("nt batches and gather", 128, 1.0, True, 1.0, 3),
    ("nt K loop", 512, 1.0, False, 1.0, 3),
]
ACT_MAX_K = 256     # activation cases: B in [-1, 1] and K <= 256
