"""Float64 reference, input generators and launch-plan replays for the bf16 GEMM (csrc/gemm.hip, csrc/gemm_common.h).  CPU only: numpy
(torch's CPU generator for the randn operands), no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  tests/test_gemm_ref_host.py pins what is here -- the activations to torch's float64
ones, the exactness argument to three f32 summation orders, the plan replays to the case table below (and, where the library loads, to
its own planner); tests/test_gpu_gemm_bounds.py holds the kernels to it.  The last section is the case table, the path replay and the
fault references of tests/test_gpu_gemm_forward_bounds.py (the forward operators of the generic epilogue on the four NT tile kernels).

The epilogue is the one of oracle.fp8_ref (the two GEMMs share csrc/gemm_common.h); added here are row_scale, EXP2, MUL_AUX, GELU_BWD,
the bf16 pre-activation the GELU forward keeps in `aux`, transposed operands, batches and gather1.

EXACT inputs: operands are integers in [-3, 3] (bf16 holds them), alpha / row_scale / res_scale powers of two in {1/2, 1, 2}, bias,
residual, rowadd and gadd multiples of 1/64 in [-2, 2].  A product is an integer of magnitude <= 9, so every partial sum over K is an
integer below 9 K: exact in f32, in ANY order and under any split of K, while 9 K < 2^24.  With the addends the result is a multiple of
2^-7 (a 1/64 residual times res_scale 1/2) of magnitude below 9 K |alpha| + 8: 24 bits hold it while 9 K |alpha| 2 < 2^18.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import fp8_ref
from oracle.layout_ref import bf16_bits
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
    # tests/test_gpu_gemm_forward_bounds.py (the case table FWD_CASES below; its fused-norm family is held by is_exact_sumsq)
    ("forward operators", 256, 0.5, True, 2.0, 3),
    ("forward row_scale", 128, 1.0, False, 2.0, 3),
    ("forward fused-norm producer", 128, 1.0, True, 1.0, 1),
]
ACT_MAX_K = 256     # activation cases: B in [-1, 1] and K <= 256


# ------------------------------------------------------------------------------------------------
# the forward operators on the four NT tile kernels: tests/test_gpu_gemm_forward_bounds.py
# ------------------------------------------------------------------------------------------------
# kernel -> (kind as tribe_debug_gemm_plan reports it, BM, BN, columns per row_sumsq slot, the tile_hint that forces it)
FWD_KERNELS = {"db128": (0, 128, 128, 64, 1), "ring128": (2, 128, 128, 64, 3), "w8_256": (1, 256, 256, 64, 2), "w8_192": (1, 256, 192, 48, 4)}
FWD_PATHS = ("P1", "P2a", "P2b", "P2c", "P3a", "P3b", "P3c")
FWD_M, FWD_K = 300, 128                    # every forced-hint case but the ragged-M ones; ragged for 128- and 256-row tiles alike
FWD_SUMSQ_SHAPE = (300, 768, 128)          # 768 is a multiple of 128, 192 and 256

# the operator sets the callers build.  dtypes: the outputs a set runs with;  p1_only: the launcher admits row_scale / c_bf16 /
# row_sumsq on tiles inside N with 16-byte operands only;  bmax = 1 where a GELU must see pre-activations near 0
FWD_OPS = {
    "none": {},
    "col_bias": {"col_bias": True},
    "voxel_head": {"alpha": 0.5, "row_bias": True},
    "res": {"res": True},
    "out_proj": {"col_bias": True, "res": True, "res_scale": True, "inplace": True},       # bf16: the residual in a buffer of its own
    "bias_rowadd7": {"col_bias": True, "rowadd": 7},
    "bias_rowadd32": {"col_bias": True, "rowadd": 32},
    "rowadd_res": {"rowadd": 7, "res": True},
    "projector": {"alpha": 0.5, "row_bias": True, "rowadd": 7, "gadd": True},
    "row_scale": {"row_scale": True, "dtypes": ("bf16",), "p1_only": True},
    "row_scale_bias_gelu": {"row_scale": True, "col_bias": True, "gelu": True, "bmax": 1, "dtypes": ("bf16",), "p1_only": True},
    "bias_gelu": {"col_bias": True, "gelu": True, "bmax": 1},
    "fused_norm": {"col_bias": True, "res": True, "res_scale": True, "inplace": True, "fused": True, "bmax": 1, "dtypes": ("f32",),
                   "p1_only": True},
}
FWD_GADD_DIV, FWD_GADD_ROWS = 32, 5
FWD_GADD_INDEX = (3, 0, 3, 4, 1, 1, 2, 0, 4, 3)        # repeats, not sorted


def fwd_dtypes(ops):
    return FWD_OPS[ops].get("dtypes", ("f32", "bf16"))


def fwd_exact(ops) -> bool:
    """Whether the set is compared bit for bit (everything but the GELU sets, which are bounded)."""
    return not FWD_OPS[ops].get("gelu", False)


def is_exact_sumsq(K, bmax, cols) -> bool:
    """The fused-norm producer family: bias and residual integers in [-2, 2], res_scale in {1, 2}, alpha = 1.  A stored value is an
    integer of magnitude at most A_MAX bmax K + 2 + 2 * 2, so a slot's sum of `cols` squares is an integer below 2^24: exact in f32
    in any order."""
    top = A_MAX * bmax * K + 6
    return top * top * cols < 2**24


class FwdCase(tuple):
    """(hint, M, N, K, ops, variant, out, kernel).  variant: 'pad' ldc = N rounded up to 4, + 4;  'ldc2' ldc = N + 2;  'c1' C offset by
    one element;  'bias1' the column bias offset by one float;  'sspad' ld_row_sumsq = slots + 3 (else the slots are packed)."""
    __slots__ = ()
    hint, M, N, K, ops, variant, out, kernel = (property(lambda s, i=i: s[i]) for i in range(8))

    def __new__(cls, *a):
        assert len(a) == 8
        return tuple.__new__(cls, a)

    @property
    def id(self):
        return f"hint{self.hint}-{self.kernel}-{self.M}x{self.N}x{self.K}-{self.ops}-{self.variant}-{self.out}"


def _fwd_cases():
    rows = []
    for kernel, (_, _, bn, _, hint) in FWD_KERNELS.items():
        inside, cross, last_quad = 2 * bn, bn + 8, bn + 6          # P1;  P2a: a full tile beside an 8-column one;  P3c: N % 4 == 2
        add = lambda M, N, ops, variant, out: rows.append(FwdCase(hint, M, N, FWD_K, ops, variant, out, kernel))      # noqa: E731
        for ops, spec in FWD_OPS.items():
            for out in fwd_dtypes(ops):
                if spec.get("fused"):
                    add(*FWD_SUMSQ_SHAPE[:2], ops, "pad", out)
                    add(*FWD_SUMSQ_SHAPE[:2], ops, "sspad", out)
                    continue
                if not (spec.get("gadd") or (spec.get("rowadd") and spec.get("res"))):
                    add(FWD_M, inside, ops, "pad", out)             # P1
                if spec.get("p1_only"):
                    continue
                add(FWD_M, cross, ops, "pad", out)                  # P2a (or P2b / P2c: sets the fast path does not take)
                add(FWD_M, cross, ops, "ldc2", out)                 # P3a
        for out in ("f32", "bf16"):
            add(FWD_M, cross, "res", "c1", out)                     # P3b: C offset by one element
            add(FWD_M, cross, "col_bias", "bias1", out)             # P3b: the bias offset by one float (beside the aligned 'pad' case)
            add(FWD_M, last_quad, "res", "pad", out)                # P3c
            add(70, inside, "none", "pad", out)                     # one tile row that ends inside a sub-tile and inside a quad
        add(70, inside, "out_proj", "pad", "f32")
        add(200, inside, "out_proj", "pad", "f32")                 # 200: two 128-row tiles / one 256-row tile, ends on a quad
    # tile_hint 6: the generic epilogue on the tiles the role kernels use (256 wide, 192 where only that divides N)
    for ops, spec in FWD_OPS.items():
        for out in fwd_dtypes(ops):
            if spec.get("fused"):
                rows.append(FwdCase(6, *FWD_SUMSQ_SHAPE, ops, "pad", out, "w8_256"))
            elif spec.get("gadd") or (spec.get("rowadd") and spec.get("res")):
                rows.append(FwdCase(6, FWD_M, 264, FWD_K, ops, "pad", out, "w8_256"))
            else:
                rows.append(FwdCase(6, FWD_M, 512, FWD_K, ops, "pad", out, "w8_256"))
    rows.append(FwdCase(6, FWD_M, 384, FWD_K, "out_proj", "pad", "f32", "w8_192"))
    rows.append(FwdCase(6, FWD_M, 384, FWD_K, "col_bias", "pad", "bf16", "w8_192"))
    # tile_hint 0, one per kind the planner can choose for an NT launch (csrc/gemm_plan.cpp, plan_tiles):
    #   `use_big = M >= 256 && N >= 256 && t256 >= 96` false and `ring = ... t128 <= 256 && K >= 256` false: double-buffered 128^2
    rows.append(FwdCase(0, 70, 136, 128, "out_proj", "pad", "f32", "db128"))
    #   the same with K >= 256: the ring kernel
    rows.append(FwdCase(0, 70, 136, 256, "out_proj", "pad", "f32", "ring128"))
    #   8-wave, 192 wide: use_big needs t256 >= 96, and `t256 < 512 && t128 >= 512 && K <= 2048 && N <= 2048` must stay false, so
    #   t128 < 512; `N % 192 == 0 && t256 <= 2048` with ceil(t192 / 256) * 0.78 < 0.95 * ceil(t256 / 256).  N = 384 (two 256-wide tile
    #   columns, the fewest) needs 48 tile rows: M = 47 * 256 + 44, t256 = 96, t128 = 95 * 3 = 285, t192 = 96: 0.78 < 0.95
    rows.append(FwdCase(0, 47 * 256 + 44, 384, 64, "out_proj", "pad", "f32", "w8_192"))
    return tuple(rows)


FWD_CASES = _fwd_cases()
FWD_RANDOM_HINTS = (1, 3, 2, 4)            # RANDOM inputs: bias + scaled residual + row_sumsq at FWD_SUMSQ_SHAPE, one per kernel


def _up4(n):
    return (n + 3) // 4 * 4


def fwd_layout(case: FwdCase) -> dict:
    """Every pitch and offset of a case's launch (elements).  The operands of the addends have pitches of their own, all above N and
    multiples of 4, so that only the variant decides whether the epilogue may use 16-byte accesses."""
    spec, N = FWD_OPS[case.ops], case.N
    pad = _up4(N) + 4
    lay = {"lda": case.K + 8, "ldb": case.K + 8, "ldc": N + 2 if case.variant == "ldc2" else pad, "lead": int(case.variant == "c1"),
           "bias_lead": int(case.variant == "bias1"), "ldres": pad + 4, "ld_rowadd": pad + 8, "ld_gadd": pad, "ld_c_bf16": pad + 4,
           "inplace": bool(spec.get("inplace")) and case.out == "f32"}
    if lay["inplace"]:
        lay["ldres"] = lay["ldc"]
    if spec.get("fused"):
        slots = N // FWD_KERNELS[case.kernel][3]
        lay["slots"], lay["ld_row_sumsq"] = slots, slots + 3 if case.variant == "sspad" else slots
    return lay


def fwd_paths(case: FwdCase) -> frozenset:
    """The epilogue paths the tiles of a case take, restated from the kernels (every buffer of the test starts 16-byte aligned):
      EpiCtx::vec (make_epi_ctx)   ldc % 4 == 0, C aligned to four elements, and 16-byte bias / residual / res_scale / rowadd / gadd with
                                   pitches that are multiples of 4
      epilogue_fast_ok             vec, no rowadd beside a residual, no gadd  (its activation clause holds for every set here)
      per tile                     epilogue_fast_ok && n0 + BN <= N: P1 (epilogue_fast), else epilogue_tile16 -> epilogue_row4
      per quad in epilogue_row4    vec && n + 4 <= N: the vector branch (P2), else the scalar one (P3)
    P2a: a tile that crosses N;  P2b: a gadd;  P2c: rowadd beside a residual.  P3a: ldc % 4 != 0;  P3b: a pointer that is not 16-byte
    aligned (C offset by one element, the bias offset by one float);  P3c: the last quad of a row whose N % 4 != 0."""
    spec, lay, N = FWD_OPS[case.ops], fwd_layout(case), case.N
    bn = FWD_KERNELS[case.kernel][2]
    has_res, has_rowadd, has_gadd = bool(spec.get("res")), bool(spec.get("rowadd")), bool(spec.get("gadd"))
    pitches = lay["ldc"] % 4 == 0 and (not has_res or lay["ldres"] % 4 == 0) and (not has_rowadd or lay["ld_rowadd"] % 4 == 0) and \
        (not has_gadd or lay["ld_gadd"] % 4 == 0)
    # C is aligned to 4 elements of its type; an in-place residual is C read as f32
    pointers = lay["lead"] % 4 == 0 and (not spec.get("col_bias") or lay["bias_lead"] % 4 == 0)
    if not pitches:
        return frozenset({"P3a"})
    if not pointers:
        return frozenset({"P3b"})
    fast_ok = not (has_rowadd and has_res) and not has_gadd
    paths = set()
    for n0 in range(0, N, bn):
        if fast_ok and n0 + bn <= N:
            paths.add("P1")
            continue
        for n in range(n0, min(n0 + bn, N), 4):
            paths.add(("P2b" if has_gadd else "P2c" if (has_rowadd and has_res) else "P2a") if n + 4 <= N else "P3c")
    return frozenset(paths)


@functools.lru_cache(maxsize=None)
def fwd_inputs(M, N, K, bmax=A_MAX):
    """The host arrays of every case at one shape (shared across kernels, variants and dtypes; never modified): integer operands and
    their exact product, the EXACT addends, and the integer addends of the fused-norm family."""
    a, b = exact_operands((M, K), (N, K), seed=7919 * M + 31 * N + K + 3 * bmax, bmax=bmax)
    g = np.random.default_rng(13 * M + N)
    t = {"a": a, "b": b, "acc": product64(a, b), "cb": sixty_fourths(g, N + 1), "rb": sixty_fourths(g, M), "res": sixty_fourths(g, M, N),
         "rs": power_of_two(g, N), "row_scale": power_of_two(g, M), "rowadd7": sixty_fourths(g, 7, N), "rowadd32": sixty_fourths(g, 32, N),
         "gadd": sixty_fourths(g, FWD_GADD_ROWS, N), "gidx": np.resize(np.array(FWD_GADD_INDEX, dtype=np.int64), -(-M // FWD_GADD_DIV)),
         "icb": g.integers(-2, 3, N + 1).astype(np.float32), "ires": g.integers(-2, 3, (M, N)).astype(np.float32),
         "irs": np.ldexp(1.0, g.integers(0, 2, N)).astype(np.float32)}
    for v in t.values():
        v.setflags(write=False)
    return t


FWD_FAULTS = ("rowadd_next_row", "rowadd_mod16", "gadd_next_row", "bias_shift4", "res_scale_shift4", "quads_permuted", "subtiles_swapped",
              "slots_swapped", "slot48_over_64", "bf16_rounded_twice")


@functools.lru_cache(maxsize=None)
def fwd_reference(M, N, K, ops, bias_lead=0, fault=None):
    """(y, v): the float64 result of an operator set on fwd_inputs and the pre-activation, step by step as the descriptor defines it.
    `fault`: the result a kernel with that addressing mistake would give (FWD_FAULTS; the slot and rounding faults act on
    fwd_slots / fwd_bf16_bits instead).  The tests must be able to tell each from the true result."""
    spec = FWD_OPS[ops]
    t = fwd_inputs(M, N, K, spec.get("bmax", A_MAX))
    fused = bool(spec.get("fused"))
    rows = np.arange(M)
    v = t["acc"] * float(np.float32(spec.get("alpha", 1.0)))
    if spec.get("row_scale"):
        v = v * t["row_scale"].astype(np.float64)[:, None]
    if spec.get("row_bias"):
        v = v + t["rb"].astype(np.float64)[:, None]
    if spec.get("col_bias"):
        cb = t["icb" if fused else "cb"].astype(np.float64)[bias_lead: bias_lead + N]
        v = v + (np.roll(cb, -4) if fault == "bias_shift4" else cb)[None, :]
    y = gelu64(v) if spec.get("gelu") else v
    if spec.get("res"):
        r = t["ires" if fused else "res"].astype(np.float64)
        if spec.get("res_scale"):
            rs = t["irs" if fused else "rs"].astype(np.float64)
            r = r * (np.roll(rs, -4) if fault == "res_scale_shift4" else rs)[None, :]
        y = y + r
    if spec.get("rowadd"):
        p = spec["rowadd"]
        idx = {"rowadd_next_row": (rows + 1) % p, "rowadd_mod16": (rows % 16) % p}.get(fault, rows % p)
        y = y + t[f"rowadd{p}"].astype(np.float64)[idx]
    if spec.get("gadd"):
        grp = np.minimum((rows + 1) // FWD_GADD_DIV, len(t["gidx"]) - 1) if fault == "gadd_next_row" else rows // FWD_GADD_DIV
        y = y + t["gadd"].astype(np.float64)[t["gidx"][grp]]
    if fault == "quads_permuted":            # the column quads of every whole 16-column group in the order (0, 2, 1, 3)
        y = y.copy()
        for n0 in range(0, N - 15, 16):
            y[:, n0 + 4: n0 + 12] = np.concatenate([y[:, n0 + 8: n0 + 12], y[:, n0 + 4: n0 + 8]], axis=1)
    if fault == "subtiles_swapped":          # the two 16-column sub-tiles of every whole pair
        y = y.copy()
        for n0 in range(0, N - 31, 32):
            y[:, n0: n0 + 32] = np.concatenate([y[:, n0 + 16: n0 + 32], y[:, n0: n0 + 16]], axis=1)
    y.setflags(write=False)
    v.setflags(write=False)
    return y, v


def fwd_slots(x, cols, fault=None) -> np.ndarray:
    """Float64 row sums of squares of x [M, N] over consecutive groups of `cols` columns: [M, N / cols]."""
    x2 = np.asarray(x, dtype=np.float64) ** 2
    M, N = x2.shape
    if fault == "slot48_over_64":            # a 48-column slot that sums the 64 columns from its start
        return np.stack([x2[:, s * cols: s * cols + 64].sum(1) for s in range(N // cols)], axis=1)
    s = x2.reshape(M, N // cols, cols).sum(2)
    if fault == "slots_swapped":             # the slots of two neighbouring column groups
        s = s.reshape(M, -1, 2)[:, :, ::-1].reshape(M, -1)
    return s


def fwd_bf16_bits(y, fault=None, extra=4) -> np.ndarray:
    """bf16 patterns of the f32 of y, round to nearest even.  'bf16_rounded_twice': the f32 is first cut (toward zero) to `extra` bits
    more than bf16 keeps, and that is rounded -- a value just above a tie loses what lifts it and goes to even.  (extra = 16 is the
    f32 itself, and the EXACT results are f32 values -- multiples of 2^-7 of magnitude mostly below 2^7, 14 bits -- so no EXACT
    input can see that one; an intermediate of 4 extra bits is what every set with a fractional addend tells from a single
    rounding: tests/test_gemm_ref_host.py.)"""
    f = np.ascontiguousarray(y, dtype=np.float32)
    if fault == "bf16_rounded_twice":
        f = (f.view(np.uint32) & np.uint32((0xFFFFFFFF << (16 - extra)) & 0xFFFFFFFF)).view(np.float32)
    return bf16_bits(f).reshape(np.shape(y))


def fwd_fill_desc(d, L, case: FwdCase, ptr: dict):
    """Fill the tribe_gemm_desc mirror `d` (L: tribe_hip._lib) for a case from base addresses: ptr['a'], ['b'], ['c'] and one per entry
    of fwd_inputs that the set uses (laid out with the pitches of fwd_layout), ['c_bf16'] and ['row_sumsq'] for the fused-norm set.
    The GPU test passes device buffers, the host test made-up 16-byte aligned addresses (the planner reads no memory)."""
    spec, lay = FWD_OPS[case.ops], fwd_layout(case)
    fused, esz = bool(spec.get("fused")), 4 if case.out == "f32" else 2
    d.M, d.N, d.K, d.batch1, d.batch0 = case.M, case.N, case.K, 1, 1
    d.A, d.lda, d.B, d.ldb = ptr["a"], lay["lda"], ptr["b"], lay["ldb"]
    d.C, d.ldc, d.c_dtype = ptr["c"] + lay["lead"] * esz, lay["ldc"], L.F32 if case.out == "f32" else L.BF16
    d.alpha, d.tile_hint = spec.get("alpha", 1.0), case.hint
    if spec.get("col_bias"):
        d.bias, d.bias_mode = ptr["icb" if fused else "cb"] + 4 * lay["bias_lead"], L.BIAS_COL
    if spec.get("row_bias"):
        d.bias, d.bias_mode = ptr["rb"], L.BIAS_ROW
    if spec.get("row_scale"):
        d.row_scale = ptr["row_scale"]
    if spec.get("gelu"):
        d.act = L.ACT_GELU
    if spec.get("res"):
        d.res, d.ldres = (d.C if lay["inplace"] else ptr["ires" if fused else "res"]), lay["ldres"]
    if spec.get("res_scale"):
        d.res_scale = ptr["irs" if fused else "rs"]
    if spec.get("rowadd"):
        d.rowadd, d.ld_rowadd, d.rowadd_period = ptr[f"rowadd{spec['rowadd']}"], lay["ld_rowadd"], spec["rowadd"]
    if spec.get("gadd"):
        d.gadd, d.gadd_index, d.gadd_div, d.ld_gadd = ptr["gadd"], ptr["gidx"], FWD_GADD_DIV, lay["ld_gadd"]
    if fused:
        d.c_bf16, d.ld_c_bf16, d.row_sumsq, d.ld_row_sumsq = ptr["c_bf16"], lay["ld_c_bf16"], ptr["row_sumsq"], lay["ld_row_sumsq"]
    return d
