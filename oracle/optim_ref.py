"""Float64 statements of the optimiser kernels of csrc/backward.hip (adam_step_kernel, adam_step_clipped_kernel,
swa_update_kernel) with per-element rounding-error bounds.  CPU only: numpy, no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  tests/test_optim_ref_host.py pins adam_step_f64 to float64 torch.optim.Adam /
AdamW, shows that a plain float32 evaluation stays inside the bounds and that the bounds reject the usual slips of an Adam
kernel; tests/test_gpu_optim_bounds.py holds the kernels to them.

The step (torch.optim.Adam's single-tensor rule, the one csrc/backward.hip restates), scalars as the C ABI receives them (f32):

    g_e  = clamp(f32(g * coef), +-clip_value)                       coef None = 1, clip_value <= 0 = no clamp
    L2:    g_e += wd * p              AdamW:  p_d = p * (1 - lr * wd)              (p_d = p otherwise)
    m'   = m + (1 - beta1) * (g_e - m)
    v'   = (1 - beta2) * g_e^2 + beta2 * v
    den  = sqrt(v') / c2s + eps       c1 = f32(1 - beta1^step),  c2s = f32(sqrt(1 - beta2^step)), both formed in double
    upd  = (lr / c1) * m' / den
    p'   = p_d - upd

Bounds (derived, none fitted).  u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u; sqrt and the divide
are correctly rounded.  dg = u (|g| + |wd p|) is the rounding of the L2 sum (0 in the other forms).  The constants are twice the
plain count of roundings, so that they hold whichever products the compiler contracts into FMAs (a contraction only removes
a rounding); every bound gets + 2^-149, the smallest f32 step.

    B_m   = 8u (|m| + |g_e|) + dg                         roundings: 1 - beta1, g_e - m, the product and the sum (4, or 3 as an FMA);
                                                          each is relative to a quantity <= |m| + |g_e|; dg enters times 1 - beta1 < 1
    B_v   = 8u v' + 2 (1 - beta2) |g_e| dg                roundings: 1 - beta2, g_e^2, beta2 v, the product, the sum (5); all terms are
                                                          non-negative, so each is relative to <= v'; d(g_e^2) = 2 |g_e| dg
    B_den = 8u den + B_v / (2 sqrt(v') c2s)               roundings: sqrt, divide, add (3), each relative to <= den; the error of v'
                                                          goes through d sqrt(x) = dx / (2 sqrt(x)); that term is 0 where v' = 0
    B_p   = 2u |p'| + [4u |p_d| AdamW] + 8u |upd|         the final subtraction (1, doubled); lr wd, 1 - lr wd and the product (AdamW);
            + (lr / c1) B_m / den + |upd| B_den / den     lr / c1, m' / den and their product (3, and a spare); then the errors of m'
                                                          and den carried through upd = (lr / c1) m' / den to first order

Overflow rule.  The reference works in float64 but in float32 RANGE: every intermediate that the kernel holds as an f32 (the
scaled gradient, the L2 sum, g_e - m, g_e^2, m', v', den, m' / den, upd, p_d, p') becomes +-inf where its magnitude exceeds the
largest finite f32, and inf / NaN then follow IEEE arithmetic (inf / inf = NaN, x / inf = 0).  So g = 1e30 gives v' = +inf,
den = +inf, upd = 0 and p' = p_d; g = +-inf gives m' = +-inf, v' = +inf and p' = NaN.  Values within half an ulp above the
largest finite f32 (which round down to it) are used by no test.  Where den = +inf the two carried terms of B_p are 0: upd is
exactly 0 there.  The denormal range (gradients below about 1e-19) is outside this statement.
"""

from __future__ import annotations

import itertools
import math
import typing as tp

import numpy as np

U = 2.0**-24          # unit roundoff of f32
TINY = 2.0**-149      # the smallest f32 step
FLT_MAX = float(np.finfo(np.float32).max)

# the case set the bounds are checked on (tests/test_optim_ref_host.py) and the kernels are held to (tests/test_gpu_optim_bounds.py)
MAGNITUDES = (-9, -8, -3, 0, 3)                                   # gradients N(0, 1) * 10^k; sqrt(v) ~ eps at -8
STEPS = (1, 2, 7, 100000)                                         # 1 runs from zero moments
DECAYS = ((0.0, False), (0.01, False), (0.01, True))              # (weight_decay, decoupled): none, L2, AdamW
HOST_LRS = (1e-4, 1e-2)
HOST_N = 200_000
BETAS, EPS = (0.9, 0.999), 1e-8

FAULTS = ("eps_in_sqrt", "c2_for_sqrt_c2", "c1_dropped", "decoupled_swapped", "l2_after_m", "beta1_for_one_minus_beta1",
          "element_skipped", "element_twice")


def f32(x: float) -> float:
    """The value the C ABI receives for a `float` argument."""
    return float(np.float32(x))


def bias_corrections(beta1: float, beta2: float, step: int, exact_scalars: bool = False) -> tuple[float, float]:
    """(c1, c2s) as tribe_adam_step forms them: in double from the f32 betas, then rounded to f32."""
    if exact_scalars:
        return 1.0 - beta1**step, math.sqrt(1.0 - beta2**step)
    b1, b2 = f32(beta1), f32(beta2)
    return f32(1.0 - b1 ** float(step)), f32(math.sqrt(1.0 - b2 ** float(step)))


def _range(x: np.ndarray) -> np.ndarray:
    """The overflow rule: beyond the largest finite f32 is +-inf.  NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > FLT_MAX, np.copysign(np.inf, x), x)


class AdamRef(tp.NamedTuple):
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    b_p: np.ndarray
    b_m: np.ndarray
    b_v: np.ndarray


def adam_step_f64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decoupled, grad_coef=None, clip_value=0.0, *,
                  exact_scalars: bool = False) -> AdamRef:
    """One Adam / AdamW step in float64 on the f32 state, and the bounds of the module docstring.  `exact_scalars` keeps the
    scalars, the bias corrections and the scaled gradient unrounded: the form that is compared with float64 torch."""
    P, G, M, V = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    if not exact_scalars:
        lr, beta1, beta2, eps, weight_decay, clip_value = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay, clip_value))
    c1, c2s = bias_corrections(beta1, beta2, step, exact_scalars)
    decayed = weight_decay != 0.0
    with np.errstate(all="ignore"):
        ge = G
        if grad_coef is not None:
            if exact_scalars:
                ge = G * float(grad_coef)
            else:       # clip_grad rounds the product on purpose (the in-place pass and the fused step must agree): so does the reference
                ge = (np.asarray(g, dtype=np.float32) * np.float32(grad_coef)).astype(np.float64)
        if clip_value > 0.0:
            ge = np.clip(ge, -clip_value, clip_value)
        dg = np.zeros_like(P)
        pd = P
        if decayed and decoupled:
            pd = _range(P * (1.0 - lr * weight_decay))
        elif decayed:
            dg = U * (np.abs(ge) + np.abs(weight_decay * P))
            ge = _range(ge + weight_decay * P)
        m1 = _range(M + (1.0 - beta1) * _range(ge - M))
        v1 = _range((1.0 - beta2) * _range(ge * ge) + beta2 * V)
        root = np.sqrt(v1)
        den = _range(root / c2s + eps)
        upd = _range((lr / c1) * _range(m1 / den))
        p1 = _range(pd - upd)

        b_m = 8 * U * (np.abs(M) + np.abs(ge)) + dg + TINY
        b_v = 8 * U * v1 + 2 * (1.0 - beta2) * np.abs(ge) * dg + TINY
        b_den = 8 * U * den + np.where(v1 > 0, b_v / (2 * root * c2s), 0.0)
        carried = np.where(np.isinf(den), 0.0, (lr / c1) * b_m / den + np.abs(upd) * b_den / den)
        b_p = 2 * U * np.abs(p1) + (4 * U * np.abs(pd) if decayed and decoupled else 0.0) + 8 * U * np.abs(upd) + carried + TINY
    return AdamRef(p1, m1, v1, b_p, b_m, b_v)


def adam_step_f32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decoupled, grad_coef=None, clip_value=0.0, *,
                  fault: str | None = None, fault_index: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The same step in numpy float32, one rounding per operation and no FMA: it exists so that the host test can check the
    bounds (it must stay inside them) and that they discriminate (`fault` injects one of FAULTS and must leave them)."""
    assert fault is None or fault in FAULTS, fault
    F = np.float32
    lr, b1, b2, eps, wd, clip = (F(x) for x in (lr, beta1, beta2, eps, weight_decay, clip_value))
    c1, c2s = (F(x) for x in bias_corrections(float(b1), float(b2), step))
    one = F(1.0)

    def once(P, G, M, V):
        if grad_coef is not None:
            G = G * F(grad_coef)
        if clip > 0:
            G = np.clip(G, -clip, clip)
        l2 = None
        if wd != 0:
            if bool(decoupled) != (fault == "decoupled_swapped"):
                P = P * (one - lr * wd)
            else:
                l2 = wd * P
        if l2 is not None and fault != "l2_after_m":
            G = G + l2
        M1 = M + (b1 if fault == "beta1_for_one_minus_beta1" else one - b1) * (G - M)
        if l2 is not None and fault == "l2_after_m":
            G = G + l2
        V1 = (one - b2) * (G * G) + b2 * V
        if fault == "eps_in_sqrt":
            den = np.sqrt(V1 / (c2s * c2s) + eps)
        elif fault == "c2_for_sqrt_c2":
            den = np.sqrt(V1) / (c2s * c2s) + eps
        else:
            den = np.sqrt(V1) / c2s + eps
        P1 = P - (lr if fault == "c1_dropped" else lr / c1) * (M1 / den)
        return P1, M1, V1

    P, G, M, V = (np.ascontiguousarray(x, dtype=F) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        P1, M1, V1 = once(P, G, M, V)
        i = slice(fault_index, fault_index + 1)
        if fault == "element_skipped":
            P1[i], M1[i], V1[i] = P[i], M[i], V[i]
        elif fault == "element_twice":
            P1[i], M1[i], V1[i] = once(P1[i].copy(), G[i], M1[i].copy(), V1[i].copy())
    assert P1.dtype == M1.dtype == V1.dtype == F
    return P1, M1, V1


def swa_update_f64(avg, p, weight) -> tuple[np.ndarray, np.ndarray]:
    """(avg', bound): avg' = avg + (p - avg) f32(weight).  Four roundings: the weight (relative to the product), the difference,
    the product, the sum: 2u |avg'| + 4u w |p - avg| + 2^-149 is twice their count.  weight == 1 is a copy: avg' = p exactly,
    bound 0, whatever `avg` holds."""
    w = f32(weight)
    A, P = np.asarray(avg).astype(np.float64), np.asarray(p).astype(np.float64)
    if w == 1.0:
        return P.copy(), np.zeros_like(P)
    out = A + (P - A) * w
    return out, 2 * U * np.abs(out) + 4 * U * w * np.abs(P - A) + TINY


def swa_update_f32(avg, p, weight) -> np.ndarray:
    F = np.float32
    A, P = np.ascontiguousarray(avg, dtype=F), np.ascontiguousarray(p, dtype=F)
    return A + (P - A) * F(weight)


def adam_state(n: int, k: int, step: int, seed: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(p, g, m, v) in f32: p ~ N(0, 1), g ~ N(0, 1) 10^k, moments of that scale (zero before step 1).  Exact zeros: g at
    i % 7 == 1, m at i % 5 == 2, v at i % 3 == 0, so every combination occurs and all three are zero at i % 105 == 57."""
    rng = np.random.default_rng(seed)
    s = 10.0**k
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * s).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (rng.standard_normal(n) * (0.3 * s)).astype(np.float32)
        v = (rng.standard_normal(n) ** 2 * (s * s)).astype(np.float32)
    i = np.arange(n)
    g[i % 7 == 1] = 0.0
    m[i % 5 == 2] = 0.0
    v[i % 3 == 0] = 0.0
    return p, g, m, v


def host_cases() -> tp.Iterator[tuple[int, int, float, bool, float]]:
    """(k, step, weight_decay, decoupled, lr) of the case set."""
    for k, step, (wd, dec), lr in itertools.product(MAGNITUDES, STEPS, DECAYS, HOST_LRS):
        yield k, step, wd, dec, lr


def ratio_report(got, want: np.ndarray, bound: np.ndarray) -> tuple[float, int]:
    """Largest |got - want| / bound over all elements and its index; a non-finite value counts as infinitely wrong.  An exact
    match under a zero bound counts as 0."""
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    if r.size == 0:
        return 0.0, -1
    i = int(r.argmax())
    return float(r[i]), i
