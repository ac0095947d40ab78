"""GPU: the optimiser kernels of csrc/backward.hip (adam_step_kernel, adam_step_clipped_kernel, swa_update_kernel) per element
against the float64 statements of oracle/optim_ref.py, on every branch, and HipAdam as a whole against float64 torch.

The kernels are called through the C entry points (tribe_adam_step, tribe_adam_step_clipped, tribe_swa_update) with a table
built here from _lib.ADAM_TENSOR_DTYPE and ops.chunk_work_list, as HipAdam.step builds it, so that a test chooses the step
count, the placement of every buffer and the shadow pointer.  Every p, g, m, v and bf16 shadow lives inside a buffer of its
own, pre-filled with a bit pattern, with at least 8 guard elements on either side.  After every launch: the guards and g are
unchanged bit for bit ("t.g is not written", the clipped kernel included), p', m', v' are finite and element-wise within B_p, B_m,
B_v of adam_step_f64, a shadow holds round-to-nearest-even bf16 of the p' that was written, and a second launch from a fresh
copy of the same state gives the same bits.  The worst |err| / bound and its index are printed per launch (pytest -s).

Branches and the cases that reach them (CHUNK = tribe_adam_chunk_elems(); one table of sizes 1, 3, 5, CHUNK - 1, CHUNK,
CHUNK + 1, CHUNK + 2, 2 CHUNK + 3: a tensor below one float4, tails of 1, 2 and 3, exact chunk fits, a last chunk of 1, 2 and 3
elements, and seven hand-overs between tensors inside one work list):
  vector body (float4) and its n % 4 tail    test_placements[aligned], test_arithmetic[*-aligned], test_clipped[*-aligned]
  scalar branch, one pointer misaligned      test_placements[g_off], [p_off], [m_off], [v_off]   (the branch is the OR of four)
  scalar branch, 8-byte but not 16           test_placements[all_off_by_two]
  shadow, vector body, 8-byte store          test_shadow_stores[aligned-shadow8]                 (pointer % 16 == 8)
  shadow, vector body, 2-byte stores         test_shadow_stores[aligned-shadow2]                 (pointer % 16 == 2)
  shadow, vector tail                        both of the above: every size with n % 4 != 0
  shadow, scalar branch                      test_shadow_stores[g_off-shadow8], [g_off-shadow2]
  no shadow                                  test_shadow_stores[*-none] and every other test without one
  no decay / L2 / AdamW, flag with wd = 0    test_arithmetic[wd0-*], [wd0_flag-*], [l2-*], [adamw-*]
  step 1 (zero moments, c1 = 1 - beta1)      test_arithmetic[*-step1-*]; steps 2, 7 and 100000 (c1 = c2s = 1) beside it
  sqrt(v) ~ eps and below                    gradient magnitudes 1e-8 and 1e-9 inside every test_arithmetic case
  clipped kernel: coef NULL / 0.37 / 1.0     test_clipped[none-*], [0.37-*], [one-*]
  clipped kernel: clamp off / on             test_clipped[*-noclamp-*], [*-clamp0.5-*]           (about 60 % of N(0, 1) clamps)
  NaN, +-inf, g^2 overflowing, g = v = 0     test_special_values: in a float4, at a chunk edge, in the tail
  SWA blend, vector body / tail / elements   test_swa_blend[aligned-*], [avg_off-*], [live_off-*]
  SWA copy (weight == 1) over junk           test_swa_first_update_is_a_copy[*-nan], [*-pattern]
  HipAdam: gradient view into a flat bucket  test_hip_adam_twelve_steps_against_float64
  HipAdam._chunks eviction and revisit       test_hip_adam_presence_patterns_evict_and_revisit_work_lists
  HipAdam: bf16 / non-contiguous gradient    test_hip_adam_converted_gradients

Bounds: oracle/optim_ref.py derives them (u = 2^-24, twice the count of roundings of each output, the errors of m' and den carried
through the update to first order, + 2^-149); tests/test_optim_ref_host.py shows that a plain f32 evaluation reaches at most 0.58
of them and that eps inside the root, c2 for sqrt(c2), a dropped c1, a swapped decay flag, a late L2 term, beta1 for 1 - beta1
and a stale or twice-updated element all leave them.  The trajectories are held to 4 x the distance of float32 torch.optim.Adam
from float64 torch.optim.Adam on the same gradients (the margin tests/test_gpu_fbank.py gives a same-precision restatement: another
equally valid order of roundings, compounding over the steps), and that distance itself to 1e-5 max|p|.  No bound comes from
what a kernel returned.
"""

import functools
import math

import numpy as np
import pytest
import torch

from oracle import optim_ref as ref

pytestmark = pytest.mark.gpu

PAD = 16                              # guard elements in front (plus the offset) and behind (minus it): at least 14
F_PATTERN, H_PATTERN = 0x5A5A5A5A, 0x5A5A
B2, EPS = ref.BETAS[1], ref.EPS
PLACEMENTS = {                        # offsets of (p, g, m, v) in floats from a 16-byte aligned address
    "aligned": (0, 0, 0, 0), "g_off": (0, 1, 0, 0), "p_off": (1, 0, 0, 0), "m_off": (0, 0, 1, 0), "v_off": (0, 0, 0, 1),
    "all_off_by_two": (2, 2, 2, 2),
}
SHADOWS = {"none": None, "shadow8": 4, "shadow2": 1}          # offset in bf16 elements: pointer % 16 == 8 / == 2
DECAY_IDS = {"wd0": (0.0, 0), "wd0_flag": (0.0, 1), "l2": (0.01, 0), "adamw": (0.01, 1)}
LR_BETA1 = ((1e-4, 0.9), (1e-2, 0.85))


@functools.lru_cache(maxsize=None)
def _chunk() -> int:
    from tribe_hip._lib import lib

    return int(lib().tribe_adam_chunk_elems())


def _sizes() -> list[int]:
    c = _chunk()
    return [1, 3, 5, c - 1, c, c + 1, c + 2, 2 * c + 3]


@functools.lru_cache(maxsize=None)
def _states(k: int, step: int):
    """The f32 state of every tensor of the size table, on the CPU.  Computed once, never modified."""
    out = tuple(ref.adam_state(n, k, step, 1000 * (k + 20) + 10 * i + (step % 7)) for i, n in enumerate(_sizes()))
    for arrays in out:
        for a in arrays:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def _refs(k, step, wd, decoupled, lr, beta1, coef=None, clip=0.0):
    return tuple(ref.adam_step_f64(*s, lr, beta1, B2, EPS, wd, step, decoupled, coef, clip) for s in _states(k, step))


class Slot:
    """n f32 (or bf16) elements `off` elements past an aligned address inside a pattern-filled buffer of their own."""

    def __init__(self, n: int, off: int, values: np.ndarray | None = None, half: bool = False, fill: int | None = None):
        self.n, self.start, self.half = n, PAD + off, half
        self.pattern = H_PATTERN if half else F_PATTERN
        self.bits = torch.full((n + 2 * PAD,), self.pattern, dtype=torch.int16 if half else torch.int32, device="cuda")
        assert self.bits.data_ptr() % 16 == 0
        self.view = self.bits.view(torch.bfloat16 if half else torch.float32)[self.start:self.start + n]
        if fill is not None:
            self.bits[self.start:self.start + n] = fill
        if values is not None:
            self.view.copy_(torch.tensor(values))
        assert self.view.data_ptr() % 16 == ((2 if half else 4) * off) % 16 and self.view.is_contiguous()

    @property
    def ptr(self) -> int:
        return self.view.data_ptr()

    def read(self) -> np.ndarray:
        """The n elements as they are now (f32 values, or bf16 bit patterns); the guards are checked on the way."""
        host = self.bits.cpu().numpy()
        inside = host[self.start:self.start + self.n]
        assert (host[:self.start] == self.pattern).all() and (host[self.start + self.n:] == self.pattern).all(), "a guard element changed"
        return inside.copy() if self.half else inside.view(np.float32).copy()


def _call(name: str, *args) -> None:
    from tribe_hip._lib import check, lib

    check(getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()


def _work(slots: list[dict]):
    """(table bytes on the GPU, chunk_tensor, chunk_start) over the slots, built as HipAdam.step builds them."""
    from tribe_hip import _lib, ops

    table = np.zeros(len(slots), dtype=_lib.ADAM_TENSOR_DTYPE)
    for i, s in enumerate(slots):
        table[i] = tuple(s[f].ptr if s.get(f) is not None else 0 for f in "pgmv") + (s["p"].n, s["s"].ptr if s.get("s") is not None else 0)
    owner, start = ops.chunk_work_list([s["p"].n for s in slots], torch.device("cuda"))
    sizes = np.array([s["p"].n for s in slots])
    assert owner.numel() == int(np.sum((sizes + _chunk() - 1) // _chunk()))
    return torch.from_numpy(table.view(np.uint8).reshape(-1)).cuda(), owner, start


def _launch_adam(states, place, shadow_off, lr, beta1, wd, decoupled, step, clipped=False, coef=None, clip=0.0, prescale=False):
    """Fresh buffers holding `states`, one launch over all of them -> the slots.  `clipped`: tribe_adam_step_clipped with `coef` (None =
    NULL) and `clip`.  `prescale`: ops.grad_scale_ on the gradients, then the plain step (what the clipped step must equal)."""
    from tribe_hip import ops

    slots = []
    for p, g, m, v in states:
        s = {f: Slot(len(p), off, a) for f, off, a in zip("pgmv", place, (p, g, m, v))}
        s["s"] = None if shadow_off is None else Slot(len(p), shadow_off, half=True)
        slots.append(s)
    table, owner, start = _work(slots)
    coef_t = None if coef is None else torch.tensor([coef], dtype=torch.float32, device="cuda")
    common = (table.data_ptr(), owner.data_ptr(), start.data_ptr(), owner.numel(), lr, beta1, B2, EPS, wd, step, int(decoupled))
    if clipped:
        _call("tribe_adam_step_clipped", *common, None if coef_t is None else coef_t.data_ptr(), clip)
    else:
        if prescale:
            ops.grad_scale_([s["g"].view for s in slots], coef_t, clip)
        _call("tribe_adam_step", *common)
    return slots


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


def _read(slots):
    """Per tensor {p, m, v, s}: the outputs on the host.  Guards are checked by Slot.read."""
    out = []
    for s in slots:
        out.append({f: s[f].read() for f in ("p", "m", "v", "g")} | {"s": None if s["s"] is None else s["s"].read()})
    return out


def _check_adam(label, states, refs, got, again):
    """The five checks after a launch (see the module docstring); -> the worst ratios."""
    worst = {f: (0.0, None) for f in "pmv"}
    for t, (state, want, out, out2) in enumerate(zip(states, refs, got, again)):
        assert _same(out["g"], state[1]), f"{label}: tensor {t}: the gradient was written"
        for f, w, b in zip("pmv", want[:3], want[3:]):
            r, i = ref.ratio_report(out[f], w, b)
            if r > worst[f][0]:
                worst[f] = (r, (t, i))
            assert _same(out[f], out2[f]), f"{label}: tensor {t}: {f}' differs between two launches"
        if out["s"] is not None:
            bf16 = torch.from_numpy(out["p"]).bfloat16().view(torch.int16).numpy()
            bad = np.flatnonzero(bf16 != out["s"])
            assert bad.size == 0, f"{label}: tensor {t} (n = {len(out['p'])}): shadow != bf16(p') at {bad[:8]} ({bad.size} elements)"
            assert _same(out["s"], out2["s"])
    print(f"{label}: worst |err| / bound  " + "  ".join(f"{f}' {worst[f][0]:.3f} at (tensor, index) {worst[f][1]}" for f in "pmv"))
    for f in "pmv":
        assert worst[f][0] <= 1.0, f"{label}: {f}' leaves its bound: ratio {worst[f][0]:.4g} at (tensor, index) {worst[f][1]}"
    return worst


def _run_and_check(label, k, step, wd, decoupled, lr, beta1, place, shadow_off, clipped=False, coef=None, clip=0.0):
    states = _states(k, step)
    refs = _refs(k, step, wd, decoupled, lr, beta1, coef, clip)
    runs = [_read(_launch_adam(states, place, shadow_off, lr, beta1, wd, decoupled, step, clipped, coef, clip)) for _ in range(2)]
    _check_adam(label, states, refs, runs[0], runs[1])
    return states, refs, runs[0]


GRID_SETTING = dict(k=0, step=7, wd=0.01, decoupled=0, lr=1e-2, beta1=0.85)      # the one setting of the placement and shadow grids


@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_placements(place):
    _run_and_check(f"placement {place}", place=PLACEMENTS[place], shadow_off=None, **GRID_SETTING)


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("place", ["aligned", "g_off"])
def test_shadow_stores(place, shadow):
    _run_and_check(f"shadow {shadow} under {place}", place=PLACEMENTS[place], shadow_off=SHADOWS[shadow], **GRID_SETTING)


@pytest.mark.parametrize("place", ["aligned", "g_off"])
@pytest.mark.parametrize("step", ref.STEPS, ids=lambda s: f"step{s}")
@pytest.mark.parametrize("decay", list(DECAY_IDS))
def test_arithmetic(decay, step, place):
    wd, decoupled = DECAY_IDS[decay]
    all_zero = 0
    for k in ref.MAGNITUDES:
        for lr, beta1 in LR_BETA1:
            states, _, got = _run_and_check(f"{decay} step {step} k {k} lr {lr} beta1 {beta1} {place}", k, step, wd, decoupled, lr, beta1,
                                            PLACEMENTS[place], None)
            if wd == 0.0:
                for (p, g, m, v), out in zip(states, got):
                    z = (g == 0) & (m == 0) & (v == 0)
                    all_zero += int(z.sum())
                    assert _same(out["p"][z], p[z]), "g = m = v = 0 without decay: p must keep its bits"
    assert wd != 0.0 or all_zero > 100


@pytest.mark.parametrize("place,shadow", [("aligned", "shadow8"), ("g_off", "shadow2")])
@pytest.mark.parametrize("clip", [0.0, 0.5], ids=["noclamp", "clamp0.5"])
@pytest.mark.parametrize("coef", [None, 0.37, 1.0], ids=["none", "0.37", "one"])
def test_clipped(coef, clip, place, shadow):
    """tribe_adam_step_clipped within the bounds of adam_step_f64 given the same coefficient and limit, and bit for bit
    ops.grad_scale_ followed by the plain step, shadow included."""
    k, step, lr, beta1 = 0, 7, 1e-2, 0.85
    for wd, decoupled in ((0.0, 0), (0.01, 0), (0.01, 1)):
        label = f"clipped coef {coef} clip {clip} wd {wd} decoupled {decoupled} {place}"
        states, _, fused = _run_and_check(label, k, step, wd, decoupled, lr, beta1, PLACEMENTS[place], SHADOWS[shadow], True, coef, clip)
        if clip:
            share = np.mean(np.concatenate([np.abs(np.clip(s[1] * np.float32(1.0 if coef is None else coef), -clip, clip)) == np.float32(clip)
                                            for s in states]))
            assert coef == 0.37 or 0.45 < share < 0.7, share
        slots = _launch_adam(states, PLACEMENTS[place], SHADOWS[shadow], lr, beta1, wd, decoupled, step, prescale=True, coef=coef, clip=clip)
        for t, (a, s) in enumerate(zip(fused, slots)):
            for f in ("p", "m", "v", "s"):
                assert _same(a[f], s[f].read()), f"{label}: tensor {t}: {f} differs from scale-then-step"


@pytest.mark.parametrize("decay", ["wd0", "l2"])
@pytest.mark.parametrize("place", ["aligned", "g_off"])
def test_special_values(place, decay):
    """g = NaN, +inf, -inf, 1e30 (its square overflows: v' = +inf, m' / den = 0, p' = p_d) and g = v = 0, each inside a float4, on the last
    lane of a chunk and in the element tail: p', m', v' are non-finite exactly where the reference in f32 range is, with the same
    class, and every other element -- the float4 neighbours of a poisoned lane included -- stays within its bound."""
    wd, decoupled = DECAY_IDS[decay]
    c = _chunk()
    n, k, step, lr, beta1 = c + 3, 0, 7, 1e-2, 0.85
    spots = [5, 4 * 77 + 2, c - 1, c + 1, c + 2]
    specials = [math.nan, math.inf, -math.inf, 1e30, 0.0]
    base = ref.adam_state(n, k, step, 77)
    for rot in range(len(spots)):
        p, g, m, v = (a.copy() for a in base)
        for j, at in enumerate(spots):
            g[at] = specials[(j + rot) % len(specials)]
            if g[at] == 0.0:
                v[at] = 0.0
        state = (p, g, m, v)
        want = ref.adam_step_f64(*state, lr, beta1, B2, EPS, wd, step, decoupled)
        got, again = (_read(_launch_adam([state], PLACEMENTS[place], None, lr, beta1, wd, decoupled, step))[0] for _ in range(2))
        assert _same(got["g"], g)
        worst = {}
        for f, w, b in zip("pmv", want[:3], want[3:]):
            o = got[f]
            assert _same(o, again[f])
            for kind, cls in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
                assert np.array_equal(cls(o), cls(w)), f"{f}' {kind} at {np.flatnonzero(cls(o))}, reference at {np.flatnonzero(cls(w))} (rotation {rot})"
            ok = np.isfinite(w)
            assert np.isfinite(b[ok]).all()
            worst[f] = ref.ratio_report(o[ok], w[ok], b[ok])
            assert worst[f][0] <= 1.0, f"{f}' leaves its bound beside a special value: {worst[f]} (rotation {rot})"
        assert np.isnan(want.p).sum() == 3 and np.isinf(want.v).sum() == 3 and np.isnan(want.v).sum() == 1
        huge = np.flatnonzero(g == np.float32(1e30))
        assert np.isposinf(got["v"][huge]).all() and np.isfinite(got["m"][huge]).all()
        if wd == 0.0:
            assert _same(got["p"][huge], p[huge]), "g = 1e30 without decay: m' / inf = 0, p must keep its bits"
        print(f"special values {place} {decay} rotation {rot}: worst |err| / bound of the finite elements  "
              + "  ".join(f"{f}' {worst[f][0]:.3f}" for f in "pmv"))


# ---- SWA --------------------------------------------------------------------------------------------------------------------
SWA_PLACEMENTS = {"aligned": (0, 0), "avg_off": (1, 0), "live_off": (0, 1)}


@functools.lru_cache(maxsize=None)
def _swa_inputs():
    rng = np.random.default_rng(5)
    out = []
    for n in _sizes():
        avg = rng.standard_normal(n).astype(np.float32)
        live = (avg + rng.standard_normal(n) * 10.0 ** -rng.integers(0, 4, n)).astype(np.float32)
        live[3::11] = avg[3::11]
        for a in (avg, live):
            a.setflags(write=False)
        out.append((avg, live))
    return tuple(out)


def _launch_swa(place, weight, fill=None):
    slots = [{"p": Slot(len(avg), place[0], None if fill is not None else avg, fill=fill), "g": Slot(len(avg), place[1], live)}
             for avg, live in _swa_inputs()]
    table, owner, start = _work(slots)
    _call("tribe_swa_update", table.data_ptr(), owner.data_ptr(), start.data_ptr(), owner.numel(), weight)
    return [(s["p"].read(), s["g"].read()) for s in slots]


@pytest.mark.parametrize("weight", [1 / 2, 1 / 3, 1 / 1000], ids=["half", "third", "thousandth"])
@pytest.mark.parametrize("place", list(SWA_PLACEMENTS))
def test_swa_blend(place, weight):
    runs = [_launch_swa(SWA_PLACEMENTS[place], weight) for _ in range(2)]
    worst = (0.0, None)
    for t, ((avg, live), (got, live_after), (got2, _)) in enumerate(zip(_swa_inputs(), *runs)):
        assert _same(live_after, live) and _same(got, got2)
        want, bound = ref.swa_update_f64(avg, live, weight)
        r, i = ref.ratio_report(got, want, bound)
        if r > worst[0]:
            worst = (r, (t, i))
    print(f"swa {place} weight {weight:.4g}: worst |err| / bound {worst[0]:.3f} at (tensor, index) {worst[1]}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("junk", ["nan", "pattern"])
@pytest.mark.parametrize("place", list(SWA_PLACEMENTS))
def test_swa_first_update_is_a_copy(place, junk):
    """weight == 1 over a buffer as torch.empty_like leaves it (NaN, or any bits): the live parameter, bit for bit."""
    fill = 0x7FC00000 if junk == "nan" else F_PATTERN
    runs = [_launch_swa(SWA_PLACEMENTS[place], 1.0, fill=fill) for _ in range(2)]
    for (avg, live), (got, live_after), (got2, _) in zip(_swa_inputs(), *runs):
        assert _same(live_after, live) and _same(got, got2)
        assert _same(got, live)


# ---- HipAdam as a whole -----------------------------------------------------------------------------------------------------
TRAINING_SHAPES = [(3072, 257), (5,), (1, 1024, 48), (16385,), (7, 3)]      # test_hip_adam_matches_torch_adam's


def _bar(label, f64, f32_, hip):
    """Per tensor: max|hip - f64| <= 4 max|torch f32 - f64|, and the f32 trajectory itself within 1e-5 max|p| of the f64 one."""
    for i, (a, b, c) in enumerate(zip(f64, f32_, hip)):
        a = a.detach()
        d32 = float((b.detach().double() - a).abs().max())
        dhip = float((c.detach().cpu().double() - a).abs().max())
        scale = float(a.abs().max())
        print(f"{label} tensor {i} {tuple(a.shape)}: max|hip - f64| {dhip:.3e}   max|torch f32 - f64| {d32:.3e}   max|p| {scale:.3e}")
        assert d32 < 1e-5 * scale, "the float32 trajectory is too far from float64 to serve as a bar"
        assert dhip <= 4.0 * d32, f"{label} tensor {i}: {dhip:.3e} > 4 x {d32:.3e}"


@pytest.mark.parametrize("decay", ["wd0", "l2", "adamw"])
def test_hip_adam_twelve_steps_against_float64(decay):
    """12 steps under OneCycleLR (lr and beta1 move every step) on the shapes of test_hip_adam_matches_torch_adam plus a parameter whose
    gradient is a view one float into a flat bucket (the scalar branch while p, m and v are aligned)."""
    from modeling_utils.optim import HipAdam

    wd, decoupled = DECAY_IDS[decay]
    gen = torch.Generator().manual_seed(21)
    shapes = TRAINING_SHAPES + [(1000,)]
    start = [torch.randn(s, generator=gen) for s in shapes]
    f64 = [t.double().clone().requires_grad_() for t in start]
    f32_ = [t.clone().requires_grad_() for t in start]
    hip = [t.clone().cuda().requires_grad_() for t in start]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opts = [cls(f64, lr=1e-3, weight_decay=wd), cls(f32_, lr=1e-3, weight_decay=wd),
            HipAdam(hip, lr=1e-3, weight_decay=wd, decoupled_weight_decay=bool(decoupled))]
    scheds = [torch.optim.lr_scheduler.OneCycleLR(o, max_lr=1e-2, total_steps=13, pct_start=0.3) for o in opts]
    bucket = torch.zeros(1000 + 8, device="cuda")
    for step in range(12):
        for a, b, c in zip(f64, f32_, hip):
            g = torch.randn(a.shape, generator=gen) * 10.0 ** (step % 5 - 2)
            a.grad, b.grad = g.double(), g.clone()
            if c is hip[-1]:
                view = bucket[1:1001]
                view.copy_(g)
                assert view.data_ptr() % 16 == 4 and c.data_ptr() % 16 == 0
                c.grad = view
            else:
                c.grad = g.cuda()
        for o in opts:
            o.step()
        for s in scheds:
            s.step()
        assert opts[2].param_groups[0]["lr"] == opts[0].param_groups[0]["lr"] and opts[2].param_groups[0]["betas"] == opts[0].param_groups[0]["betas"]
    _bar(f"12 steps {decay}", f64, f32_, hip)
    assert [float(opts[2].state[p]["step"]) for p in hip] == [12.0] * len(hip)


PRESENCE_SHAPES = [(257, 33), (1000,), (40, 7), (16385,), (5,)]
# 20 distinct subsets: ten, each followed by its complement.  After every pair all parameters have the same step count again, so
# each subset is ONE launch with a work list of its own (parameters with different counts are launched apart): 20 distinct lists
# against a cache of 16.  Then the first pair again, evicted by now, and one subset more, which leaves the counts unequal.
_HALVES = [tuple(i for i in range(5) if m >> i & 1) for m in range(1, 11)]
PRESENCE = [s for a in _HALVES for s in (a, tuple(i for i in range(5) if i not in a))]
PRESENCE += PRESENCE[:2] + [(0, 2)]


def test_hip_adam_presence_patterns_evict_and_revisit_work_lists():
    from modeling_utils.optim import HipAdam

    class Spy(HipAdam):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            self.misses, self.sizes = [], []

        def _work_list(self, gi, params):
            sig = (gi,) + tuple(p.numel() for p in params)
            if sig not in self._chunks:
                self.misses.append(sig)
            out = super()._work_list(gi, params)
            self.sizes.append(len(self._chunks))
            return out

    assert len(set(PRESENCE[:20])) == 20
    gen = torch.Generator().manual_seed(22)
    start = [torch.randn(s, generator=gen) for s in PRESENCE_SHAPES]
    f64 = [t.double().clone().requires_grad_() for t in start]
    f32_ = [t.clone().requires_grad_() for t in start]
    hip = [t.clone().cuda().requires_grad_() for t in start]
    opts = [torch.optim.Adam(f64, lr=1e-2), torch.optim.Adam(f32_, lr=1e-2), Spy(hip, lr=1e-2)]
    for active in PRESENCE:
        for o in opts:
            o.zero_grad(set_to_none=True)
        for i in active:
            g = torch.randn(PRESENCE_SHAPES[i], generator=gen)
            f64[i].grad, f32_[i].grad, hip[i].grad = g.double(), g.clone(), g.cuda()
        for o in opts:
            o.step()
    spy = opts[2]
    print(f"work lists built: {len(spy.misses)}, distinct: {len(set(spy.misses))}, cached at the end: {len(spy._chunks)}")
    assert max(spy.sizes) == 16 and len(set(spy.misses)) > 16, "the cache never filled: the eviction did not run"
    assert len(spy.misses) > len(set(spy.misses)), "no evicted work list was asked for again"
    _bar("presence patterns", f64, f32_, hip)
    assert [float(spy.state[p]["step"]) for p in hip] == [float(opts[0].state[p]["step"]) for p in f64]


def test_hip_adam_converted_gradients():
    """A bf16 gradient and a transposed (non-contiguous) f32 gradient: the step taken with grad.float().contiguous(), bit for bit."""
    from modeling_utils.optim import HipAdam

    gen = torch.Generator().manual_seed(23)
    start = [torch.randn(64, 48, generator=gen), torch.randn(48, 64, generator=gen)]
    raw = [t.clone().cuda().requires_grad_() for t in start]
    conv = [t.clone().cuda().requires_grad_() for t in start]
    opt_raw, opt_conv = HipAdam(raw, lr=1e-2, weight_decay=0.01), HipAdam(conv, lr=1e-2, weight_decay=0.01)
    for _ in range(3):
        grads = [torch.randn(64, 48, generator=gen).cuda().bfloat16(), torch.randn(64, 48, generator=gen).cuda().t()]
        assert grads[0].dtype == torch.bfloat16 and not grads[1].is_contiguous() and grads[1].shape == raw[1].shape
        raw[0].grad_dtype = None                  # a gradient of another dtype than its parameter has to be allowed explicitly
        for p, q, g in zip(raw, conv, grads):
            p.grad, q.grad = g, g.float().contiguous()
        opt_raw.step(), opt_conv.step()
        for p, q, g in zip(raw, conv, grads):
            assert torch.equal(p.grad, g) and p.grad.dtype == g.dtype                   # the conversion is a copy: p.grad stays
            for a, b in ((p, q), (opt_raw.state[p]["exp_avg"], opt_conv.state[q]["exp_avg"]),
                         (opt_raw.state[p]["exp_avg_sq"], opt_conv.state[q]["exp_avg_sq"])):
                assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    assert not torch.equal(raw[0].detach().cpu(), start[0])
