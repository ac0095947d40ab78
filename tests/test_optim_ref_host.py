"""CPU: the float64 optimiser statements of oracle/optim_ref.py and their bounds, before tests/test_gpu_optim_bounds.py holds the HIP
kernels to them.

  * the bounds are a CONDITION a correct float32 evaluation meets: adam_step_f32 (numpy, one rounding per operation, no FMA) stays
    within ratio 1.0 of B_p, B_m and B_v on every case of the set (gradient magnitudes 10^k for k in -9, -8, -3, 0, 3; steps 1, 2,
    7, 100000; no decay / L2 / AdamW; lr 1e-4 and 1e-2; 200 000 elements each, exact zeros in g, m and v); likewise the SWA blend;
  * the bounds DISCRIMINATE: each of the slips an Adam kernel is prone to (optim_ref.FAULTS) leaves them on at least one case;
  * adam_step_f64 IS torch's operation: with unrounded scalars it follows float64 torch.optim.Adam / AdamW to 1e-12 over 3 steps.

The worst ratios and the case that rejects each fault are printed (pytest -s)."""

import numpy as np
import pytest
import torch

from oracle import optim_ref as ref

B1, B2 = ref.BETAS
FAULT_INDEX = 100_003        # an element with g, m, v all non-zero (i % 7 = 6, i % 5 = 3, i % 3 = 1)


def _ratios(got, want: ref.AdamRef):
    return tuple(ref.ratio_report(a, b, c) for a, b, c in zip(got, want[:3], want[3:]))


@pytest.fixture(scope="module")
def sweep():
    """One pass over the case set: per case the float64 reference once, the f32 restatement's worst ratios, and every fault not yet
    rejected.  -> (worst ratio per output with its case, {fault: (case, output, ratio)})."""
    worst = {name: (0.0, None) for name in "pmv"}
    rejected: dict[str, tuple] = {}
    moved = []
    for seed, case in enumerate(ref.host_cases()):
        k, step, wd, dec, lr = case
        state = ref.adam_state(ref.HOST_N, k, step, seed)
        args = (*state, lr, B1, B2, ref.EPS, wd, step, dec)
        want = ref.adam_step_f64(*args)
        for name, (r, i) in zip("pmv", _ratios(ref.adam_step_f32(*args), want)):
            if r > worst[name][0]:
                worst[name] = (r, (case, i))
        moved.append((float(np.median(np.abs(want.p - state[0].astype(np.float64)) / want.b_p)), case))
        for fault in ref.FAULTS:
            if fault in rejected or (fault == "decoupled_swapped" and wd == 0.0):
                continue
            got = ref.adam_step_f32(*args, fault=fault, fault_index=FAULT_INDEX)
            for name, (r, i) in zip("pmv", _ratios(got, want)):
                if r > 1.0:
                    rejected[fault] = (case, name, r, i)
                    break
    return worst, rejected, min(moved)


def test_float32_restatement_stays_within_every_bound(sweep):
    worst, _, moved = sweep
    for name, (r, where) in worst.items():
        print(f"adam_step_f32 / B_{name}: worst ratio {r:.3f} at (k, step, wd, decoupled, lr), index = {where}")
    print(f"smallest median |p' - p| / B_p over the cases: {moved[0]:.1f} at {moved[1]}")
    assert all(r <= 1.0 for r, _ in worst.values())
    # in every case the typical element moves by more than its bound, so a stale element shows wherever it sits (the weakest case
    # is AdamW at lr 1e-4 and gradients of 1e-9, where both the decay and the update are a few u |p|)
    assert moved[0] > 1.0


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_bounds_reject_the_fault(sweep, fault):
    _, rejected, _ = sweep
    assert fault in rejected, f"{fault}: inside the bounds on every case of the set"
    case, name, r, i = rejected[fault]
    print(f"{fault}: rejected by B_{name}, ratio {r:.3g} at index {i} of (k, step, wd, decoupled, lr) = {case}")


@pytest.mark.parametrize("coef,clip", [(None, 0.5), (0.37, 0.0), (0.37, 0.5), (1.0, 0.5)])
def test_float32_restatement_with_clipping_stays_within_every_bound(coef, clip):
    """The clipped form: the product g * coef is rounded in the reference too, so the same bounds hold."""
    for seed, (wd, dec) in enumerate(ref.DECAYS):
        state = ref.adam_state(50_000, 0, 7, 500 + seed)
        args = (*state, 1e-2, B1, B2, ref.EPS, wd, 7, dec, coef, clip)
        want = ref.adam_step_f64(*args)
        ratios = _ratios(ref.adam_step_f32(*args), want)
        print(f"coef={coef} clip={clip} wd={wd} decoupled={dec}: p {ratios[0][0]:.3f} m {ratios[1][0]:.3f} v {ratios[2][0]:.3f}")
        assert all(r <= 1.0 for r, _ in ratios)
        if clip and coef in (None, 1.0):         # N(0, 1) against 0.5: about 60 % of the gradients sit on the limit
            assert 0.45 < float(np.mean(np.abs(np.clip(state[1], -clip, clip)) == np.float32(clip))) < 0.7


def test_swa_blend_stays_within_its_bound_and_the_first_update_is_a_copy():
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in (-6, 0, 4):
        avg = (rng.standard_normal(ref.HOST_N) * 10.0**k).astype(np.float32)
        p = (avg + rng.standard_normal(ref.HOST_N) * 10.0 ** (k - rng.integers(0, 4, ref.HOST_N))).astype(np.float32)
        p[::11] = avg[::11]                      # nothing to blend
        avg[5::13] = 0.0
        for w in (1 / 2, 1 / 3, 1 / 1000):
            want, bound = ref.swa_update_f64(avg, p, w)
            r, i = ref.ratio_report(ref.swa_update_f32(avg, p, w), want, bound)
            print(f"swa k={k} w={w:.4g}: worst ratio {r:.3f} at {i}")
            worst = max(worst, r)
            # the bound tells a blend from its neighbours: another weight, or no update at all
            assert ref.ratio_report(ref.swa_update_f32(avg, p, w * (1 + 2.0**-18)), want, bound)[0] > 1.0
            assert ref.ratio_report(avg, want, bound)[0] > 1.0
    assert worst <= 1.0
    junk = np.full(8, np.nan, np.float32)
    want, bound = ref.swa_update_f64(junk, p[:8], 1.0)
    assert np.array_equal(want, p[:8].astype(np.float64)) and not bound.any()


@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.0, True), (0.01, False), (0.01, True)])
def test_adam_step_f64_is_torch_adam(wd, decoupled):
    """Unrounded scalars, float64 state: three steps of torch.optim.Adam / AdamW to 1e-12 relative."""
    g = torch.Generator().manual_seed(11)
    lr, eps, n = 3e-3, 1e-8, 4096
    p_t = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_()
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p_t], lr=lr, betas=(B1, B2), eps=eps, weight_decay=wd)
    p, m, v = p_t.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (step - 2)
        p_t.grad = grad.clone()
        opt.step()
        p, m, v = ref.adam_step_f64(p, grad.numpy(), m, v, lr, B1, B2, eps, wd, step, decoupled, exact_scalars=True)[:3]
        st = opt.state[p_t]
        for mine, theirs in ((p, p_t), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            torch.testing.assert_close(torch.from_numpy(mine), theirs.detach(), rtol=1e-12, atol=0.0)
