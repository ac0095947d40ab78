"""GPU: gradient clipping (tribe_grad_norm, tribe_grad_scale, tribe_adam_step_clipped) against float64 on the CPU.

Bounds (derived, none fitted):
  norm         an f32 square is exact in f64 (48 bits); the f64 sum and sqrt add < 1e-12 relative at these sizes; one rounding to f32:
               |norm - ref| <= 2^-23 ref for L2, equality for max-abs
  coefficient  min(1, max_norm / (norm + 1e-6)) formed in f64, one rounding: within 2^-23 relative, exactly 1.0 where the rule gives 1
  scaled g     one rounding of the coefficient and one of the product: |g' - g coef64| <= 2^-22 |g coef64|; zeros stay zero; a
               coefficient of 1 leaves the bits alone
  clamp        exact
  fused step   bit for bit the in-place scale followed by the plain step; against torch.optim.Adam on the CPU the tolerances of
               test_hip_adam_matches_torch_adam (rtol 2e-6, atol 2e-7): the coefficient's rounding is an order below them; per
               element against float64, with the coefficient and the limit given, under the derived bounds of oracle/optim_ref.py
               in tests/test_gpu_optim_bounds.py::test_clipped
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 16384
EPS23, EPS22 = 2.0 ** -23, 2.0 ** -22
SETS = {
    "sizes": [(1,), (5,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 3,)],
    "2d": [(3072, 257)],
    "view": [(CHUNK + 1,)],              # placed one element into its buffer: not 16-byte aligned, the element path
    "big": [(300 * CHUNK,)],             # more than 256 chunks: the second launch's strided loop runs twice
    "single": [(1,)],
}


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """CPU gradients N(0, 1) * 10^k (with a few exact zeros), their float64 L2 norm and max-abs.  Computed once, never modified."""
    g = torch.Generator().manual_seed(100 * sorted(SETS).index(name) + k + 3)
    grads = [torch.randn(s, generator=g) * 10.0 ** k for s in SETS[name]]
    for t in grads:
        if t.numel() > 4:
            t.view(-1)[1::max(2, t.numel() // 3)] = 0.0
    flat = torch.cat([t.double().flatten() for t in grads])
    return grads, math.sqrt(float((flat * flat).sum())), float(flat.abs().max())


def _gpu(name, grads):
    """Fresh GPU copies (of CPU or GPU tensors) with the set's placement: "view" keeps every copy off 16-byte alignment."""
    out = []
    for t in grads:
        if name == "view":
            buf = torch.empty(t.numel() + 8, device="cuda")
            v = buf[1:1 + t.numel()]
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            v.copy_(t)
            out.append(v)
        else:
            out.append(t.to("cuda", copy=True))
    return out


def _rule(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_scaled(got, before, coef64):
    """|g' - g coef64| <= 2^-22 |g coef64| element-wise (zeros therefore stay zero)."""
    for g1, g0 in zip(got, before):
        want = g0.double() * coef64
        err = (g1.cpu().double() - want).abs()
        assert bool((err <= EPS22 * want.abs()).all()), f"worst {float((err / want.abs().clamp_min(1e-300)).max()):.3e} relative"


@pytest.mark.parametrize("k", [-3, 0, 3])
@pytest.mark.parametrize("name", sorted(SETS))
def test_norm_coefficient_and_scaled_gradients_against_float64(name, k):
    from modeling_utils.optim import clip_grad_norm_
    from tribe_hip import ops

    cpu, l2, mx = _case(name, k)
    dev = _gpu(name, cpu)
    for norm_type, ref in ((2.0, l2), (math.inf, mx)):
        # the coefficient below 1, exactly 1, and the norm within 1e-6 of max_norm (the +1e-6 of the rule then decides)
        for max_norm in (0.25 * ref, 4.0 * ref, ref + 5e-7):
            coef64 = _rule(ref, max_norm)
            norm, coef = ops.grad_norm(dev, max_norm, norm_type)
            assert norm.shape == coef.shape == () and norm.dtype == coef.dtype == torch.float32 and norm.is_cuda and coef.is_cuda
            n, c = float(norm), float(coef)
            print(f"{name} k={k} norm_type={norm_type} max_norm={max_norm:.6e}: norm {n!r} ref {ref!r} coef {c!r} rule {coef64!r}")
            if norm_type == 2.0:
                assert abs(n - ref) <= EPS23 * ref
            else:
                assert n == ref
            assert abs(c - coef64) <= EPS23 * coef64
            if coef64 == 1.0:
                assert c == 1.0
            work = _gpu(name, dev)
            ops.grad_scale_(work, coef)
            if c == 1.0:
                assert all(_same_bits(a, b) for a, b in zip(work, dev))
            _check_scaled(work, cpu, coef64)
            # the public function: same kernels on p.grad, the norm returned
            params = [torch.nn.Parameter(torch.empty_like(t)) for t in dev]
            for p, t in zip(params, _gpu(name, dev)):
                p.grad = t
            got = clip_grad_norm_(params, max_norm, norm_type)
            assert _same_bits(got, norm) and all(_same_bits(p.grad, w) for p, w in zip(params, work))
    assert all(_same_bits(a, b.cuda()) for a, b in zip(dev, cpu))          # the norm only reads


@pytest.mark.parametrize("name", ["sizes", "view", "big"])
def test_three_launches_give_identical_bits(name):
    from tribe_hip import ops

    cpu, l2, mx = _case(name, 0)
    dev = _gpu(name, cpu)
    for norm_type, ref in ((2.0, l2), (math.inf, mx)):
        outs, scaled = [], []
        for _ in range(3):
            norm, coef = ops.grad_norm(dev, 0.3 * ref, norm_type)
            work = _gpu(name, dev)
            ops.grad_scale_(work, coef)
            outs.append(torch.stack([norm, coef]))
            scaled.append(work)
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
        for again in scaled[1:]:
            assert all(_same_bits(a, b) for a, b in zip(scaled[0], again))


@pytest.mark.parametrize("name,where", [("sizes", (5, 2 * CHUNK + 2)), ("view", (0, CHUNK)), ("big", (0, 299 * CHUNK + 7)), ("single", (0, 0))])
def test_nan_and_inf_follow_torch(name, where):
    """One NaN: norm and coefficient NaN for both kinds (max-abs must carry it: fmax drops NaN).  One inf: norm inf, coefficient 0,
    finite gradients become 0.  Ordinary float values: nothing here can fault."""
    from modeling_utils.optim import clip_grad_norm_
    from tribe_hip import ops

    cpu, _, _ = _case(name, 0)
    for at in dict.fromkeys(where):
        for bad in (math.nan, math.inf, -math.inf):
            dev = _gpu(name, cpu)
            dev[-1].view(-1)[at] = bad                       # the last tensor: vector body, element tail or a chunk past the 256th
            for norm_type in (2.0, math.inf):
                norm, coef = ops.grad_norm(dev, 1.0, norm_type)
                n, c = float(norm), float(coef)
                if math.isnan(bad):
                    assert math.isnan(n) and math.isnan(c), (name, at, norm_type, n, c)
                else:
                    assert n == math.inf and c == 0.0, (name, at, bad, norm_type, n, c)
                params = [torch.nn.Parameter(torch.empty_like(t)) for t in dev]
                for p, t in zip(params, _gpu(name, dev)):
                    p.grad = t
                with pytest.raises(RuntimeError, match="non-finite"):
                    clip_grad_norm_(params, 1.0, norm_type, error_if_nonfinite=True)
                assert all(_same_bits(p.grad, t) for p, t in zip(params, dev))          # raised before anything was scaled
                got = clip_grad_norm_(params, 1.0, norm_type)
                assert _same_bits(got, norm)
                flat = torch.cat([p.grad.flatten() for p in params]).cpu()
                if math.isnan(bad):
                    assert bool(flat.isnan().all())                                     # as torch: everything times NaN
                else:
                    assert int(flat.isnan().sum()) == 1 and int((flat != 0).sum()) == 1   # inf * 0 = NaN, every finite value -> 0


@pytest.mark.parametrize("name", ["sizes", "2d", "view"])
def test_clip_grad_value_is_torch_clamp_exactly(name):
    from modeling_utils.optim import clip_grad_value_
    from tribe_hip import ops

    cpu, _, _ = _case(name, 0)
    cpu = [t.clone() for t in cpu]
    special = torch.tensor([math.nan, math.inf, -3.0, -math.inf, 3.0, 0.5, -0.5, 0.0])
    cpu[-1].view(-1)[:min(8, cpu[-1].numel())] = special[:min(8, cpu[-1].numel())]
    if cpu[-1].numel() > 12:
        cpu[-1].view(-1)[-3:] = special[:3]                   # the element tail too
    for clip in (0.5, 1e-3):
        params = [torch.nn.Parameter(torch.empty_like(t)) for t in _gpu(name, cpu)]
        for p, t in zip(params, _gpu(name, cpu)):
            p.grad = t
        assert clip_grad_value_(params, clip) is None
        for p, t in zip(params, cpu):
            torch.testing.assert_close(p.grad.cpu(), torch.clamp(t, -clip, clip), rtol=0.0, atol=0.0, equal_nan=True)
    # the kernel under both arguments at once: clamp(g * coef, +-v)
    dev = _gpu(name, cpu)
    coef = torch.tensor(0.37, device="cuda")
    ops.grad_scale_(dev, coef, 0.2)
    for a, t in zip(dev, cpu):
        torch.testing.assert_close(a.cpu(), torch.clamp(t * torch.tensor(0.37), -0.2, 0.2), rtol=0.0, atol=0.0, equal_nan=True)


ADAM_SHAPES = [(3072, 257), (5,), (1, 1024, 48), (16385,), (7, 3)]      # test_hip_adam_matches_torch_adam's


def _clip64(grads, max_norm):
    """float64 oracle of clip_grad_norm_ on CPU f32 gradients: (norm, coefficient, clipped gradients rounded to f32)."""
    flat = torch.cat([g.double().flatten() for g in grads])
    norm = math.sqrt(float((flat * flat).sum()))
    coef = _rule(norm, max_norm)
    return norm, coef, [(g.double() * coef).float() for g in grads]


@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.01, False), (0.01, True)])
@pytest.mark.parametrize("mode", ["norm", "value"])
def test_fused_clipped_step_equals_scale_then_step(wd, decoupled, mode):
    """HipAdam.step(grad_scale=coef) on one copy against ops.grad_scale_ + plain step() on another, five steps under OneCycleLR:
    parameters, exp_avg, exp_avg_sq and bf16 shadows equal bit for bit, p.grad untouched by the fused path; and against torch.optim.Adam /
    AdamW on the CPU fed the float64-clipped gradients."""
    from modeling_utils import shadow
    from modeling_utils.optim import HipAdam
    from tribe_hip import ops

    torch.manual_seed(0)
    ref = [torch.randn(s).requires_grad_() for s in ADAM_SHAPES]
    fused = [p.detach().clone().cuda().requires_grad_() for p in ref]
    plain = [p.detach().clone().cuda().requires_grad_() for p in ref]
    shadows = {}
    for params in (fused, plain):            # bf16 operand copies: an aligned one (4-wide stores) and one a single element into its buffer
        aligned = torch.zeros(params[0].numel(), dtype=torch.bfloat16, device="cuda")
        odd = torch.zeros(params[3].numel() + 4, dtype=torch.bfloat16, device="cuda")[1:1 + params[3].numel()]
        shadow.register(params[0], aligned, lambda version: None)
        shadow.register(params[3], odd, lambda version: None)
        shadows[id(params)] = (aligned, odd)
    kw = dict(lr=1e-3, weight_decay=wd)
    opt_ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, **kw)
    opt_f, opt_p = (HipAdam(ps, decoupled_weight_decay=decoupled, **kw) for ps in (fused, plain))
    scheds = [torch.optim.lr_scheduler.OneCycleLR(o, max_lr=1e-2, total_steps=6, pct_start=0.3) for o in (opt_ref, opt_f, opt_p)]
    max_norm, clip_value = 50.0, 0.8         # the norm is ~9 at step 0 (coefficient exactly 1), then 92, 920, ...: clipped
    try:
        for step in range(5):
            grads = [torch.randn(a.shape) * (10.0 ** (step - 2)) for a in ref]
            for a, b, c, g in zip(ref, fused, plain, grads):
                b.grad, c.grad = g.clone().cuda(), g.clone().cuda()
            if mode == "norm":
                norm64, coef64, clipped = _clip64(grads, max_norm)
                assert (coef64 == 1.0) == (step == 0)
                _, coef_f = ops.grad_norm([p.grad for p in fused], max_norm)
                _, coef_p = ops.grad_norm([p.grad for p in plain], max_norm)
                opt_f.step(grad_scale=coef_f)
                ops.grad_scale_([p.grad for p in plain], coef_p)
            else:
                clipped = [g.clamp(-clip_value, clip_value) for g in grads]
                opt_f.step(grad_clip_value=clip_value)
                ops.grad_scale_([p.grad for p in plain], None, clip_value)
            opt_p.step()
            for a, g in zip(ref, clipped):
                a.grad = g
            opt_ref.step()
            for s in scheds:
                s.step()
            assert opt_f.param_groups[0]["lr"] == opt_ref.param_groups[0]["lr"] and opt_f.param_groups[0]["betas"] == opt_ref.param_groups[0]["betas"]
            for a, b, c, g in zip(ref, fused, plain, grads):
                assert _same_bits(b.grad, g.cuda()), "the fused step must leave p.grad as it was"
                assert _same_bits(b, c) and _same_bits(opt_f.state[b]["exp_avg"], opt_p.state[c]["exp_avg"])
                assert _same_bits(opt_f.state[b]["exp_avg_sq"], opt_p.state[c]["exp_avg_sq"])
                torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=2e-6, atol=2e-7)
                if mode == "value":
                    assert torch.equal(c.grad.cpu(), g.clamp(-clip_value, clip_value))
            for (sa, so), (pa, po) in [(shadows[id(fused)], shadows[id(plain)])]:
                assert torch.equal(sa, pa) and torch.equal(so, po)
                assert torch.equal(sa, fused[0].detach().bfloat16().flatten()) and torch.equal(so, fused[3].detach().bfloat16().flatten())
        assert [float(opt_f.state[p]["step"]) for p in fused] == [5.0] * len(fused)
    finally:
        for params in (fused, plain):
            shadow.forget(params[0]), shadow.forget(params[3])


def test_clipped_step_over_parameter_subsets():
    """A parameter whose grad is None is left out of the norm and not stepped; a late starter keeps its own step count under the
    clipped step (test_hip_adam_late_starting_parameter_keeps_its_own_step_count, with clipping)."""
    from modeling_utils.optim import HipAdam, clip_grad_norm_
    from tribe_hip import ops

    torch.manual_seed(1)
    shapes = [(257, 33), (1000,), (40, 7)]
    ref = [torch.randn(s).requires_grad_() for s in shapes]
    mine = [p.detach().clone().cuda().requires_grad_() for p in ref]
    opt_ref, opt = torch.optim.Adam(ref, lr=1e-2), HipAdam(mine, lr=1e-2)
    present = [[0, 2], [0, 2], [0, 1, 2], [1], [0, 1, 2]]        # parameter 1 joins at step 3; 0 and 2 sit out step 4
    max_norm = 3.0
    for active in present:
        opt_ref.zero_grad(set_to_none=True), opt.zero_grad(set_to_none=True)
        grads = {i: torch.randn(shapes[i]) for i in active}
        norm64, coef64, clipped = _clip64([grads[i] for i in active], max_norm)
        assert coef64 < 1.0
        for i, g in zip(active, clipped):
            ref[i].grad, mine[i].grad = g, grads[i].clone().cuda()
        before = [p.detach().clone() for p in mine]
        norm, coef = ops.grad_norm([p.grad for p in mine if p.grad is not None], max_norm)
        assert abs(float(norm) - norm64) <= EPS23 * norm64 and abs(float(coef) - coef64) <= EPS23 * coef64
        # the public function sees the same subset (it works on copies here: the fused step reads the unscaled gradients)
        shadow_params = [torch.nn.Parameter(p.detach().clone()) for p in mine]
        for q, p in zip(shadow_params, mine):
            q.grad = None if p.grad is None else p.grad.clone()
        assert _same_bits(clip_grad_norm_(shadow_params, max_norm), norm)
        opt_ref.step(), opt.step(grad_scale=coef)
        for i, (a, b) in enumerate(zip(ref, mine)):
            torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=2e-6, atol=2e-7)
            if i not in active:
                assert _same_bits(b, before[i])
    assert [float(opt.state[p]["step"]) for p in mine] == [4.0, 3.0, 4.0]


class _TwoLinear(torch.nn.Module):
    def __init__(self, opt_cls, lr=1e-3):
        super().__init__()
        torch.manual_seed(7)
        self.a, self.b = torch.nn.Linear(12, 16), torch.nn.Linear(16, 4)
        self.opt_cls, self.lr = opt_cls, lr

    def training_step(self, batch, i):
        return (self.b(torch.tanh(self.a(batch[:, :12]))) - batch[:, 12:]).square().mean()

    def configure_optimizers(self, total_steps=None):
        return self.opt_cls(self.parameters(), lr=self.lr)


def _recording_adam():
    from modeling_utils.optim import HipAdam

    class Recording(HipAdam):
        def __init__(self, params, **kw):
            params = list(params)
            super().__init__(params, **kw)
            self.watched, self.start = params, [p.detach().clone() for p in params]
            self.trace, self.kwargs = [], []

        def step(self, closure=None, **kw):
            self.trace.append([p.grad.detach().clone() for p in self.watched])
            self.kwargs.append(kw)
            return super().step(closure, **kw)

    return Recording


def test_trainer_fit_clips_by_global_norm():
    from algonauts2025.trainer import Trainer

    g = torch.Generator().manual_seed(4)
    batches = [torch.randn(32, 16, generator=g) * 2.0 for _ in range(3)]
    clip = 1e-2
    finals = {}
    for reduce in (False, True):             # True: a world of one, gradients are views of the reducer's buckets
        module = _TwoLinear(_recording_adam())
        trainer = Trainer(max_epochs=2, reduce_gradients=reduce, gradient_clip_val=clip, gradient_clip_algorithm="norm")
        trainer.fit(module, batches)
        opt = trainer.optimizers[0]
        assert len(opt.trace) == 6 and all(set(kw) == {"grad_scale"} for kw in opt.kwargs)
        ref = [p.cpu().clone().requires_grad_() for p in opt.start]
        opt_ref = torch.optim.Adam(ref, lr=1e-3)
        for grads in opt.trace:
            norm64, coef64, clipped = _clip64([t.cpu() for t in grads], clip)
            assert coef64 < 1.0, "every step must clip"
            for p, t in zip(ref, clipped):
                p.grad = t
            opt_ref.step()
        for p, q in zip(opt.watched, ref):
            torch.testing.assert_close(p.detach().cpu(), q.detach(), rtol=2e-6, atol=2e-7)
        assert [set(r) for r in trainer.history] == [{"epoch", "train/loss", "lr", "grad_norm"}] * 2
        print(f"reduce={reduce}: history grad_norm {trainer.history[-1]['grad_norm']!r}, float64 norm of the last step {norm64!r}")
        assert abs(trainer.history[-1]["grad_norm"] - norm64) <= EPS23 * norm64
        finals[reduce] = [p.detach().clone() for p in opt.watched]
    assert all(_same_bits(a, b) for a, b in zip(finals[False], finals[True]))


def test_trainer_fit_clips_by_value_and_is_silent_without_clipping():
    from algonauts2025.trainer import Trainer

    g = torch.Generator().manual_seed(5)
    batches = [torch.randn(32, 16, generator=g) * 2.0 for _ in range(3)]
    clip = 1e-3
    module = _TwoLinear(_recording_adam())
    trainer = Trainer(max_epochs=1, reduce_gradients=False, gradient_clip_val=clip, gradient_clip_algorithm="value")
    trainer.fit(module, batches)
    opt = trainer.optimizers[0]
    assert opt.kwargs == [{"grad_clip_value": clip}] * 3
    assert all(float(torch.cat([t.flatten() for t in grads]).abs().max()) > clip for grads in opt.trace)
    ref = [p.cpu().clone().requires_grad_() for p in opt.start]
    opt_ref = torch.optim.Adam(ref, lr=1e-3)
    for grads in opt.trace:
        for p, t in zip(ref, grads):
            p.grad = t.cpu().clamp(-clip, clip)
        opt_ref.step()
    for p, q in zip(opt.watched, ref):
        torch.testing.assert_close(p.detach().cpu(), q.detach(), rtol=2e-6, atol=2e-7)
    assert [set(r) for r in trainer.history] == [{"epoch", "train/loss", "lr"}]

    module = _TwoLinear(_recording_adam())
    trainer = Trainer(max_epochs=1, reduce_gradients=False, gradient_clip_val=None)
    trainer.fit(module, batches)
    assert trainer.optimizers[0].kwargs == [{}] * 3                              # the plain step, as before
    assert [set(r) for r in trainer.history] == [{"epoch", "train/loss", "lr"}]


def test_other_optimisers_are_clipped_in_place():
    """Any optimiser that is not HipAdam: clip_grad_norm_ on p.grad (the HIP kernels for GPU f32 gradients), then its own step."""
    from algonauts2025.trainer import Trainer

    g = torch.Generator().manual_seed(6)
    batches = [torch.randn(32, 16, generator=g) * 2.0 for _ in range(2)]
    clip = 1e-2
    seen = []

    class Sgd(torch.optim.SGD):
        def step(self, closure=None):
            seen.append([p.grad.detach().clone() for grp in self.param_groups for p in grp["params"]])
            return super().step(closure)

    module = _TwoLinear(Sgd, lr=0.1)
    trainer = Trainer(max_epochs=1, reduce_gradients=False, gradient_clip_val=clip)
    trainer.fit(module, batches)
    for grads in seen:
        flat = torch.cat([t.double().flatten() for t in grads]).cpu()
        norm = math.sqrt(float((flat * flat).sum()))
        # already clipped when the optimiser saw them: clip * n / (n + 1e-6) with the norm n > clip, so within 1e-6 / clip below clip
        assert clip * (1.0 - 1.1e-6 / clip) <= norm <= clip * (1.0 + 1e-6)
    assert "grad_norm" in trainer.history[-1] and trainer.history[-1]["grad_norm"] > clip
