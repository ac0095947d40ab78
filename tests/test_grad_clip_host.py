"""CPU: the clipping rule the HIP kernels implement, pinned against torch in float64, and the host side of gradient clipping
(the fallback route of modeling_utils.optim.clip_grad_norm_ / clip_grad_value_, the Trainer's arguments, the declared symbols)."""

import math
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(300, 17), (5,), (16385,), (1,)]


def clip_rule_f64(grads, max_norm, norm_type):
    """The rule as tribe_grad_norm states it, in float64: (norm, min(1, max_norm / (norm + 1e-6)))."""
    flat = torch.cat([g.detach().double().flatten() for g in grads])
    norm = float(flat.abs().max()) if norm_type == math.inf else math.sqrt(float((flat * flat).sum()))
    return norm, min(1.0, max_norm / (norm + 1e-6))


def _params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in SHAPES]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, dtype=dtype)
    return params


@pytest.mark.parametrize("norm_type", [2.0, math.inf])
@pytest.mark.parametrize("clips", [True, False])
def test_float64_rule_matches_torch_clip_grad_norm(norm_type, clips):
    """The restated rule against torch's function and against this package's (which hands float64 CPU tensors to torch's)."""
    from modeling_utils.optim import clip_grad_norm_

    params, again = _params(torch.float64), _params(torch.float64)
    before = [p.grad.clone() for p in params]
    norm, _ = clip_rule_f64(before, 1.0, norm_type)
    max_norm = norm * (0.25 if clips else 4.0)
    norm, coef = clip_rule_f64(before, max_norm, norm_type)
    assert (coef < 1.0) == clips
    got = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type)
    assert abs(float(got) - norm) <= 1e-12 * norm
    for p, g in zip(params, before):
        torch.testing.assert_close(p.grad, g * coef, rtol=1e-12, atol=0.0)
    assert torch.equal(clip_grad_norm_(again, max_norm, norm_type), got) and all(torch.equal(p.grad, q.grad) for p, q in zip(again, params))


def test_cpu_tensors_take_torchs_own_route_bit_for_bit():
    from modeling_utils.optim import clip_grad_norm_, clip_grad_value_

    for norm_type in (2.0, math.inf, 3.0):
        mine, ref = _params(torch.float32), _params(torch.float32)
        a, b = clip_grad_norm_(mine, 0.5, norm_type), torch.nn.utils.clip_grad_norm_(ref, 0.5, norm_type)
        assert torch.equal(a, b) and all(torch.equal(p.grad, q.grad) for p, q in zip(mine, ref))
    mine, ref = _params(torch.float32), _params(torch.float32)
    mine[1].grad = ref[1].grad = None                                  # a parameter without a gradient is left out
    mine[0].grad[0, :3] = ref[0].grad[0, :3] = torch.tensor([math.nan, math.inf, -3.0])
    assert clip_grad_value_(mine, 0.25) is None
    torch.nn.utils.clip_grad_value_(ref, 0.25)
    assert mine[1].grad is None
    for p, q in zip(mine[:1] + mine[2:], ref[:1] + ref[2:]):
        torch.testing.assert_close(p.grad, q.grad, rtol=0.0, atol=0.0, equal_nan=True)
    assert math.isnan(float(mine[0].grad[0, 0])) and float(mine[0].grad[0, 1]) == 0.25 and float(mine[0].grad[0, 2]) == -0.25
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(mine, 1.0, error_if_nonfinite=True)


def test_no_gradients_give_a_zero_norm():
    from modeling_utils.optim import clip_grad_norm_, clip_grad_value_

    params = [torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(2, 2))]
    for got in (clip_grad_norm_(params, 1.0), clip_grad_norm_([], 1.0)):
        assert got.shape == () and got.dtype == torch.float32 and float(got) == 0.0
    assert clip_grad_value_(params, 1.0) is None


def test_sparse_gradients_raise():
    from modeling_utils.optim import clip_grad_norm_, clip_grad_value_

    p = torch.nn.Parameter(torch.randn(4, 3))
    p.grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="sparse"):
        clip_grad_value_([p], 1.0)


def test_trainer_checks_the_clip_algorithm():
    from algonauts2025.trainer import Trainer

    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(max_epochs=1, gradient_clip_val=1.0, gradient_clip_algorithm="foo")
    assert Trainer(max_epochs=1).gradient_clip_val is None
    assert Trainer(max_epochs=1, gradient_clip_val=0.0).gradient_clip_val is None             # <= 0 disables, as None does
    t = Trainer(max_epochs=1, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert t.gradient_clip_val == 0.5 and t.gradient_clip_algorithm == "value"


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.a, self.b = torch.nn.Linear(6, 8), torch.nn.Linear(8, 3)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))

    def training_step(self, batch, i):
        return (self(batch[:, :6]) - batch[:, 6:]).square().mean()

    def configure_optimizers(self, total_steps=None):
        return torch.optim.Adam(self.parameters(), lr=1e-2)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_cpu_fit_with_clipping_equals_a_hand_written_loop(algorithm):
    from algonauts2025.trainer import Trainer

    g = torch.Generator().manual_seed(2)
    batches = [torch.randn(16, 9, generator=g) * 3.0 for _ in range(4)]
    clip = 0.05
    mine, ref = _Tiny(), _Tiny()
    trainer = Trainer(max_epochs=2, device="cpu", gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    trainer.fit(mine, batches)
    opt, norms = ref.configure_optimizers(), []
    for _ in range(2):
        for i, batch in enumerate(batches):
            opt.zero_grad(set_to_none=True)
            ref.training_step(batch, i).backward()
            if algorithm == "norm":
                norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)))
            else:
                torch.nn.utils.clip_grad_value_(ref.parameters(), clip)
            opt.step()
    for p, q in zip(mine.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    if algorithm == "norm":
        assert min(norms) > clip                                       # every step clipped
        assert [set(r) for r in trainer.history] == [{"epoch", "train/loss", "lr", "grad_norm"}] * 2
        assert trainer.history[-1]["grad_norm"] == norms[-1] and trainer.history[0]["grad_norm"] == norms[3]
    else:
        assert [set(r) for r in trainer.history] == [{"epoch", "train/loss", "lr"}] * 2


def test_clip_symbols_are_declared_and_bound():
    from tribe_hip import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    for name, n_args in (("tribe_grad_norm", 9), ("tribe_grad_scale", 7), ("tribe_adam_step_clipped", 14)):
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)", header)
        assert decl is not None, f"{name} is not declared in include/tribe_hip.h"
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5
    # argument checks come before any launch: no GPU needed
    handle = _lib.lib()
    assert handle.tribe_grad_norm(None, None, None, 1, 0, 1.0, None, None, None) < 0 and b"null pointer" in handle.tribe_last_error()
    assert handle.tribe_grad_scale(None, None, None, 1, None, 0.0, None) < 0
    assert handle.tribe_adam_step_clipped(None, None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, None, 0.0, None) < 0
    one = (_lib.i64 * 1)(0)
    assert handle.tribe_grad_norm(one, one, one, 1, 2, 1.0, one, one, None) < 0 and b"norm_kind" in handle.tribe_last_error()
    assert handle.tribe_grad_norm(one, one, one, 0, 0, 1.0, one, one, None) < 0 and b"chunks" in handle.tribe_last_error()
