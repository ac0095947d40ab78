"""GPU: the element-wise loss family (nn.L1Loss, nn.SmoothL1Loss(beta), nn.HuberLoss(delta), nn.MSELoss; mean | sum) against
float64 restatements: torch.nn.functional.{l1_loss, smooth_l1_loss, huber_loss, mse_loss} on CPU f64 copies of the inputs, and f64
autograd for the gradient.  The reference project builds these losses with getattr(torch.nn, name), so torch's own f64 is the reference.

Every launch form is reached by size and alignment only: one partly filled workgroup (n <= 5, with and without a float4), the float4
remainder loop and the n % 4 tail (4097, 16_500), the grid sized to n at the reference's batch (16 x 1000 x 100: 391 workgroups, one
trip of the unrolled loop), a grid near the cap (64 x 1000 x 100), the capped 2048-workgroup grid running its unrolled loop three
times (N_CAPPED), and the scalar form for inputs that are 4- but not 16-byte aligned.

Bounds (u = 2^-24, one f32 rounding):
  * forward: each term is a few f32 operations on the pair (<= 4 u relative), terms are added in f32 chains of at most 16 (<= 16 u of
    a sum of non-negative terms, so relative to the result), the chains in f64, the result rounded once to f32: <= ~21 u = 1.3e-6.
    The bound is the project's standing 1e-5 relative for "f32 terms in f32 chains of <= 16, then f64": it is ~8 x that worst case and
    far below what a wrong branch, a wrong 1 / n or a dropped 1 / beta leaves.
  * backward: d = p - t (u), the clamp is exact, times k = gs * num / den (2 u, num / den the factor common to all elements) and one product (u): 4 u relative per element;
    rtol 1e-4, atol 0, the existing loss-gradient bound.  atol = 0 makes an exact zero of the reference an exact zero here.
    An element within u |d| of the clamp point may take the other branch than f64 does: there both branches agree to u as well.
"""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import tribe_ref  # noqa: E402

# csrc/robust_loss.hip: FWD_UNROLL float4 pairs per lane and trip, 256 lanes, at most FWD_MAX_WG workgroups
FWD_UNROLL, FWD_MAX_WG, LANES = 4, 2048, 256
N_CAPPED = 3 * (FWD_UNROLL * 4 * FWD_MAX_WG * LANES) + 4 * 300_001 + 3     # three trips, a float4 remainder, a 3-element tail
SIZES = [1, 3, 4, 5, 4097, 16_500, 16 * 1000 * 100, 64 * 1000 * 100, N_CAPPED]
# (kind, parameter): beta for smooth_l1, delta for huber
CASES = [("l1", None), ("smooth_l1", 1.0), ("smooth_l1", 0.05), ("smooth_l1", 0.0), ("huber", 1.0), ("huber", 0.3), ("mse", None)]
REDUCTIONS = ["mean", "sum"]
GS = 0.75            # upstream gradient


def f32(v: float) -> float:
    """The value a float argument of the C ABI arrives with."""
    return float(np.float32(v))


def _call(name: str, *args) -> None:
    from tribe_hip._lib import check, lib

    check(getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    return _ops


@functools.lru_cache(maxsize=1)
def _base(n: int):
    """As test_mse_fwd_bwd: true = 0.8 N(0, 1) + 0.5 pred, every 7th element exactly equal (zeros of the gradient, L1's sign(0))."""
    g = torch.Generator().manual_seed(n % 100_003)
    pred = torch.randn(n, generator=g)
    true = torch.randn(n, generator=g).mul_(0.8).add_(pred, alpha=0.5)
    true[3::7] = pred[3::7]
    return pred, true


def _data(n: int, c: float):
    """The base pair plus elements planted exactly on the clamp point c (an f32 value) with both signs: d = +c, -c, +c at indices
    1, 2, 4, and for c = 1 the pairs (1.5, 0.5) and (-0.25, 0.75) at 5 and 6.  All of these differences are exact in f32."""
    pred, true = (x.clone() for x in _base(n))
    c = f32(c)
    for i, (p, t) in ((1, (c, 0.0)), (2, (0.0, c)), (4, (2 * c, c))):
        if i < n:
            pred[i], true[i] = p, t
    if c == 1.0 and n > 6:
        pred[5], true[5] = 1.5, 0.5
        pred[6], true[6] = -0.25, 0.75
    return pred, true


def _reference(kind: str, param, reduction: str, p64: torch.Tensor, t64: torch.Tensor) -> torch.Tensor:
    if kind == "l1":
        return F.l1_loss(p64, t64, reduction=reduction)
    if kind == "smooth_l1":
        return F.smooth_l1_loss(p64, t64, reduction=reduction, beta=f32(param))
    if kind == "huber":
        return F.huber_loss(p64, t64, reduction=reduction, delta=f32(param))
    return F.mse_loss(p64, t64, reduction=reduction)


def _check_pair(ops, kind, param, pred, true, pd, td, dp, what):
    """Forward (value, run-to-run bits) and backward of one (kind, param) on host pair (pred, true) = device pair (pd, td), both
    reductions; dp is the NaN-prefilled device buffer the gradient goes to."""
    n = pred.numel()
    c = 0.0 if param is None else param
    t64 = true.double()
    for reduction in REDUCTIONS:
        p64 = pred.double().requires_grad_()
        ref = _reference(kind, param, reduction, p64, t64)
        out = ops.elem_loss(pd, td, kind, c, reduction)
        again = ops.elem_loss(pd, td, kind, c, reduction)
        got = float(out)
        err = abs(got - float(ref)) / float(ref)
        print(f"{what} {reduction}: loss {got:.9g} vs f64 {float(ref):.9g}, rel err {err:.2e}")
        assert err <= 1e-5, f"{what} {reduction}: {got} vs {float(ref)}"
        assert torch.equal(out.view(torch.int32), again.view(torch.int32)), f"{what} {reduction}: two calls differ in bits"
        (grad,) = torch.autograd.grad(ref, p64, torch.tensor(GS, dtype=torch.float64))
        dp.fill_(float("nan"))
        gsd = torch.tensor([GS], device="cuda")
        _call("tribe_elem_loss_bwd", pd.data_ptr(), td.data_ptr(), n, ops.ELEM_LOSS_KINDS[kind], c, ops.ELEM_LOSS_REDUCTIONS[reduction],
              gsd.data_ptr(), dp.data_ptr())
        got_grad = dp.cpu().double()
        nz = grad != 0
        worst = float(((got_grad[nz] - grad[nz]).abs() / grad[nz].abs()).max()) if nz.any() else 0.0
        print(f"{what} {reduction}: gradient worst rel err {worst:.2e}, {int((~nz).sum())} exact zeros")
        torch.testing.assert_close(got_grad, grad, rtol=1e-4, atol=0)
        assert (got_grad[~nz] == 0).all()


@pytest.mark.parametrize("kind, param", CASES)
@pytest.mark.parametrize("n", SIZES)
def test_elem_loss_fwd_bwd(ops, n, kind, param):
    c = 1.0 if not param else param                       # L1 / MSE / beta == 0 get the c = 1 plants too
    pred, true = _data(n, c)
    if param and n >= 4097:
        # each regime must hold a real share of the elements, or a kernel with one branch wrong could pass: >= 15 % each
        linear = float(((pred.double() - true.double()).abs() > f32(param)).double().mean())
        print(f"{kind}({param}) n={n}: linear share {linear:.3f}")
        assert 0.15 <= linear <= 0.85, f"{kind}({param}) n={n}: linear regime holds {linear:.1%}"
    pd, td = pred.cuda(), true.cuda()
    assert pd.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    dp = torch.empty(n, device="cuda")
    _check_pair(ops, kind, param, pred, true, pd, td, dp, f"{kind}({param}) n={n}")


@pytest.mark.parametrize("kind, param", CASES)
@pytest.mark.parametrize("which", ["both", "true_only", "grad_only"])
def test_elem_loss_four_byte_aligned_inputs(ops, kind, param, which):
    """x[1:] of an n + 1 buffer, n % 4 != 0: a contiguous input 4 bytes past a 16-byte boundary takes the scalar form, forward and
    backward; so does a pair of which only one side, or only the gradient buffer (backward), is off."""
    n = 1_000_002
    assert n % 4 != 0
    pred, true = _data(n, 1.0 if not param else param)

    def dev(x: torch.Tensor, off: bool) -> torch.Tensor:
        buf = torch.zeros(n + 1, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[1:] if off else buf[:n]
        v.copy_(x)
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if off else 0)
        return v

    pd, td = dev(pred, which == "both"), dev(true, which in ("both", "true_only"))
    dp = dev(torch.zeros(n), which in ("both", "grad_only"))
    _check_pair(ops, kind, param, pred, true, pd, td, dp, f"{kind}({param}) {which} misaligned")


def test_modules_on_matrices_and_bvt(ops):
    """HuberLoss on the reference's [(B T'), V] matrices and on the un-flattened [B, V, T'] pair: the same sum in another order of
    partials, so both are within the forward bound of f64 nn.HuberLoss on the '(b t) d' flatten, and of each other."""
    from modeling_utils.losses import HuberLoss, L1Loss, MSELoss, SmoothL1Loss

    g = torch.Generator().manual_seed(5)
    B, V, T = 5, 33, 21
    p = torch.randn(B, V, T, generator=g)
    t = 0.5 * p + 0.8 * torch.randn(B, V, T, generator=g)
    x64, y64 = tribe_ref.flatten_bt(p).double(), tribe_ref.flatten_bt(t).double()
    for ours, theirs in ((HuberLoss(), torch.nn.HuberLoss()), (HuberLoss("sum", delta=0.3), torch.nn.HuberLoss("sum", delta=f32(0.3))),
                         (SmoothL1Loss(beta=0.05), torch.nn.SmoothL1Loss(beta=f32(0.05))), (L1Loss(), torch.nn.L1Loss()),
                         (MSELoss(reduction="sum"), torch.nn.MSELoss(reduction="sum"))):
        p64 = p.double().requires_grad_()
        ref = theirs(tribe_ref.flatten_bt(p64), y64)
        ref.backward()
        flat = float(ours(tribe_ref.flatten_bt(p).contiguous().cuda(), tribe_ref.flatten_bt(t).contiguous().cuda()))
        flat_strided = float(ours(tribe_ref.flatten_bt(p.cuda()), tribe_ref.flatten_bt(t.cuda())))   # non-contiguous views
        pg = p.cuda().requires_grad_()
        loss = ours.forward_bvt(pg, t.cuda())
        bvt = float(loss)
        print(type(ours).__name__, ours.reduction, flat, flat_strided, bvt, float(ref))
        for got in (flat, flat_strided, bvt):
            assert abs(got - float(ref)) <= 1e-5 * float(ref)
        assert abs(flat - bvt) <= 1e-5 * abs(bvt)
        loss.backward()
        assert pg.grad.shape == (B, V, T) and pg.grad.is_contiguous()
        torch.testing.assert_close(pg.grad.cpu().double(), p64.grad, rtol=1e-4, atol=0)
        assert x64.shape == (B * T, V)


class _HuberByHand(torch.nn.Module):
    """A loss hip_loss_for declines (not one of the four stock types): the step's foreign-loss branch."""

    def __init__(self, delta: float):
        super().__init__()
        self.inner = torch.nn.HuberLoss(reduction="none", delta=delta)

    def forward(self, pred, true):
        return self.inner(pred, true).mean()


@pytest.mark.parametrize("name, kwargs", [("SmoothL1Loss", {}), ("HuberLoss", {"delta": 0.5})])
def test_training_step_routes_grid_losses_through_hip(ops, monkeypatch, name, kwargs):
    """BrainModule with the stock module TorchLossConfig builds: training_step + backward against the CPU oracle's model with
    torch.nn.functional's loss on the '(b t) d' flatten.  Bounds of tests/test_gpu_training.py: loss within 2e-3 * max(1, loss_ref),
    per-tensor gradient error <= 6e-2 (bf16 GEMM operands; both losses have Lipschitz gradients, so that noise is not amplified)."""
    from algonauts2025.model import FmriEncoderConfig
    from algonauts2025.pl_module import BrainModule
    from data_utils.dataloader import SegmentData
    from modeling_utils.losses import TorchLossConfig, hip_loss_for

    fdims = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
    V, Tout, S, B, T = 50, 10, 3, 4, 31
    dims = tribe_ref.EncoderDims(hidden=768, depth=2, heads=4)
    ref = tribe_ref.FmriEncoderRef(fdims, V, Tout, S, dims=dims).train()
    with torch.no_grad():
        tribe_ref.fill_params_(ref, seed=2)
    model = FmriEncoderConfig(n_subjects=S, hidden=768, depth=2, heads=4).build(fdims, V, Tout)
    model.load_state_dict(ref.state_dict())
    model = model.cuda().train()
    data = tribe_ref.synthetic_batch(B, T, fdims, S, seed=4)
    fmri = torch.randn(B, V, Tout, generator=torch.Generator().manual_seed(9))
    fn = {"SmoothL1Loss": F.smooth_l1_loss, "HuberLoss": F.huber_loss}[name]
    loss_ref = fn(tribe_ref.flatten_bt(ref(data)), tribe_ref.flatten_bt(fmri), **kwargs)
    loss_ref.backward()

    calls = []
    real = ops.elem_loss

    def counted(*args, **kw):
        calls.append(args[2:])
        return real(*args, **kw)

    monkeypatch.setattr(ops, "elem_loss", counted)
    stock = TorchLossConfig(name=name, kwargs=kwargs).build()
    assert type(stock).__module__.startswith("torch.nn")
    bm = BrainModule(model, stock, None, {})
    batch = SegmentData(data={**{k: v.cuda() for k, v in data.items()}, "fmri": fmri.cuda()}, segments=[None] * B)
    loss = bm.training_step(batch, 0)
    assert bm.loss is stock and len(calls) == 1, calls
    assert float(bm.logged["train/loss"]) == float(loss)
    print(name, "train/loss", float(loss), "oracle", float(loss_ref))
    assert loss.requires_grad and abs(float(loss) - float(loss_ref)) < 2e-3 * max(1.0, float(loss_ref))
    loss.backward()
    assert len(calls) == 1
    ref_grads = dict(ref.named_parameters())
    worst = {}
    for pname, p in model.named_parameters():
        want = ref_grads[pname].grad
        if want is None:
            continue
        assert p.grad is not None, f"no gradient for {pname}"
        a, b = p.grad.cpu().double().flatten(), want.double().flatten()
        worst[pname] = float((a - b).norm() / (b.norm() + 1e-30))
    print("max grad rel err", max(worst.values()), "over", len(worst), "tensors")
    bad = {k: v for k, v in worst.items() if v > 6e-2}
    assert not bad, f"gradient mismatch: {bad}"

    # the foreign-loss branch is still there for what hip_loss_for declines: same loss, no call of the new op
    by_hand = _HuberByHand(**kwargs) if name == "HuberLoss" else _HuberByHand(1.0)     # SmoothL1(beta = 1) is Huber(delta = 1)
    assert hip_loss_for(by_hand) is None
    model.zero_grad(set_to_none=True)
    bm_foreign = BrainModule(model, by_hand, None, {})
    loss_foreign = bm_foreign.training_step(batch, 0)
    assert len(calls) == 1, "the foreign-loss branch must not reach ops.elem_loss"
    print("foreign branch", float(loss_foreign), "HIP", float(loss))
    assert abs(float(loss_foreign) - float(loss)) <= 1e-5 * abs(float(loss))
    loss_foreign.backward()
    assert all(p.grad is not None for pname, p in model.named_parameters() if ref_grads[pname].grad is not None)
    # a second step of the first module calls the op once more (the counterpart is cached, not the result)
    bm.training_step(batch, 1)
    assert len(calls) == 2
