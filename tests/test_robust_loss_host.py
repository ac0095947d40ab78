"""CPU (no GPU): the host side of the element-wise loss family (L1 / SmoothL1 / Huber / MSE): the classes and their argument
checks, `hip_loss_for`'s mapping from stock torch modules, the step's routing decision, and the C ABI declarations.  No kernel runs."""

import re
from pathlib import Path

import pytest
import torch
from torch import nn

from modeling_utils.losses import HuberLoss, L1Loss, MSELoss, SmoothL1Loss, TorchLossConfig, hip_loss_for

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("tribe_elem_loss_workspace_bytes", "tribe_elem_loss_fwd", "tribe_elem_loss_bwd")


@pytest.mark.parametrize("stock, want, attrs", [
    (nn.MSELoss(), MSELoss, {"reduction": "mean"}),
    (nn.MSELoss(reduction="sum"), MSELoss, {"reduction": "sum"}),
    (nn.L1Loss(reduction="sum"), L1Loss, {"reduction": "sum"}),
    (nn.L1Loss(), L1Loss, {"reduction": "mean"}),
    (nn.SmoothL1Loss(beta=0.05), SmoothL1Loss, {"reduction": "mean", "beta": 0.05}),
    (nn.SmoothL1Loss(reduction="sum", beta=0.0), SmoothL1Loss, {"reduction": "sum", "beta": 0.0}),
    (nn.HuberLoss(delta=0.3), HuberLoss, {"reduction": "mean", "delta": 0.3}),
    (nn.HuberLoss(reduction="sum"), HuberLoss, {"reduction": "sum", "delta": 1.0}),
])
def test_hip_loss_for_maps_stock_modules(stock, want, attrs):
    hip = hip_loss_for(stock)
    assert type(hip) is want and not type(hip).__module__.startswith("torch.")
    assert callable(hip.forward_bvt)
    for name, value in attrs.items():
        assert getattr(hip, name) == value


def test_hip_loss_for_declines_everything_else():
    class MyHuber(nn.HuberLoss):
        pass

    for module in (nn.HuberLoss(reduction="none"), nn.L1Loss(reduction="none"), MyHuber(), nn.CrossEntropyLoss(), nn.PoissonNLLLoss(),
                   HuberLoss(), MSELoss(), nn.Identity()):
        assert hip_loss_for(module) is None, type(module)
    # torch constructs these and reports the bad value at the first call; so does the step, through the stock module
    assert hip_loss_for(nn.HuberLoss(delta=0.0)) is None
    assert hip_loss_for(nn.SmoothL1Loss(beta=-1.0)) is None


def test_defaults_and_argument_names_follow_torch():
    assert (L1Loss().reduction, SmoothL1Loss().beta, HuberLoss().delta) == ("mean", 1.0, 1.0)
    assert SmoothL1Loss("sum", 0.5).beta == 0.5 and HuberLoss("sum", 2.0).delta == 2.0
    assert SmoothL1Loss(beta=0.0).beta == 0.0            # torch accepts beta == 0 (L1)
    assert MSELoss(reduction="sum").reduction == "sum"
    assert MSELoss().reduction == "mean"


def test_constructors_refuse_what_torch_refuses_at_call_time():
    x, y = torch.zeros(3), torch.ones(3)
    with pytest.raises(RuntimeError) as torch_huber:
        nn.functional.huber_loss(x, y, delta=0.0)
    with pytest.raises(ValueError) as ours:
        HuberLoss(delta=0.0)
    assert str(ours.value) == str(torch_huber.value).splitlines()[0]
    with pytest.raises(ValueError):
        HuberLoss(delta=-1.0)
    with pytest.raises(RuntimeError) as torch_smooth:
        nn.functional.smooth_l1_loss(x, y, beta=-1.0)
    with pytest.raises(ValueError) as ours:
        SmoothL1Loss(beta=-1.0)
    assert str(ours.value) == str(torch_smooth.value).splitlines()[0]
    for cls in (L1Loss, SmoothL1Loss, HuberLoss, MSELoss):
        with pytest.raises(NotImplementedError):
            cls(reduction="none")
        with pytest.raises(ValueError):
            cls(reduction="median")


@pytest.mark.parametrize("loss", [L1Loss(), SmoothL1Loss(), HuberLoss(), MSELoss(), MSELoss(reduction="sum")])
def test_no_cpu_fallback(loss):
    from tribe_hip._lib import TribeHipError

    x, y = torch.randn(6, 5), torch.randn(6, 5)
    with pytest.raises(TribeHipError):
        loss(x, y)
    with pytest.raises(TribeHipError):
        loss.forward_bvt(x.view(2, 5, 3).requires_grad_(), y.view(2, 5, 3))


def test_ops_elem_loss_checks_arguments_before_any_launch():
    from tribe_hip import ops
    from tribe_hip._lib import TribeHipError

    with pytest.raises(TribeHipError):
        ops.elem_loss(torch.zeros(4), torch.zeros(4), "huber")
    assert set(ops.ELEM_LOSS_KINDS) == {"l1", "smooth_l1", "huber", "mse"} and set(ops.ELEM_LOSS_REDUCTIONS) == {"mean", "sum"}


def test_step_routes_stock_losses_without_replacing_them():
    from algonauts2025.pl_module import BrainModule

    stock = TorchLossConfig(name="HuberLoss", kwargs={"delta": 0.5}).build()
    assert type(stock) is nn.HuberLoss
    bm = BrainModule(nn.Identity(), stock, None, {})
    hip = bm._hip_loss()
    assert type(hip) is HuberLoss and hip.delta == 0.5
    assert bm.loss is stock and bm._hip_loss() is hip            # resolved once
    assert not any(isinstance(m, HuberLoss) for m in bm.modules())
    stock.delta = 0.25                                           # a changed hyper-parameter is seen
    assert bm._hip_loss().delta == 0.25
    stock.reduction = "none"
    assert bm._hip_loss() is None
    bm.loss = nn.SmoothL1Loss(beta=0.1)                          # and so is a replaced loss
    assert type(bm._hip_loss()) is SmoothL1Loss and bm._hip_loss().beta == 0.1
    bm.loss = nn.CrossEntropyLoss()
    assert bm._hip_loss() is None
    # on the CPU the stock module keeps running as it is (the HIP path takes GPU predictions only)
    bm.loss = nn.HuberLoss()
    p, t = torch.randn(2, 5, 3), torch.randn(2, 5, 3)
    torch.testing.assert_close(bm._primary_loss(p, t), nn.functional.huber_loss(p, t))


def test_abi_declares_the_family():
    from tribe_hip import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    # the enum values the binding passes are the header's
    for c_name, value in (("TRIBE_LOSS_L1", 0), ("TRIBE_LOSS_SMOOTH_L1", 1), ("TRIBE_LOSS_HUBER", 2), ("TRIBE_LOSS_MSE", 3),
                          ("TRIBE_REDUCE_MEAN", 0), ("TRIBE_REDUCE_SUM", 1)):
        assert re.search(rf"\b{c_name}\s*=\s*{value}\b", header), c_name
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header)


@pytest.mark.parametrize("args, message", [
    ((0, 1.0, 0), "empty input"),
    ((7, 1.0, 0), "unknown loss kind"),
    ((2, 1.0, 2), "unknown reduction"),
    ((2, 0.0, 0), "non-positive values for delta"),
    ((2, float("inf"), 1), "finite"),
    ((1, -0.5, 0), "negative values for beta"),
    ((1, float("nan"), 0), "finite"),
])
def test_entry_points_refuse_bad_arguments_before_any_launch(args, message):
    """The checks run on the host before the first launch, so placeholder addresses are never read.  n = 0 for the first case."""
    from tribe_hip._lib import check, lib

    kind, param, reduction = args
    n = 0 if message == "empty input" else 8
    with pytest.raises(ValueError, match=message):
        check(lib().tribe_elem_loss_fwd(16, 16, n, kind, param, reduction, 16, 16, 1 << 20, None), "tribe_elem_loss_fwd")
    with pytest.raises(ValueError, match=message):
        check(lib().tribe_elem_loss_bwd(16, 16, n, kind, param, reduction, 16, 16, None), "tribe_elem_loss_bwd")


def test_entry_points_refuse_null_and_small_workspace():
    from tribe_hip._lib import check, lib

    with pytest.raises(ValueError, match="null pointer"):
        check(lib().tribe_elem_loss_fwd(None, 16, 8, 0, 0.0, 0, 16, 16, 1 << 20, None), "tribe_elem_loss_fwd")
    with pytest.raises(ValueError, match="null pointer"):
        check(lib().tribe_elem_loss_bwd(16, 16, 8, 0, 0.0, 0, None, 16, None), "tribe_elem_loss_bwd")
    need = lib().tribe_elem_loss_workspace_bytes(8)
    assert need == 2048 * 8
    with pytest.raises(ValueError, match="workspace too small"):
        check(lib().tribe_elem_loss_fwd(16, 16, 8, 0, 0.0, 0, 16, 16, need - 1, None), "tribe_elem_loss_fwd")
