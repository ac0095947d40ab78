"""CPU (no GPU): MlpConfig.build with hidden sizes -- module layout, state_dict keys, the stock forward -- and
FmriEncoderConfig.projector_hidden_sizes.

The layout is torchvision.ops.MLP's, restated from its source (per hidden size Linear, norm, activation, Dropout; then the last
Linear and a Dropout).  torchvision is not installed where these tests run, so the key lists below are literals: parity with
torchvision itself is unpinned.
"""

import ctypes
import itertools
import re
from pathlib import Path

import pytest
import torch
from torch import nn

from modeling_utils.models.common import Mlp, MlpConfig

ROOT = Path(__file__).resolve().parents[1]
NORMS = {"layer": nn.LayerNorm, None: None}
ACTS = {"gelu": nn.GELU, "relu": nn.ReLU, "elu": nn.ELU, None: nn.Identity}
GRID = list(itertools.product(["layer", None], ["gelu", "relu", "elu", None], [True, False]))


def _config(norm, act, bias=True, **kw):
    return MlpConfig(hidden_sizes=[130, 65], norm_layer=norm, activation_layer=act, bias=bias, **kw)


@pytest.mark.parametrize("norm,act,bias", GRID)
def test_layout_and_state_dict(norm, act, bias):
    mlp = _config(norm, act, bias).build(70, 33)
    assert isinstance(mlp, Mlp) and isinstance(mlp, nn.Sequential)
    block = [nn.Linear] + ([nn.LayerNorm] if norm else []) + [ACTS[act], nn.Dropout]
    assert [type(m) for m in mlp] == block * 2 + [nn.Linear, nn.Dropout]
    if norm:
        want = {"0.weight": (130, 70), "0.bias": (130,), "1.weight": (130,), "1.bias": (130,), "4.weight": (65, 130), "4.bias": (65,),
                "5.weight": (65,), "5.bias": (65,), "8.weight": (33, 65), "8.bias": (33,)}
        linear_bias = ["0.bias", "4.bias", "8.bias"]
    else:
        want = {"0.weight": (130, 70), "0.bias": (130,), "3.weight": (65, 130), "3.bias": (65,), "6.weight": (33, 65), "6.bias": (33,)}
        linear_bias = ["0.bias", "3.bias", "6.bias"]
    if not bias:
        want = {k: v for k, v in want.items() if k not in linear_bias}
    got = mlp.state_dict()
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == want
    # stock defaults: LayerNorm eps 1e-5 with affine, exact GELU, ELU alpha 1, Dropout(0)
    for m in mlp:
        if isinstance(m, nn.LayerNorm):
            assert m.eps == 1e-5 and m.elementwise_affine
        if isinstance(m, nn.GELU):
            assert m.approximate == "none"
        if isinstance(m, nn.ELU):
            assert m.alpha == 1.0
        if isinstance(m, nn.Dropout):
            assert m.p == 0.0


@pytest.mark.parametrize("norm,act,bias", GRID)
def test_cpu_forward_is_the_stock_modules(norm, act, bias):
    torch.manual_seed(3)
    mlp = _config(norm, act, bias).build(70, 33)
    layers, width = [], 70
    for h in (130, 65):
        layers.append(nn.Linear(width, h, bias=bias))
        if norm:
            layers.append(nn.LayerNorm(h))
        layers += [ACTS[act](), nn.Dropout(0.0)]
        width = h
    layers += [nn.Linear(width, 33, bias=bias), nn.Dropout(0.0)]
    hand = nn.Sequential(*layers)
    with torch.no_grad():
        for p in mlp.parameters():
            p.normal_(0.0, 0.3)
    hand.load_state_dict(mlp.state_dict())
    x = torch.randn(4, 9, 70)
    assert torch.equal(mlp(x), hand(x))
    assert (mlp.stock_calls, mlp.hip_calls) == (1, 0)


def test_build_without_output_size_ends_at_the_last_hidden_size():
    mlp = _config("layer", "gelu").build(70)
    assert [tuple(m.weight.shape) for m in mlp if isinstance(m, nn.Linear)] == [(130, 70), (65, 130)]
    assert mlp(torch.randn(3, 70)).shape == (3, 65)


def test_build_does_not_mutate_the_config():
    cfg = _config("layer", "gelu")
    a, b = cfg.build(70, 33), cfg.build(70, 33)
    assert cfg.hidden_sizes == [130, 65]
    assert list(a.state_dict()) == list(b.state_dict())


def test_unit_norm_is_a_value_error():
    with pytest.raises(ValueError):
        _config("unit", "gelu").build(70, 33)


@pytest.mark.parametrize("norm,act", [("batch", "relu"), ("layer", "prelu"), ("batch", "prelu")])
def test_stock_only_modules_build_and_run(norm, act):
    mlp = _config(norm, act).build(70, 33)
    assert not mlp.hip_supported()
    assert mlp(torch.randn(6, 70)).shape == (6, 33)
    assert any(isinstance(m, nn.BatchNorm1d if norm == "batch" else nn.PReLU) for m in mlp)


def test_empty_hidden_sizes_is_a_bare_linear():
    for hidden in (None, []):
        lin = MlpConfig(hidden_sizes=hidden, norm_layer="layer", activation_layer="gelu").build(70, 33)
        assert type(lin) is nn.Linear and tuple(lin.weight.shape) == (33, 70)


FDIMS = {"text": (2, 96), "audio": (2, 80), "video": (1, 72)}


def _model(**kw):
    from algonauts2025.model import FmriEncoderConfig

    return FmriEncoderConfig(hidden=768, depth=2, heads=2, n_subjects=4, contrastive_enabled=True, **kw).build(FDIMS, 50, 10)


def test_model_with_projector_hidden_sizes():
    model = _model(projector_hidden_sizes=[160, 100])
    keys = list(model.state_dict())
    per_mlp = ["0.weight", "0.bias", "1.weight", "1.bias", "4.weight", "4.bias", "5.weight", "5.bias", "8.weight", "8.bias"]
    for prefix in ("projectors.text.", "projectors.audio.", "projectors.video.", "contrastive_heads.video."):
        assert [k[len(prefix):] for k in keys if k.startswith(prefix)] == per_mlp
    sd = model.state_dict()
    assert tuple(sd["projectors.text.0.weight"].shape) == (160, 192) and tuple(sd["projectors.text.4.weight"].shape) == (100, 160)
    assert tuple(sd["projectors.text.8.weight"].shape) == (256, 100) and tuple(sd["contrastive_heads.video.8.weight"].shape) == (768, 100)
    assert all(isinstance(m, Mlp) for m in model.projectors.values())


def test_model_default_is_unchanged():
    from algonauts2025.model import FmriEncoderConfig

    assert FmriEncoderConfig().projector_hidden_sizes is None
    with_none, without = _model(projector_hidden_sizes=None), _model()
    assert list(with_none.state_dict()) == list(without.state_dict())
    assert all(type(m) is nn.Linear for m in with_none.projectors.values())
    assert "projectors.text.weight" in with_none.state_dict()


def test_library_exports_the_new_symbols():
    from tribe_hip import _lib

    names = ["tribe_norm_act_fwd", "tribe_norm_act_bwd", "tribe_norm_act_bwd_workspace_bytes", "tribe_norm_act_path"]
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in names:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert re.search(r"TRIBE_ACT_RELU\s*=\s*8\b", header) and re.search(r"TRIBE_ACT_ELU\s*=\s*9\b", header)
    assert (_lib.ACT_RELU, _lib.ACT_ELU) == (8, 9) and _lib.ABI_VERSION == 5
    # 64 rows per partial, two f64 sums per column
    handle.tribe_norm_act_bwd_workspace_bytes.restype = ctypes.c_size_t
    handle.tribe_norm_act_bwd_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    assert handle.tribe_norm_act_bwd_workspace_bytes(65, 10) == 2 * 2 * 10 * 8
