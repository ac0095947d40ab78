"""CPU (no GPU): the dropout definition restated in numpy (tests/dropout_restatement.py) pinned to known answers, the config surface
(ff_dropout, layer_dropout, projector_dropout, MlpConfig.dropout_backend), the two C symbols and their argument errors."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.dropout_restatement import keep_mask, philox4x32_10, scale, threshold

ROOT = Path(__file__).resolve().parents[1]
SEED, SITE = 0x0123456789ABCDEF, 7


def _words(text: str) -> np.ndarray:
    return np.array([int(w, 16) for w in text.split()], dtype=np.uint32)


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert (philox4x32_10(_words(counter), _words(key)) == _words(want)).all()


def test_threshold_and_scale():
    assert threshold(0.5) == 1 << 31 and threshold(0.0) == 0 and threshold(0.1) == 429496729 and threshold(0.15) == 644245094
    assert scale(0.5) == np.float32(2.0) and scale(0.1) == np.float32(1.0 / 0.9) and scale(0.1).dtype == np.float32


def test_small_mask_known_answer():
    want = np.array([[0, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 0, 0, 1, 1]], dtype=bool)
    assert (keep_mask(3, 5, 0.5, SEED, SITE) == want).all()


@pytest.mark.parametrize("p, kept", [(0.1, 948355), (0.15, 895656), (0.5, 526904)])
def test_keep_counts_known_answers(p, kept):
    n = 257 * 4100
    got = int(keep_mask(257, 4100, p, SEED, SITE).sum())
    assert got == kept
    assert abs(got - n * (1 - p)) < 0.11 * (n * p * (1 - p)) ** 0.5


@pytest.mark.parametrize("seed, site", [(SEED, 8), (SEED - 1, SITE)])
def test_other_site_or_seed_gives_an_independent_mask(seed, site):
    a, b = keep_mask(257, 4100, 0.5, SEED, SITE), keep_mask(257, 4100, 0.5, seed, site)
    n = a.size
    sigma = abs(float((a == b).sum()) - n / 2) / (n / 4) ** 0.5
    print(f"seed {seed:#x} site {site}: agreement {sigma:.2f} sigma from one half")
    assert sigma < 5


def test_mask_is_indexed_by_dim_not_by_rows():
    """idx = r * dim + c: a [6, 10] mask read row-major is the [3, 20] mask read row-major."""
    assert (keep_mask(6, 10, 0.15, SEED, SITE).reshape(-1) == keep_mask(3, 20, 0.15, SEED, SITE).reshape(-1)).all()


# ---- config surface -------------------------------------------------------------------------------------------------------------------
def test_encoder_config_builds_with_dropout():
    from modeling_utils.models.transformer import TransformerEncoderConfig

    enc = TransformerEncoderConfig(depth=2, heads=4, ff_dropout=0.2, layer_dropout=0.5).build(dim=256)
    assert (enc.ff_dropout, enc.layer_dropout) == (0.2, 0.5)
    assert all(enc.layers[2 * i + 1][1].ff[1].p == 0.2 for i in range(2))
    assert TransformerEncoderConfig(depth=1, heads=4, layer_dropout=1.0).build(dim=256).layer_dropout == 1.0
    plain = TransformerEncoderConfig(depth=1, heads=4).build(dim=256)
    assert (plain.ff_dropout, plain.layer_dropout, plain.layers[1][1].ff[1].p) == (0.0, 0.0, 0.0)
    for bad in (dict(ff_dropout=1.0), dict(ff_dropout=-0.1), dict(layer_dropout=1.5), dict(layer_dropout=-0.1)):
        with pytest.raises(ValueError):
            TransformerEncoderConfig(depth=1, heads=4, **bad).build(dim=256)


def test_model_config_fields():
    from algonauts2025.model import FmriEncoderConfig
    from modeling_utils.models.common import Mlp

    cfg = FmriEncoderConfig()
    assert (cfg.ff_dropout, cfg.layer_dropout, cfg.projector_dropout) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        FmriEncoderConfig(projector_dropout=0.1)                       # no hidden sizes: the single Linear has no dropout
    for bad in (dict(ff_dropout=1.0), dict(layer_dropout=1.01), dict(projector_dropout=1.0, projector_hidden_sizes=[32]),
                dict(ff_dropout=-0.5)):
        with pytest.raises(ValueError):
            FmriEncoderConfig(**bad)
    fdims = {"text": (1, 24), "audio": (1, 16), "video": None}
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, ff_dropout=0.2, layer_dropout=0.5, projector_dropout=0.1,
                              projector_hidden_sizes=[40], contrastive_enabled=True, contrastive_modalities=["audio"]).build(fdims, 12, 5)
    assert (model.encoder.ff_dropout, model.encoder.layer_dropout) == (0.2, 0.5)
    mlps = [model.projectors["text"], model.projectors["audio"], model.contrastive_heads["audio"]]
    assert all(isinstance(m, Mlp) and m.dropout == 0.1 and m.dropout_backend == "hip" for m in mlps)
    assert [m.dropout_site for m in mlps] == [(2 << 56) | (0 << 16), (2 << 56) | (1 << 16), (3 << 56) | (1 << 16)]
    assert model.last_dropout_key is None and model.last_layer_drops is None
    plain = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, projector_hidden_sizes=[40]).build(fdims, 12, 5)
    assert all(m.dropout == 0.0 and m.dropout_backend == "torch" for m in plain.projectors.values())


def test_mlp_dropout_backend():
    from modeling_utils.models.common import MlpConfig

    assert MlpConfig().dropout_backend == "torch"
    stock = MlpConfig(hidden_sizes=[8], dropout=0.1).build(4, 2)
    hip = MlpConfig(hidden_sizes=[8], dropout=0.1, dropout_backend="hip").build(4, 2)
    assert stock.dropout_backend == "torch" and not stock.train().hip_supported() and stock.eval().hip_supported()
    assert hip.dropout_backend == "hip" and hip.train().hip_supported() and hip.hip_dropout_active() and not hip.eval().hip_dropout_active()
    assert list(stock.state_dict()) == list(hip.state_dict())
    with pytest.raises(ValueError):
        MlpConfig(dropout_backend="triton")
    with pytest.raises(ValueError):
        MlpConfig(hidden_sizes=[8], dropout=1.0, dropout_backend="hip").build(4, 2)
    hip.train()(torch.randn(5, 4))                                       # CPU tensors: the stock modules, whatever the backend
    assert (hip.hip_calls, hip.stock_calls) == (0, 1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_symbols():
    from tribe_hip import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("tribe_dropout_apply", "tribe_dropout_path"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5 and re.search(r"#define TRIBE_ABI_VERSION 5\b", header)


def test_argument_errors_need_no_gpu():
    from tribe_hip import _lib
    from tribe_hip.ops import dropout_params

    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(x=p, y=p, dtype=_lib.F32, rows=2, dim=8, ld_x=8, ld_y=8, threshold=1 << 31, scale=2.0, seed=1, site=2, stream=None)
    bad = [dict(x=None), dict(y=None), dict(dtype=2), dict(dtype=-1), dict(rows=0), dict(dim=0), dict(ld_x=7), dict(ld_y=7),
           dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=0.5), dict(scale=-2.0)]
    for change in bad:
        args = {**ok, **change}
        assert lib.tribe_dropout_apply(*args.values()) < 0, change
        assert b"tribe_dropout_apply" in lib.tribe_last_error()
    for p_bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dropout_params(p_bad)
    assert dropout_params(0.5) == (1 << 31, np.float32(2.0)) and dropout_params(0.0) == (0, np.float32(1.0))
    assert dropout_params(0.1) == (threshold(0.1), scale(0.1))
    # the branch report is host arithmetic on pointers and pitches
    path = lambda off, dtype, dim, ld: lib.tribe_dropout_path(p + off, p + off, dtype, dim, ld, ld)   # noqa: E731
    base = (16 - p % 16) % 16
    assert path(base, _lib.F32, 8, 8) == 0 and path(base, _lib.BF16, 8, 8) == 0
    assert path(base, _lib.BF16, 12, 12) == 1 and path(base + 8, _lib.BF16, 8, 8) == 1
    assert path(base, _lib.F32, 6, 8) == 2 and path(base + 4, _lib.F32, 8, 8) == 2 and path(base, _lib.F32, 8, 9) == 2
    assert path(base + 2, _lib.BF16, 8, 8) == 2
