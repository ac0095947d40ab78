"""CPU (no GPU): attention dropout's host surface -- the two C symbols and their argument errors, the config fields (FmriEncoderConfig /
TransformerEncoderConfig attn_dropout), the site constant, and the restated mask (tests/dropout_restatement.py) on the logical
[B * heads * T, T] tensors the GPU tests use."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests.dropout_restatement import keep_mask

ROOT = Path(__file__).resolve().parents[1]
SEED = 0x5EED0123456789AB
SITE = 4 << 56


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_symbols():
    from tribe_hip import _lib

    C = ctypes
    vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float
    mask = [i64, C.c_uint32, f32, C.c_uint64, C.c_uint64, vp]                      # row0, threshold, scale_keep, seed, site, stream
    want = {
        "tribe_softmax_dropout_fwd": [vp, vp, vp] + [i64] * 5 + mask,              # S, Pd, lse; rows, T, T_pad, ld_s, ld_p
        "tribe_softmax_dropout_bwd": [vp] * 5 + [i64] * 7 + [f32] + mask,          # P, dPd, negD, dS, Pd; rows, T, T_pad, 4 pitches; scale
    }
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, argtypes in want.items():
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert hasattr(handle, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
        declared = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(declared.split(",")) == len(argtypes)
    fn = _lib.lib().tribe_softmax_dropout_fwd
    assert fn.restype is C.c_int and list(fn.argtypes) == want["tribe_softmax_dropout_fwd"]


def test_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    a, b, c, d = p, p + 4096, p + 8192, p + 12288
    bad_keep = [dict(scale_keep=float("nan")), dict(scale_keep=float("inf")), dict(scale_keep=0.5), dict(scale_keep=-2.0)]
    ok = dict(S=a, Pd=b, lse=c, rows=2, T=6, T_pad=8, ld_s=6, ld_p=8, row0=0, threshold=1 << 31, scale_keep=2.0, seed=1, site=SITE, stream=None)
    for change in [dict(S=None), dict(Pd=None), dict(lse=None), dict(rows=0), dict(rows=-1), dict(T=0), dict(T=-3), dict(T_pad=5),
                   dict(ld_s=5), dict(ld_p=7), dict(row0=-1)] + bad_keep:
        args = {**ok, **change}
        assert lib.tribe_softmax_dropout_fwd(*args.values()) < 0, change
        assert b"tribe_softmax_dropout_fwd" in lib.tribe_last_error()
    ok = dict(P=a, dPd=b, negD=c, dS=d, Pd=a, rows=2, T=6, T_pad=8, ld_p=8, ld_dp=6, ld_ds=8, ld_pd=8, scale=0.125, row0=0,
              threshold=1 << 31, scale_keep=2.0, seed=1, site=SITE, stream=None)
    for change in [dict(P=None), dict(dPd=None), dict(negD=None), dict(dS=None), dict(Pd=None), dict(rows=0), dict(T=0), dict(T_pad=5),
                   dict(ld_p=7), dict(ld_dp=5), dict(ld_ds=7), dict(ld_pd=7), dict(row0=-1), dict(dS=a), dict(Pd=d),
                   dict(ld_p=16)] + bad_keep:                                       # (in place with two different pitches)
        args = {**ok, **change}
        assert lib.tribe_softmax_dropout_bwd(*args.values()) < 0, change
        assert b"tribe_softmax_dropout_bwd" in lib.tribe_last_error()


# ---- config surface -------------------------------------------------------------------------------------------------------------------
def test_model_config_field():
    from algonauts2025.model import SITE_ATTN, SITE_FF, SITE_HEAD, SITE_PROJECTOR, FmriEncoderConfig

    assert (SITE_FF, SITE_PROJECTOR, SITE_HEAD, SITE_ATTN) == (1, 2, 3, 4) and SITE_ATTN << 56 == SITE
    assert FmriEncoderConfig().attn_dropout == 0.0
    assert FmriEncoderConfig(attn_dropout=0.25).attn_dropout == 0.25
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            FmriEncoderConfig(attn_dropout=bad)
    fdims = {"text": (1, 24), "audio": (1, 16), "video": None}
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, attn_dropout=0.2).build(fdims, 12, 5)
    assert model.encoder.attn_dropout == 0.2 and (model.encoder.ff_dropout, model.encoder.layer_dropout) == (0.0, 0.0)
    assert model.last_dropout_key is None
    assert FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4).build(fdims, 12, 5).encoder.attn_dropout == 0.0


def test_encoder_config_validates_and_stores_attn_dropout():
    from modeling_utils.models.transformer import TransformerEncoderConfig

    assert TransformerEncoderConfig().attn_dropout == 0.1                           # the reference config's default
    assert TransformerEncoderConfig(depth=1, heads=4).build(dim=256).attn_dropout == 0.1
    assert TransformerEncoderConfig(depth=1, heads=4, attn_dropout=0.0).build(dim=256).attn_dropout == 0.0
    for bad in (1.0, -0.1, 2.0):
        with pytest.raises(ValueError):
            TransformerEncoderConfig(depth=1, heads=4, attn_dropout=bad).build(dim=256)


def test_no_source_calls_attn_dropout_inert():
    for path in [ROOT / "README.md", ROOT / "DESIGN.md", *(ROOT / "algonauts-2025_amd").rglob("*.py")]:
        for line in path.read_text().splitlines():
            assert not ("attn_dropout" in line and "inert" in line), f"{path.name}: {line.strip()}"


# ---- the restated mask on the attention shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,p", [(280, 70, 0.2), (576, 192, 0.1), (33, 33, 0.5), (1192, 298, 0.1)])
def test_restated_mask_keep_fraction_and_no_empty_row(rows, T, p):
    keep = keep_mask(rows, T, p, SEED, SITE | 1)
    n = keep.size
    sigma = (float(keep.sum()) - n * (1 - p)) / (n * p * (1 - p)) ** 0.5
    print(f"[{rows}, {T}] p={p}: keep fraction {keep.mean():.4f}, {sigma:+.2f} sigma from 1 - p")
    assert abs(sigma) < 3
    assert keep.any(axis=1).all()                                                   # no query row loses every key


def test_mask_rows_do_not_depend_on_the_slab():
    """idx = (row0 + r) * T + j: rows 13.. of the whole mask are the rows a slab starting at row0 = 13 must draw (T % 4 != 0)."""
    from tests.dropout_restatement import words

    whole = words(40, 70, SEED, SITE)
    flat = words(1, 40 * 70, SEED, SITE).reshape(-1)
    assert (whole[13:] == flat[13 * 70:].reshape(27, 70)).all()
    assert np.array_equal(keep_mask(40, 70, 0.2, SEED, SITE)[13:], flat[13 * 70:].reshape(27, 70) >= np.uint32(int(0.2 * 4294967296.0)))
