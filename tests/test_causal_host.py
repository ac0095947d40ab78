"""CPU (no GPU): the host surface of causal encoders -- the config switches (TransformerEncoderConfig.causal, FmriEncoderConfig.causal), the
three new C entry points with their ctypes signatures and argument errors, the unchanged ABI version, and the restated causal oracle
(tests/causal_restatement.py), which must itself be causal."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests.causal_restatement import CausalAttention, make_causal, tril_mask

ROOT = Path(__file__).resolve().parents[1]
SITE = 4 << 56

STILL_UNSUPPORTED = [dict(cross_attend=True), dict(use_rmsnorm=True), dict(rel_pos_bias=True), dict(alibi_pos_bias=True), dict(rotary_xpos=True),
                     dict(residual_attn=True), dict(use_scalenorm=False)]


# ---- config surface -------------------------------------------------------------------------------------------------------------------
def test_encoder_config_builds_a_causal_hip_encoder():
    from modeling_utils.models.transformer import HipEncoder, TransformerEncoderConfig

    plain = TransformerEncoderConfig(depth=2, heads=2).build(768)
    causal = TransformerEncoderConfig(depth=2, heads=2, causal=True).build(768)
    assert isinstance(causal, HipEncoder) and causal.causal is True and plain.causal is False
    assert list(causal.state_dict().keys()) == list(plain.state_dict().keys())
    assert [tuple(v.shape) for v in causal.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert HipEncoder(dim=256, depth=1, heads=4, dim_head=64).causal is False      # off by default


@pytest.mark.parametrize("switch", STILL_UNSUPPORTED, ids=lambda d: next(iter(d)))
def test_the_other_seven_switches_still_raise(switch):
    from modeling_utils.models.transformer import TransformerEncoderConfig

    for causal in (False, True):
        with pytest.raises(NotImplementedError) as err:
            TransformerEncoderConfig(depth=1, heads=4, causal=causal, **switch).build(256)
        assert "causal" not in str(err.value)                                       # names the offending switch, never `causal`
        assert next(iter(switch)).replace("use_scalenorm", "not use_scalenorm") in str(err.value)


def test_model_config_field_validates_and_builds():
    from algonauts2025.model import FmriEncoderConfig

    assert FmriEncoderConfig().causal is False
    assert FmriEncoderConfig(causal=True).causal is True
    fdims = {"text": (1, 24), "audio": (1, 16), "video": None}
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, causal=True, attn_dropout=0.1).build(fdims, 12, 5)
    assert model.encoder.causal is True and model.encoder.attn_dropout == 0.1
    plain = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4).build(fdims, 12, 5)
    assert plain.encoder.causal is False and list(plain.state_dict().keys()) == list(model.state_dict().keys())


def test_pack_carries_the_flag():
    from tribe_hip import ops

    assert ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12).causal is False
    assert ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12, causal=True).causal is True


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_new_entry_points():
    from tribe_hip import _lib

    C = ctypes
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    mask = [i64, C.c_uint32, f32, C.c_uint64, C.c_uint64, vp]                      # row0, threshold, scale_keep, seed, site, stream
    want = {
        "tribe_softmax_causal_fwd": [vp, vp, vp] + [i64] * 5 + mask,
        "tribe_softmax_causal_bwd": [vp] * 5 + [i64] * 7 + [f32] + mask,
        "tribe_encoder_fwd_ex": [C.POINTER(_lib.EncoderDesc), C.c_uint32, vp, vp, i32, vp, sz, vp],
    }
    text = (ROOT / "include" / "tribe_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, argtypes in want.items():
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert hasattr(handle, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
        declared = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(declared.split(",")) == len(argtypes)
    assert re.search(r"#define TRIBE_ENCODER_CAUSAL 1u\b", header) and _lib.ENCODER_CAUSAL == 1
    # additive: the version and the existing entry points' signatures stand
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5
    assert _lib.SIGNATURES["tribe_encoder_fwd"] == (C.c_int, [C.POINTER(_lib.EncoderDesc), vp, vp, i32, vp, sz, vp])
    assert _lib.SIGNATURES["tribe_softmax_causal_fwd"] == _lib.SIGNATURES["tribe_softmax_dropout_fwd"]
    assert _lib.SIGNATURES["tribe_softmax_causal_bwd"] == _lib.SIGNATURES["tribe_softmax_dropout_bwd"]


def test_row_kernel_argument_errors_need_no_gpu():
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
        assert lib.tribe_softmax_causal_fwd(*args.values()) < 0, change
        assert b"tribe_softmax_causal_fwd" in lib.tribe_last_error()
    ok = dict(P=a, dPd=b, negD=c, dS=d, Pd=a, rows=2, T=6, T_pad=8, ld_p=8, ld_dp=6, ld_ds=8, ld_pd=8, scale=0.125, row0=0,
              threshold=1 << 31, scale_keep=2.0, seed=1, site=SITE, stream=None)
    for change in [dict(P=None), dict(dPd=None), dict(negD=None), dict(dS=None), dict(Pd=None), dict(rows=0), dict(T=0), dict(T_pad=5),
                   dict(ld_p=7), dict(ld_dp=5), dict(ld_ds=7), dict(ld_pd=7), dict(row0=-1), dict(dS=a), dict(Pd=d),
                   dict(ld_p=16)] + bad_keep:                                       # (in place with two different pitches)
        args = {**ok, **change}
        assert lib.tribe_softmax_causal_bwd(*args.values()) < 0, change
        assert b"tribe_softmax_causal_bwd" in lib.tribe_last_error()


def test_encoder_fwd_ex_rejects_unknown_flag_bits_before_anything_else():
    from tribe_hip import _lib

    lib = _lib.lib()
    for flags in (2, 3, 1 << 31):
        assert lib.tribe_encoder_fwd_ex(None, flags, None, None, _lib.F32, None, 0, None) < 0
        assert b"tribe_encoder_fwd_ex" in lib.tribe_last_error() and b"flag" in lib.tribe_last_error()
    for flags in (0, 1):                                                            # known bits: the shared body's own validation answers
        assert lib.tribe_encoder_fwd_ex(None, flags, None, None, _lib.F32, None, 0, None) < 0
        assert b"null descriptor" in lib.tribe_last_error()


# ---- the restated oracle --------------------------------------------------------------------------------------------------------------
def test_tril_mask_follows_the_query_index():
    m = tril_mask(7, 5, row0=3)                                                     # queries 3, 4, 0, 1, 2, 3, 4
    assert m.sum(1).tolist() == [4, 5, 1, 2, 3, 4, 5] and bool(m[:, 0].all())
    assert torch.equal(tril_mask(5, 5), torch.ones(5, 5).tril().bool())


@pytest.mark.parametrize("rotary", [True, False])
def test_restated_causal_oracle_is_causal(rotary):
    """float64: replacing the inputs at positions > t leaves the outputs at positions <= t exactly equal, and moves the later ones; the
    unmasked oracle on the same inputs does change at positions <= t."""
    from oracle import xt_encoder

    torch.manual_seed(0)
    enc = xt_encoder.Encoder(dim=256, depth=2, heads=4, attn_dim_head=64, rotary_pos_emb=rotary).double().eval()
    keys = list(enc.state_dict().keys())
    B, T, t = 2, 23, 9
    x = torch.randn(B, T, 256, dtype=torch.float64)
    y = x.clone()
    y[:, t + 1:] = torch.randn(B, T - t - 1, 256, dtype=torch.float64)
    with torch.no_grad():
        plain_x, plain_y = enc(x), enc(y)
        assert not torch.equal(plain_x[:, : t + 1], plain_y[:, : t + 1])
        make_causal(enc)
        assert all(isinstance(layer[1], CausalAttention) for layer in enc.layers[0::2]) and list(enc.state_dict().keys()) == keys
        out_x, out_y = enc(x), enc(y)
    assert torch.equal(out_x[:, : t + 1], out_y[:, : t + 1])
    assert not torch.equal(out_x[:, t + 1:], out_y[:, t + 1:])
    assert not torch.equal(out_x, plain_x)
