"""CPU (no GPU): the host surface of block append on streamed causal encoders -- the four new C entry points (declared in the header, bound
with matching prototypes, the ABI version unchanged), their argument errors, which name the entry point and need no device, the ValueErrors
of ops.attention_extend / kv_append_block / encoder_extend, HipEncoder.extend and EncoderStream.push_block -- and what the GPU grid of
tests/test_gpu_extend_attention.py can detect.

Mask power check.  The GPU test holds tribe_attention_extend_fwd to oracle.attention_ref.forward_bound on the grid of tests/extend_cases.py.
Here, in float64 on the CPU, five wrong masks are compared with the right one (query t of the block sees keys j <= pos + t) on the `diffuse`
inputs of that grid: the offset ignored (j <= t), the whole block visible (j <= pos + k - 1), one key too many, one key too few, and the
block's own cache slots still zero (attention launched before the fill).  Wherever a wrong mask differs from the right one at all, at every
grid point with pos <= 300, its output leaves the bound by a factor >= 3.  (pos, k) = (1000, 24) tests the tile loop, not the mask -- one
key in a thousand moves a diffuse row by 1-3 bounds -- and is left out of this check only; perm2 / perm06 are one-hot at dim_head 384 and
carry no power claim against off-by-one masks.  The clean emulation of the flash kernels (ar.emulate_forward, causal, last k rows) stays
within the bound on the whole grid, all three input kinds."""

import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

from oracle import attention_ref as ar
from tests.extend_cases import BATCH_HEADS, DIM_HEADS, POS_K, problem

ROOT = Path(__file__).resolve().parents[1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_new_entry_points():
    from tribe_hip import _lib

    C = ctypes
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    desc = C.POINTER(_lib.EncoderDesc)
    want = {
        "tribe_kv_append_block": (C.c_int, [vp, i64, i64, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
        "tribe_attention_extend_fwd": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, i64, i64, f32, vp, vp]),
        "tribe_encoder_extend_workspace_bytes": (sz, [desc, i64]),
        "tribe_encoder_extend_fwd": (C.c_int, [desc, vp, vp, i32, vp, vp, i64, i64, vp, sz, vp]),
    }
    text = (ROOT / "include" / "tribe_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, signature in want.items():
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert hasattr(handle, name)
        assert _lib.SIGNATURES[name] == signature
        declared = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(declared.split(",")) == len(signature[1])
    # additive: the version and the streaming entry points of before stand
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5
    assert _lib.SIGNATURES["tribe_kv_append"] == (C.c_int, [vp, i64, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp])
    assert _lib.SIGNATURES["tribe_encoder_step_fwd"] == (C.c_int, [desc, vp, vp, i32, vp, vp, i64, i64, vp, sz, vp])
    assert re.search(r"#define TRIBE_ENCODER_CAUSAL 1u\b", header) and not re.search(r"#define TRIBE_ENCODER_\w+ [2-9]", header)


def _buffer(nbytes=1 << 16):
    buf = (ctypes.c_char * (nbytes + 256))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_kv_append_block_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(qkv=p, B=2, k=3, heads=2, dim_head=64, rot_dim=32, interleaved=1, cos=p + 4096, sin=p + 8192, pos=3, kc=p + 16384, vc=p + 32768,
              cap=8, stream=None)
    for change in [dict(qkv=None), dict(kc=None), dict(vc=None), dict(B=0), dict(heads=0), dict(dim_head=0), dict(dim_head=60), dict(k=0),
                   dict(k=-1), dict(pos=-1), dict(pos=6), dict(k=6), dict(cap=0), dict(rot_dim=72), dict(rot_dim=12), dict(rot_dim=-8),
                   dict(cos=None), dict(sin=None), dict(interleaved=2), dict(qkv=p + 2), dict(kc=p + 16384 + 8)]:
        args = {**ok, **change}
        assert lib.tribe_kv_append_block(*args.values()) < 0, change
        assert b"tribe_kv_append_block" in lib.tribe_last_error(), change


def test_attention_extend_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(q=p, ld_q=384, kc=p + 4096, vc=p + 8192, B=2, heads=2, dim_head=64, cap=16, pos=5, k=4, scale=0.125, out=p + 16384, stream=None)
    for change in [dict(q=None), dict(kc=None), dict(vc=None), dict(out=None), dict(B=0), dict(heads=0), dict(dim_head=96), dict(dim_head=256),
                   dict(dim_head=0), dict(k=0), dict(k=-2), dict(pos=-1), dict(pos=13), dict(k=12), dict(cap=0), dict(ld_q=64), dict(ld_q=130),
                   dict(q=p + 2), dict(kc=p + 4096 + 8), dict(vc=p + 8192 + 8), dict(out=p + 16384 + 4)]:
        args = {**ok, **change}
        assert lib.tribe_attention_extend_fwd(*args.values()) < 0, change
        assert b"tribe_attention_extend_fwd" in lib.tribe_last_error(), change


def _desc(_lib, **kw):
    d = _lib.EncoderDesc()
    d.B, d.T, d.dim, d.depth, d.heads, d.dim_head, d.ff_inner, d.rot_dim, d.rotary_interleaved = 2, 3, 256, 0, 4, 64, 1024, 0, 1
    d.norm_gain_scale, d.norm_eps = 16.0, 1e-12
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_encoder_extend_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    byref = ctypes.byref
    assert lib.tribe_encoder_extend_fwd(None, p, p, _lib.F32, p, p, 8, 0, p, 1 << 16, None) < 0
    assert b"tribe_encoder_extend_fwd" in lib.tribe_last_error() and b"null descriptor" in lib.tribe_last_error()
    d = _desc(_lib, final_norm_g=p)
    ok = dict(d=byref(d), x=p, y=p + 4096, y_dtype=_lib.F32, kc=p + 8192, vc=p + 16384, cap=8, pos=5, ws=p + 32768, ws_bytes=1 << 15, stream=None)
    for change in [dict(x=None), dict(y=None), dict(kc=None), dict(vc=None), dict(ws=None), dict(pos=-1), dict(pos=6), dict(cap=0), dict(cap=7),
                   dict(kc=p + 8192 + 8), dict(ws=p + 32768 + 16), dict(ws_bytes=16)]:
        assert lib.tribe_encoder_extend_fwd(*{**ok, **change}.values()) < 0, change
        assert b"tribe_encoder_extend_fwd" in lib.tribe_last_error(), change
    for bad in (_desc(_lib, final_norm_g=p, T=0), _desc(_lib, final_norm_g=p, T=-1), _desc(_lib, final_norm_g=p, T=4),
                _desc(_lib, final_norm_g=p, dim_head=256), _desc(_lib, final_norm_g=p, dim_head=320)):
        assert lib.tribe_encoder_extend_fwd(*{**ok, "d": byref(bad)}.values()) < 0, (bad.T, bad.dim_head)
        assert b"tribe_encoder_extend_fwd" in lib.tribe_last_error(), (bad.T, bad.dim_head)
    assert lib.tribe_encoder_extend_workspace_bytes(byref(d), 8) > 0 and lib.tribe_encoder_extend_workspace_bytes(None, 8) == 0
    assert lib.tribe_encoder_extend_workspace_bytes(byref(_desc(_lib, T=0)), 8) == 0
    more = _desc(_lib, final_norm_g=p, T=30)
    assert lib.tribe_encoder_extend_workspace_bytes(byref(more), 64) > lib.tribe_encoder_extend_workspace_bytes(byref(d), 64)


# ---- ops: shape and dtype checks come first and begin with the C name ---------------------------------------------------------------------
def test_ops_checks_name_the_entry_point():
    from tribe_hip import ops

    bf, f = torch.bfloat16, torch.float32
    kc = torch.zeros(2, 2, 8, 64, dtype=bf)
    qkv = torch.zeros(6, 384, dtype=bf)                                                 # B = 2, k = 3
    cos = torch.zeros(8, 16)
    what = "tribe_kv_append_block"
    with pytest.raises(ValueError, match=rf"^{what}: positions pos=6 .. pos\+k=9 outside the cache capacity 8"):
        ops.kv_append_block(qkv, kc, kc.clone(), 6, 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: k=0 must be at least 1"):
        ops.kv_append_block(qkv[:0], kc, kc.clone(), 0, 0, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: qkv must be contiguous \[B\*k=6, 384\]"):
        ops.kv_append_block(qkv[:, :256], kc, kc.clone(), 0, 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: qkv must be contiguous \[B\*k=6, 384\]"):
        ops.kv_append_block(qkv[:4], kc, kc.clone(), 0, 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: cos must be a contiguous f32 \[>= pos\+k=7"):
        ops.kv_append_block(qkv, kc, kc.clone(), 4, 3, 32, cos[:6], cos, True)
    with pytest.raises(TypeError, match=rf"^{what}: k_cache must be bfloat16"):
        ops.kv_append_block(qkv, kc.float(), kc, 0, 3, 32, cos, cos, True)
    with pytest.raises(TypeError, match=rf"^{what}: qkv must be torch.bfloat16"):
        ops.kv_append_block(qkv.float(), kc, kc.clone(), 0, 3, 32, cos, cos, True)
    what = "tribe_attention_extend_fwd"
    with pytest.raises(ValueError, match=rf"^{what}: positions pos=6 .. pos\+k=9 outside"):
        ops.attention_extend(qkv, kc, kc.clone(), 6, 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: positions pos=-1 "):
        ops.attention_extend(qkv, kc, kc.clone(), -1, 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: k=0 must be at least 1"):
        ops.attention_extend(qkv, kc, kc.clone(), 0, 0, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: q must be \[B\*k=6, >= 128\]"):
        ops.attention_extend(qkv[:5], kc, kc.clone(), 0, 3, 0.125)
    with pytest.raises(TypeError, match=rf"^{what}: q must be torch.bfloat16"):
        ops.attention_extend(qkv.float(), kc, kc.clone(), 0, 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: dim_head=96"):
        ops.attention_extend(qkv, torch.zeros(2, 2, 8, 96, dtype=bf), torch.zeros(2, 2, 8, 96, dtype=bf), 0, 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: k_cache must be a contiguous \[B, heads, cap, dim_head\]"):
        ops.attention_extend(qkv, kc[0], kc[0], 0, 3, 0.125)
    what = "tribe_encoder_extend_fwd"
    pack = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12, causal=True)
    plain = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12)
    caches = torch.zeros(1, 2, 4, 8, 64, dtype=bf)
    x = torch.zeros(6, 256, dtype=f)
    with pytest.raises(ValueError, match=rf"^{what}: the encoder is bidirectional"):
        ops.encoder_extend(x, plain, caches, caches.clone(), 0, 3)
    with pytest.raises(ValueError, match=rf"^{what}: positions pos=6 .. pos\+k=9 outside"):
        ops.encoder_extend(x, pack, caches, caches.clone(), 6, 3)
    with pytest.raises(ValueError, match=rf"^{what}: x must be contiguous \[B\*k=6, 256\]"):
        ops.encoder_extend(x[:4], pack, caches, caches.clone(), 0, 3)
    with pytest.raises(ValueError, match=rf"^{what}: caches .* do not match"):
        ops.encoder_extend(x, pack, caches[:, :, :2].contiguous(), caches[:, :, :2].contiguous(), 0, 3)


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
def _encoder(causal=True, **kw):
    from modeling_utils.models.transformer import TransformerEncoderConfig

    return TransformerEncoderConfig(depth=2, heads=4, causal=causal, **kw).build(256)


def test_extend_value_errors():
    from modeling_utils.models.transformer import EncoderCache

    enc = _encoder()
    cache = enc.new_cache(2, 8)
    with pytest.raises(ValueError, match="no incremental form"):
        _encoder(causal=False).extend(torch.zeros(2, 3, 256), cache)
    with pytest.raises(ValueError, match=r"HipEncoder.extend: expected \[B, k, dim\]"):
        enc.extend(torch.zeros(2, 256), cache)
    with pytest.raises(ValueError, match=r"HipEncoder.extend: expected \[B, k, dim\]"):
        enc.extend(torch.zeros(2, 1, 3, 256), cache)
    with pytest.raises(ValueError, match="batch size 3 does not match the cache's 2"):
        enc.extend(torch.zeros(3, 4, 256), cache)
    with pytest.raises(ValueError, match="expected last dim 256"):
        enc.extend(torch.zeros(2, 4, 128), cache)
    with pytest.raises(ValueError, match="x is on meta, the cache on cpu"):
        enc.extend(torch.zeros(2, 3, 256, device="meta"), cache)
    with pytest.raises(ValueError, match="k must be at least 1"):
        enc.extend(torch.zeros(2, 0, 256), cache)
    with pytest.raises(ValueError, match="run past max_len=8"):
        enc.extend(torch.zeros(2, 9, 256), cache)
    cache.pos = 6
    with pytest.raises(ValueError, match=r"6 positions filled \+ 3 would run past max_len=8"):
        enc.extend(torch.zeros(2, 3, 256), cache)
    with pytest.raises(ValueError, match="was not made for this encoder"):
        enc.extend(torch.zeros(2, 2, 256), EncoderCache(1, 2, 4, 8, 64, None))
    with pytest.raises(TypeError, match="must be an EncoderCache"):
        enc.extend(torch.zeros(2, 2, 256), None)
    assert cache.pos == 6                                                              # a refused block leaves the cache where it was
    # prefill keeps refusing a cache that holds positions; extend is the route onto one
    with pytest.raises(ValueError, match="already holds 6 positions"):
        enc.prefill(torch.zeros(2, 2, 256), cache)
    assert "nference only" in enc.extend.__doc__


def test_push_block_value_errors():
    from algonauts2025.model import FmriEncoderConfig

    fdims = {"text": (1, 24), "audio": (1, 16)}
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32, causal=True).build(fdims, 12, 5)
    stream = model.stream(2)
    sid = torch.zeros(2, 1, dtype=torch.int64)
    block = {"text": torch.zeros(2, 1, 24, 3), "audio": torch.zeros(2, 16, 3), "subject_id": sid}
    with pytest.raises(ValueError, match="EncoderStream.push_block: text: batch size 3 does not match the stream's 2"):
        stream.push_block({**block, "text": torch.zeros(3, 1, 24, 3)})
    with pytest.raises(ValueError, match=r"EncoderStream.push_block: audio: expected \[B, L, D, T\] or \[B, D, T\]"):
        stream.push_block({**block, "audio": torch.zeros(2, 16)})
    with pytest.raises(ValueError, match="EncoderStream.push_block: modalities disagree on the number of time steps"):
        stream.push_block({**block, "text": torch.zeros(2, 1, 24, 4)})
    with pytest.raises(ValueError, match="is on meta, the stream on cpu"):
        stream.push_block({**block, "audio": torch.zeros(2, 16, 3, device="meta")})
    with pytest.raises(ValueError, match="none of the modalities"):
        stream.push_block({"subject_id": sid})
    with pytest.raises(ValueError, match="run past max_len=32"):
        stream.push_block({"text": torch.zeros(2, 1, 24, 33), "audio": torch.zeros(2, 16, 33), "subject_id": sid})
    stream.cache.pos = 30
    with pytest.raises(ValueError, match=r"EncoderStream.push_block: 30 steps seen \+ 3 would run past max_len=32"):
        stream.push_block(block)
    assert stream.pos == 30
    plain = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32).build(fdims, 12, 5)
    with pytest.raises(ValueError, match="no incremental form"):
        plain.stream(2)


# ---- what the GPU grid can detect ---------------------------------------------------------------------------------------------------------
def _masked_f64(q, k, v, scale, pos, visible):
    """float64 attention of the block's rows under `visible` [k rows, pos + k keys] (True = seen)."""
    bias = torch.zeros(visible.shape, dtype=torch.float64).masked_fill(~visible, -math.inf)
    return ar.attention_f64(q[:, :, pos:], k, v, scale, bias=bias)[0]


def _wrong_masks(pos, k):
    """name -> visible [k, pos + k]; row t of the block is position pos + t.  A row keeps key 0 whatever the fault (no empty row)."""
    Tk = pos + k
    j, t = torch.arange(Tk)[None, :], torch.arange(k)[:, None]
    keep0 = j == 0
    return {
        "offset ignored": (j <= t) | keep0,
        "whole block visible": (j <= pos + k - 1) | keep0,
        "one key too many": (j <= pos + t + 1) | keep0,
        "one key too few": (j <= pos + t - 1) | keep0,
    }


@pytest.mark.parametrize("d", DIM_HEADS)
def test_wrong_masks_leave_the_bound_on_the_gpu_grid(d):
    for pos, k in POS_K:
        if pos > 300:
            continue
        for B, heads in BATCH_HEADS:
            q, kk, v, scale, want, P, bound = problem("diffuse", B, heads, d, pos, k)
            Tk = pos + k
            right = torch.arange(Tk)[None, :] <= pos + torch.arange(k)[:, None]
            assert float(((_masked_f64(q, kk, v, scale, pos, right) - want).abs() / bound).max()) < 1e-6   # the harness states the same problem
            faults = {}
            for name, visible in _wrong_masks(pos, k).items():
                if not torch.equal(visible, right):
                    faults[name] = _masked_f64(q, kk, v, scale, pos, visible)
            kz, vz = kk.clone(), v.clone()
            kz[:, :, pos:], vz[:, :, pos:] = 0.0, 0.0
            faults["block slots still zero"] = _masked_f64(q, kz, vz, scale, pos, right)
            for name, out in faults.items():
                ratio = float(((out - want).abs() / bound).max())
                print(f"d={d} (pos, k)=({pos}, {k}) (B, heads)=({B}, {heads}) {name}: worst |wrong - right| / bound {ratio:.1f}")
                assert ratio >= 3.0, (d, pos, k, B, heads, name, ratio)
    # which faults exist where: every point has the zero-slot fault; the others need pos > 0, k > 1 or a key to drop
    assert set(_wrong_masks(5, 16)) == {"offset ignored", "whole block visible", "one key too many", "one key too few"}


@pytest.mark.parametrize("d", DIM_HEADS)
def test_clean_emulation_stays_within_the_bound(d):
    worst = 0.0
    for pos, k in POS_K:
        for B, heads in BATCH_HEADS:
            for kind in ar.KINDS:
                q, kk, v, scale, want, P, bound = problem(kind, B, heads, d, pos, k)
                got = ar.emulate_forward(q, kk, v, scale, causal=True)[0][:, :, pos:]
                ratio, where = ar.ratio_report(got, want, bound)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (d, pos, k, B, heads, kind, ratio, where)
    print(f"d={d}: worst |emulation - float64| / bound over the grid {worst:.3f}")
