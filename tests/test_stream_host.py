"""CPU (no GPU): the host surface of streamed causal encoders -- the seven new C entry points (declared in the header, bound with matching
prototypes, the ABI version unchanged), their argument errors, which name the entry point and need no device, the ValueErrors of
HipEncoder.new_cache / prefill / step and FmriEncoder.stream / EncoderStream, and the shapes a cache allocates."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_new_entry_points():
    from tribe_hip import _lib

    C = ctypes
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    desc = C.POINTER(_lib.EncoderDesc)
    want = {
        "tribe_kv_append": (C.c_int, [vp, i64, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
        "tribe_attention_decode_splits": (i32, [i64, i32, i64]),
        "tribe_attention_decode_workspace_bytes": (sz, [i64, i32, i32, i64]),
        "tribe_attention_decode_fwd": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, i64, f32, vp, vp, sz, vp]),
        "tribe_encoder_step_workspace_bytes": (sz, [desc, i64]),
        "tribe_encoder_step_fwd": (C.c_int, [desc, vp, vp, i32, vp, vp, i64, i64, vp, sz, vp]),
        "tribe_encoder_prefill_fwd": (C.c_int, [desc, vp, vp, i32, vp, vp, i64, vp, sz, vp]),
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
    # additive: the version, the descriptor and the existing encoder entry points stand
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5
    assert _lib.SIGNATURES["tribe_encoder_fwd"] == (C.c_int, [desc, vp, vp, i32, vp, sz, vp])
    assert _lib.SIGNATURES["tribe_encoder_fwd_ex"] == (C.c_int, [desc, C.c_uint32, vp, vp, i32, vp, sz, vp])
    assert re.search(r"#define TRIBE_ENCODER_CAUSAL 1u\b", header) and not re.search(r"#define TRIBE_ENCODER_\w+ [2-9]", header)


def _buffer(nbytes=1 << 16):
    buf = (ctypes.c_char * (nbytes + 256))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_kv_append_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(qkv=p, B=2, heads=2, dim_head=64, rot_dim=32, interleaved=1, cos=p + 4096, sin=p + 8192, pos=3, k=p + 16384, v=p + 32768, cap=8,
              stream=None)
    for change in [dict(qkv=None), dict(k=None), dict(v=None), dict(B=0), dict(heads=0), dict(dim_head=0), dict(dim_head=60), dict(pos=-1),
                   dict(pos=8), dict(cap=0), dict(rot_dim=72), dict(rot_dim=12), dict(rot_dim=-8), dict(cos=None), dict(sin=None),
                   dict(interleaved=2), dict(qkv=p + 2), dict(k=p + 16384 + 8)]:
        args = {**ok, **change}
        assert lib.tribe_kv_append(*args.values()) < 0, change
        assert b"tribe_kv_append" in lib.tribe_last_error(), change


def test_attention_decode_argument_errors_and_split_rule_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(q=p, ld_q=384, k=p + 4096, v=p + 8192, B=2, heads=2, dim_head=64, cap=16, n=5, scale=0.125, out=p + 16384, ws=p + 32768,
              ws_bytes=1 << 14, stream=None)
    for change in [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(B=0), dict(heads=0), dict(dim_head=96), dict(dim_head=256),
                   dict(n=0), dict(n=17), dict(ld_q=64), dict(ld_q=130), dict(q=p + 2), dict(k=p + 4096 + 8)]:
        args = {**ok, **change}
        assert lib.tribe_attention_decode_fwd(*args.values()) < 0, change
        assert b"tribe_attention_decode_fwd" in lib.tribe_last_error(), change
    # more than one split: the workspace is required, aligned and large enough
    many = {**ok, "cap": 4096, "n": 4096}
    assert lib.tribe_attention_decode_splits(2, 2, 4096) > 1
    need = lib.tribe_attention_decode_workspace_bytes(2, 2, 64, 4096)
    for change in [dict(ws=None), dict(ws=p + 32768 + 16), dict(ws_bytes=need - 1)]:
        assert lib.tribe_attention_decode_fwd(*{**many, **change}.values()) < 0, change
        assert b"tribe_attention_decode_fwd" in lib.tribe_last_error() and b"workspace" in lib.tribe_last_error()
    # the split count: a function of (B, heads, n) alone -- a power of two, never more workgroups than fill the chip once B * heads does,
    # each split at least 64 keys; the workspace holds (m, l) and dim_head floats per part
    for B, heads in ((1, 1), (1, 8), (3, 2), (16, 8), (64, 8)):
        last = 1
        for n in (1, 63, 64, 127, 128, 129, 1000, 1024, 4096, 100000):
            sp = lib.tribe_attention_decode_splits(B, heads, n)
            assert sp >= last and sp & (sp - 1) == 0 and sp <= 32 and (sp == 1 or (sp * 64 <= n and B * heads * sp // 2 < 256)), (B, heads, n, sp)
            assert lib.tribe_attention_decode_workspace_bytes(B, heads, 384, n) >= (0 if sp == 1 else B * heads * sp * (384 + 2) * 4)
            last = sp
    assert lib.tribe_attention_decode_splits(1, 8, 1024) == 16 and lib.tribe_attention_decode_splits(16, 8, 1024) == 2
    assert lib.tribe_attention_decode_splits(64, 8, 100000) == 1 and lib.tribe_attention_decode_splits(0, 8, 5) == 0


def _desc(_lib, **kw):
    d = _lib.EncoderDesc()
    d.B, d.T, d.dim, d.depth, d.heads, d.dim_head, d.ff_inner, d.rot_dim, d.rotary_interleaved = 2, 1, 256, 0, 4, 64, 1024, 0, 1
    d.norm_gain_scale, d.norm_eps = 16.0, 1e-12
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_encoder_step_and_prefill_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    byref = ctypes.byref
    assert lib.tribe_encoder_step_fwd(None, p, p, _lib.F32, p, p, 8, 0, p, 1 << 16, None) < 0
    assert b"tribe_encoder_step_fwd" in lib.tribe_last_error() and b"null descriptor" in lib.tribe_last_error()
    assert lib.tribe_encoder_prefill_fwd(None, p, p, _lib.F32, p, p, 8, p, 1 << 16, None) < 0
    assert b"tribe_encoder_prefill_fwd" in lib.tribe_last_error() and b"null descriptor" in lib.tribe_last_error()
    d = _desc(_lib, final_norm_g=p)
    ok = dict(d=byref(d), x=p, y=p + 4096, y_dtype=_lib.F32, k=p + 8192, v=p + 16384, cap=8, pos=0, ws=p + 32768, ws_bytes=1 << 15, stream=None)
    for change in [dict(x=None), dict(y=None), dict(k=None), dict(v=None), dict(ws=None), dict(pos=-1), dict(pos=8), dict(cap=0),
                   dict(ws=p + 32768 + 16), dict(ws_bytes=16)]:
        assert lib.tribe_encoder_step_fwd(*{**ok, **change}.values()) < 0, change
        assert b"tribe_encoder_step_fwd" in lib.tribe_last_error(), change
    two = _desc(_lib, final_norm_g=p, T=2)
    assert lib.tribe_encoder_step_fwd(*{**ok, "d": byref(two)}.values()) < 0 and b"one position" in lib.tribe_last_error()
    assert lib.tribe_encoder_step_workspace_bytes(byref(d), 8) > 0 and lib.tribe_encoder_step_workspace_bytes(None, 8) == 0
    assert lib.tribe_encoder_step_workspace_bytes(byref(d), 4096) >= lib.tribe_encoder_step_workspace_bytes(byref(d), 8)
    ok = dict(d=byref(two), x=p, y=p + 4096, y_dtype=_lib.F32, k=p + 8192, v=p + 16384, cap=8, ws=p + 32768, ws_bytes=1 << 15, stream=None)
    for change in [dict(x=None), dict(y=None), dict(k=None), dict(v=None), dict(ws=None), dict(cap=1), dict(k=p + 8192 + 8)]:
        assert lib.tribe_encoder_prefill_fwd(*{**ok, **change}.values()) < 0, change
        assert b"tribe_encoder_prefill_fwd" in lib.tribe_last_error(), change


# ---- ops: shape and dtype checks come first and begin with the C name ---------------------------------------------------------------------
def test_ops_checks_name_the_entry_point():
    from tribe_hip import ops

    bf, f = torch.bfloat16, torch.float32
    k = torch.zeros(2, 2, 8, 64, dtype=bf)
    qkv = torch.zeros(2, 384, dtype=bf)
    cos = torch.zeros(8, 16)
    with pytest.raises(ValueError, match=r"^tribe_kv_append: pos=8 outside"):
        ops.kv_append(qkv, k, k.clone(), 8, 32, cos, cos, True)
    with pytest.raises(ValueError, match=r"^tribe_kv_append: qkv must be"):
        ops.kv_append(qkv[:, :256], k, k.clone(), 0, 32, cos, cos, True)
    with pytest.raises(ValueError, match=r"^tribe_kv_append: cos must be"):
        ops.kv_append(qkv, k, k.clone(), 3, 32, cos[:3], cos, True)
    with pytest.raises(TypeError, match=r"^tribe_kv_append: k_cache must be bfloat16"):
        ops.kv_append(qkv, k.float(), k, 0, 32, cos, cos, True)
    with pytest.raises(ValueError, match=r"^tribe_kv_append: k_cache .* and v_cache .* differ"):
        ops.kv_append(qkv, k, torch.zeros(2, 2, 9, 64, dtype=bf), 0, 32, cos, cos, True)
    with pytest.raises(ValueError, match=r"^tribe_attention_decode_fwd: n=9 keys outside"):
        ops.attention_decode(qkv, k, k.clone(), 9, 0.125)
    with pytest.raises(ValueError, match=r"^tribe_attention_decode_fwd: n=0 keys outside"):
        ops.attention_decode(qkv, k, k.clone(), 0, 0.125)
    with pytest.raises(ValueError, match=r"^tribe_attention_decode_fwd: q must be \[B=2"):
        ops.attention_decode(qkv[:1], k, k.clone(), 1, 0.125)
    with pytest.raises(TypeError, match=r"^tribe_attention_decode_fwd: q must be torch.bfloat16"):
        ops.attention_decode(qkv.float(), k, k.clone(), 1, 0.125)
    with pytest.raises(ValueError, match=r"^tribe_attention_decode_fwd: dim_head=96"):
        ops.attention_decode(qkv, torch.zeros(2, 2, 8, 96, dtype=bf), torch.zeros(2, 2, 8, 96, dtype=bf), 1, 0.125)
    with pytest.raises(ValueError, match=r"^tribe_attention_decode_fwd: k_cache must be a contiguous \[B, heads, cap, dim_head\]"):
        ops.attention_decode(qkv, k[0], k[0], 1, 0.125)
    pack = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12, causal=True)
    plain = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12)
    caches = torch.zeros(1, 2, 4, 8, 64, dtype=bf)
    x = torch.zeros(2, 256, dtype=f)
    with pytest.raises(ValueError, match=r"^tribe_encoder_step_fwd: the encoder is bidirectional"):
        ops.encoder_step(x, plain, caches, caches.clone(), 0)
    with pytest.raises(ValueError, match=r"^tribe_encoder_step_fwd: pos=8 outside"):
        ops.encoder_step(x, pack, caches, caches.clone(), 8)
    with pytest.raises(ValueError, match=r"^tribe_encoder_step_fwd: x must be \[B=2"):
        ops.encoder_step(x[:1], pack, caches, caches.clone(), 0)
    with pytest.raises(ValueError, match=r"^tribe_encoder_step_fwd: caches .* do not match"):
        ops.encoder_step(x, pack, caches[:, :, :2].contiguous(), caches[:, :, :2].contiguous(), 0)
    with pytest.raises(ValueError, match=r"^tribe_encoder_prefill_fwd: T=9 positions do not fit"):
        ops.encoder_prefill(torch.zeros(18, 256), pack, caches, caches.clone(), 9)
    with pytest.raises(ValueError, match=r"^tribe_encoder_prefill_fwd: x must be a contiguous f32 \[B\*T=6"):
        ops.encoder_prefill(torch.zeros(5, 256), pack, caches, caches.clone(), 3)
    with pytest.raises(ValueError, match=r"^tribe_encoder_prefill_fwd: the encoder is bidirectional"):
        ops.encoder_prefill(torch.zeros(6, 256), plain, caches, caches.clone(), 3)


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
def _encoder(causal=True, **kw):
    from modeling_utils.models.transformer import TransformerEncoderConfig

    return TransformerEncoderConfig(depth=2, heads=4, causal=causal, **kw).build(256)


def test_new_cache_allocates_the_stated_shapes():
    from modeling_utils.models.transformer import EncoderCache

    enc = _encoder()
    cache = enc.new_cache(3, 50)
    assert isinstance(cache, EncoderCache) and cache.pos == 0
    for t in (cache.k, cache.v):
        assert tuple(t.shape) == (2, 3, 4, 50, 64) and t.dtype == torch.bfloat16 and t.is_contiguous() and t.device.type == "cpu"
    assert cache.k.data_ptr() != cache.v.data_ptr() and (cache.batch_size, cache.max_len, cache.device) == (3, 50, torch.device("cpu"))
    assert cache.k.numel() * 2 + cache.v.numel() * 2 == 2 * 2 * 3 * 4 * 50 * 64 * 2          # 2 * depth * B * heads * cap * dim_head * 2
    cache.pos = 7
    cache.reset()
    assert cache.pos == 0
    assert enc.new_cache(1, 1, device="meta").k.device.type == "meta"
    for bad in ((0, 5), (2, 0), (-1, 5)):
        with pytest.raises(ValueError, match="must be positive"):
            enc.new_cache(*bad)


def test_bidirectional_encoders_have_no_incremental_form():
    enc = _encoder(causal=False)
    with pytest.raises(ValueError, match="no incremental form"):
        enc.new_cache(2, 8)
    cache = _encoder().new_cache(2, 8)
    with pytest.raises(ValueError, match="no incremental form"):
        enc.step(torch.zeros(2, 256), cache)
    with pytest.raises(ValueError, match="no incremental form"):
        enc.prefill(torch.zeros(2, 3, 256), cache)


def test_step_and_prefill_value_errors():
    from modeling_utils.models.transformer import EncoderCache

    enc = _encoder()
    cache = enc.new_cache(2, 8)
    with pytest.raises(ValueError, match="batch size 3 does not match the cache's 2"):
        enc.step(torch.zeros(3, 256), cache)
    with pytest.raises(ValueError, match="batch size 3 does not match the cache's 2"):
        enc.prefill(torch.zeros(3, 4, 256), cache)
    with pytest.raises(ValueError, match="expected last dim 256"):
        enc.step(torch.zeros(2, 128), cache)
    with pytest.raises(ValueError, match=r"expected \[B, dim\]"):
        enc.step(torch.zeros(2, 1, 256), cache)
    with pytest.raises(ValueError, match=r"expected \[B, T0, dim\]"):
        enc.prefill(torch.zeros(2, 256), cache)
    with pytest.raises(ValueError, match="x is on meta, the cache on cpu"):
        enc.step(torch.zeros(2, 256, device="meta"), cache)
    with pytest.raises(ValueError, match="x is on meta, the cache on cpu"):
        enc.prefill(torch.zeros(2, 3, 256, device="meta"), cache)
    with pytest.raises(ValueError, match="run past max_len=8"):
        enc.prefill(torch.zeros(2, 9, 256), cache)
    cache.pos = 8
    with pytest.raises(ValueError, match="run past max_len=8"):
        enc.step(torch.zeros(2, 256), cache)
    cache.pos = 3
    with pytest.raises(ValueError, match="already holds 3 positions"):
        enc.prefill(torch.zeros(2, 4, 256), cache)
    with pytest.raises(ValueError, match="was not made for this encoder"):
        enc.step(torch.zeros(2, 256), EncoderCache(1, 2, 4, 8, 64, None))                   # a one-layer encoder's cache
    with pytest.raises(TypeError, match="must be an EncoderCache"):
        enc.step(torch.zeros(2, 256), None)
    assert "nference only" in enc.step.__doc__ and "nference only" in enc.prefill.__doc__


def test_model_stream_value_errors():
    from algonauts2025.model import EncoderStream, FmriEncoderConfig

    fdims = {"text": (1, 24), "audio": (1, 16)}
    plain = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32).build(fdims, 12, 5)
    with pytest.raises(ValueError, match="no incremental form"):
        plain.stream(2)
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32, causal=True).build(fdims, 12, 5)
    stream = model.stream(2)
    assert isinstance(stream, EncoderStream) and stream.pos == 0 and tuple(stream.cache.k.shape) == (1, 2, 4, 32, 64)   # None: max_timesteps
    assert model.stream(3, max_len=7).cache.max_len == 7
    with pytest.raises(ValueError, match="exceeds the positional table"):
        model.stream(2, max_len=33)
    sid = torch.zeros(2, 1, dtype=torch.int64)
    step = {"text": torch.zeros(2, 1, 24, 1), "audio": torch.zeros(2, 16, 1), "subject_id": sid}
    with pytest.raises(ValueError, match="batch size 3 does not match the stream's 2"):
        stream.push({**step, "text": torch.zeros(3, 1, 24, 1)})
    with pytest.raises(ValueError, match="expected one time step per call"):
        stream.push({"text": torch.zeros(2, 1, 24, 2), "audio": torch.zeros(2, 16, 2), "subject_id": sid})
    with pytest.raises(ValueError, match="disagree on the number of time steps"):
        stream.prefill({**step, "text": torch.zeros(2, 1, 24, 3)})
    with pytest.raises(ValueError, match="is on meta, the stream on cpu"):
        stream.push({**step, "audio": torch.zeros(2, 16, 1, device="meta")})
    with pytest.raises(ValueError, match="none of the modalities"):
        stream.push({"subject_id": sid})
    with pytest.raises(ValueError, match="run past max_len=32"):
        stream.prefill({"text": torch.zeros(2, 1, 24, 33), "audio": torch.zeros(2, 16, 33), "subject_id": sid})
    stream.cache.pos = 32
    with pytest.raises(ValueError, match="run past max_len=32"):
        stream.push(step)
    stream.cache.pos = 4
    with pytest.raises(ValueError, match="already holds 4 steps"):
        stream.prefill(step)
    stream.reset()
    assert stream.pos == 0
