"""CPU (no GPU): the host surface of slots -- independent timelines in one KV cache, a position per sequence.  The five new C entry points
(declared in the header, bound with matching prototypes, the ABI version unchanged), their argument errors, which name the entry point and
need no device, the ValueErrors of the ops wrappers (positions are validated on the host before any launch), the bookkeeping of
EncoderSlots, the errors of HipEncoder.step_slots / extend_slots and of SlotStream, and what stays as it was: `step` refuses an EncoderSlots,
`stream()` still returns an EncoderStream."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_slot_entry_points():
    from tribe_hip import _lib

    C = ctypes
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    desc = C.POINTER(_lib.EncoderDesc)
    want = {
        "tribe_kv_append_slots": (C.c_int, [vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
        "tribe_attention_decode_slots_fwd": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, vp, i64, f32, vp, vp, sz, vp]),
        "tribe_attention_extend_slots_fwd": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, vp, i64, f32, vp, vp]),
        "tribe_encoder_step_slots_fwd": (C.c_int, [desc, vp, vp, i32, vp, vp, i64, vp, i64, vp, sz, vp]),
        "tribe_encoder_extend_slots_fwd": (C.c_int, [desc, vp, vp, i32, vp, vp, i64, vp, vp, sz, vp]),
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
        assert re.search(r"const int32_t\s*\*\s*pos\b", declared), f"{name}: positions are a const int32_t* pos"
    # additive: the version, the descriptor and the streaming entry points of before stand
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5 and _lib.lib().tribe_version() == 5
    assert _lib.SIGNATURES["tribe_kv_append_block"] == (C.c_int, [vp, i64, i64, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp])
    assert _lib.SIGNATURES["tribe_attention_decode_fwd"] == (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, i64, f32, vp, vp, sz, vp])
    assert _lib.SIGNATURES["tribe_attention_extend_fwd"] == (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i64, i64, i64, f32, vp, vp])
    assert _lib.SIGNATURES["tribe_encoder_step_fwd"] == (C.c_int, [desc, vp, vp, i32, vp, vp, i64, i64, vp, sz, vp])
    assert _lib.SIGNATURES["tribe_encoder_extend_fwd"] == (C.c_int, [desc, vp, vp, i32, vp, vp, i64, i64, vp, sz, vp])


def _buffer(nbytes=1 << 16):
    buf = (ctypes.c_char * (nbytes + 256))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_kv_append_slots_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(qkv=p, B=2, k=3, heads=2, dim_head=64, rot_dim=32, interleaved=1, cos=p + 4096, sin=p + 8192, pos=p + 12288, kc=p + 16384,
              vc=p + 32768, cap=8, stream=None)
    for change in [dict(pos=None), dict(qkv=None), dict(kc=None), dict(vc=None), dict(B=0), dict(heads=0), dict(dim_head=0), dict(dim_head=60),
                   dict(k=0), dict(k=-1), dict(k=9), dict(cap=0), dict(rot_dim=72), dict(rot_dim=12), dict(rot_dim=-8), dict(cos=None),
                   dict(sin=None), dict(interleaved=2), dict(qkv=p + 2), dict(kc=p + 16384 + 8), dict(pos=p + 12288 + 2)]:
        args = {**ok, **change}
        assert lib.tribe_kv_append_slots(*args.values()) < 0, change
        assert b"tribe_kv_append_slots" in lib.tribe_last_error(), change


def test_attention_slots_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    ok = dict(q=p, ld_q=384, kc=p + 4096, vc=p + 8192, B=2, heads=2, dim_head=64, cap=16, pos=p + 12288, n_max=5, scale=0.125, out=p + 16384,
              ws=p + 32768, ws_bytes=1 << 15, stream=None)
    for change in [dict(pos=None), dict(q=None), dict(kc=None), dict(vc=None), dict(out=None), dict(B=0), dict(heads=0), dict(dim_head=96),
                   dict(dim_head=256), dict(dim_head=0), dict(n_max=0), dict(n_max=-3), dict(n_max=17), dict(cap=0), dict(ld_q=64),
                   dict(ld_q=130), dict(q=p + 2), dict(kc=p + 4096 + 8), dict(vc=p + 8192 + 8), dict(pos=p + 12288 + 2)]:
        args = {**ok, **change}
        assert lib.tribe_attention_decode_slots_fwd(*args.values()) < 0, change
        assert b"tribe_attention_decode_slots_fwd" in lib.tribe_last_error(), change
    # more than one split needs the workspace: B * heads = 4, n_max = 1024 -> 16 splits
    split = {**ok, "cap": 1024, "n_max": 1024}
    assert lib.tribe_attention_decode_splits(2, 2, 1024) > 1
    for change in [dict(ws=None), dict(ws=p + 32768 + 16), dict(ws_bytes=16)]:
        assert lib.tribe_attention_decode_slots_fwd(*{**split, **change}.values()) < 0, change
        assert b"tribe_attention_decode_slots_fwd" in lib.tribe_last_error(), change

    ok = dict(q=p, ld_q=384, kc=p + 4096, vc=p + 8192, B=2, heads=2, dim_head=64, cap=16, pos=p + 12288, k=4, scale=0.125, out=p + 16384,
              stream=None)
    for change in [dict(pos=None), dict(q=None), dict(kc=None), dict(vc=None), dict(out=None), dict(B=0), dict(heads=0), dict(dim_head=96),
                   dict(dim_head=256), dict(dim_head=0), dict(k=0), dict(k=-2), dict(k=17), dict(cap=0), dict(ld_q=64), dict(ld_q=130),
                   dict(q=p + 2), dict(kc=p + 4096 + 8), dict(vc=p + 8192 + 8), dict(out=p + 16384 + 4), dict(pos=p + 12288 + 2)]:
        args = {**ok, **change}
        assert lib.tribe_attention_extend_slots_fwd(*args.values()) < 0, change
        assert b"tribe_attention_extend_slots_fwd" in lib.tribe_last_error(), change


def _desc(_lib, **kw):
    d = _lib.EncoderDesc()
    d.B, d.T, d.dim, d.depth, d.heads, d.dim_head, d.ff_inner, d.rot_dim, d.rotary_interleaved = 2, 3, 256, 0, 4, 64, 1024, 0, 1
    d.norm_gain_scale, d.norm_eps = 16.0, 1e-12
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_encoder_slots_argument_errors_need_no_gpu():
    from tribe_hip import _lib

    lib = _lib.lib()
    keep, p = _buffer()
    byref = ctypes.byref
    assert lib.tribe_encoder_step_slots_fwd(None, p, p, _lib.F32, p, p, 8, p, 1, p, 1 << 16, None) < 0
    assert b"tribe_encoder_step_slots_fwd" in lib.tribe_last_error() and b"null descriptor" in lib.tribe_last_error()
    assert lib.tribe_encoder_extend_slots_fwd(None, p, p, _lib.F32, p, p, 8, p, p, 1 << 16, None) < 0
    assert b"tribe_encoder_extend_slots_fwd" in lib.tribe_last_error() and b"null descriptor" in lib.tribe_last_error()

    one = _desc(_lib, final_norm_g=p, T=1)
    ok = dict(d=byref(one), x=p, y=p + 4096, y_dtype=_lib.F32, kc=p + 8192, vc=p + 16384, cap=8, pos=p + 24576, n_max=5, ws=p + 32768,
              ws_bytes=1 << 15, stream=None)
    for change in [dict(pos=None), dict(x=None), dict(y=None), dict(kc=None), dict(vc=None), dict(ws=None), dict(n_max=0), dict(n_max=9),
                   dict(cap=0), dict(ws=p + 32768 + 16), dict(ws_bytes=16), dict(d=byref(_desc(_lib, final_norm_g=p, T=2)))]:
        assert lib.tribe_encoder_step_slots_fwd(*{**ok, **change}.values()) < 0, change
        assert b"tribe_encoder_step_slots_fwd" in lib.tribe_last_error(), change

    d = _desc(_lib, final_norm_g=p)
    ok = dict(d=byref(d), x=p, y=p + 4096, y_dtype=_lib.F32, kc=p + 8192, vc=p + 16384, cap=8, pos=p + 24576, ws=p + 32768, ws_bytes=1 << 15,
              stream=None)
    for change in [dict(pos=None), dict(x=None), dict(y=None), dict(kc=None), dict(vc=None), dict(ws=None), dict(cap=0), dict(cap=2),
                   dict(kc=p + 8192 + 8), dict(ws=p + 32768 + 16), dict(ws_bytes=16)]:
        assert lib.tribe_encoder_extend_slots_fwd(*{**ok, **change}.values()) < 0, change
        assert b"tribe_encoder_extend_slots_fwd" in lib.tribe_last_error(), change
    for bad in (_desc(_lib, final_norm_g=p, T=0), _desc(_lib, final_norm_g=p, T=-1), _desc(_lib, final_norm_g=p, T=9),
                _desc(_lib, final_norm_g=p, dim_head=256), _desc(_lib, final_norm_g=p, dim_head=320)):
        assert lib.tribe_encoder_extend_slots_fwd(*{**ok, "d": byref(bad)}.values()) < 0, (bad.T, bad.dim_head)
        assert b"tribe_encoder_extend_slots_fwd" in lib.tribe_last_error(), (bad.T, bad.dim_head)


# ---- ops: positions are validated on the host, the message begins with the C name ---------------------------------------------------------
def test_ops_checks_name_the_entry_point():
    from tribe_hip import ops

    bf, f = torch.bfloat16, torch.float32
    kc = torch.zeros(2, 2, 8, 64, dtype=bf)
    qkv = torch.zeros(6, 384, dtype=bf)                                                 # B = 2, k = 3
    cos = torch.zeros(8, 16)
    what = "tribe_kv_append_slots"
    with pytest.raises(ValueError, match=rf"^{what}: pos\[1\]=6 .. \+k=9 outside the cache capacity 8"):
        ops.kv_append_slots(qkv, kc, kc.clone(), [0, 6], 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: pos\[0\]=-2 "):
        ops.kv_append_slots(qkv, kc, kc.clone(), [-2, 0], 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: pos holds 3 positions for B=2"):
        ops.kv_append_slots(qkv, kc, kc.clone(), [0, 0, 0], 3, 32, cos, cos, True)
    with pytest.raises(TypeError, match=rf"^{what}: pos must be a list or tuple of ints"):
        ops.kv_append_slots(qkv, kc, kc.clone(), torch.zeros(2, dtype=torch.int32), 3, 32, cos, cos, True)
    with pytest.raises(TypeError, match=rf"^{what}: pos\[1\] must be an int"):
        ops.kv_append_slots(qkv, kc, kc.clone(), [0, 1.0], 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: k=0 must be at least 1"):
        ops.kv_append_slots(qkv[:0], kc, kc.clone(), [0, 0], 0, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: qkv must be contiguous \[B\*k=6, 384\]"):
        ops.kv_append_slots(qkv[:4], kc, kc.clone(), [0, -1], 3, 32, cos, cos, True)
    with pytest.raises(ValueError, match=rf"^{what}: cos must be a contiguous f32 \[>= cap=8"):
        ops.kv_append_slots(qkv, kc, kc.clone(), [0, 5], 3, 32, cos[:7], cos, True)
    with pytest.raises(TypeError, match=rf"^{what}: k_cache must be bfloat16"):
        ops.kv_append_slots(qkv, kc.float(), kc, [0, 0], 3, 32, cos, cos, True)
    what = "tribe_attention_decode_slots_fwd"
    q = torch.zeros(2, 128, dtype=bf)
    with pytest.raises(ValueError, match=rf"^{what}: pos\[0\]=8 "):
        ops.attention_decode_slots(q, kc, kc.clone(), [8, 0], 8, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: n_max=9 keys outside 1 .. capacity 8"):
        ops.attention_decode_slots(q, kc, kc.clone(), [0, 0], 9, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: n_max=0 keys outside"):
        ops.attention_decode_slots(q, kc, kc.clone(), [-1, -1], 0, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: n_max=3 is no upper bound"):
        ops.attention_decode_slots(q, kc, kc.clone(), [1, 3], 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: dim_head=96"):
        ops.attention_decode_slots(q, torch.zeros(2, 2, 8, 96, dtype=bf), torch.zeros(2, 2, 8, 96, dtype=bf), [0, 0], 1, 0.125)
    with pytest.raises(TypeError, match=rf"^{what}: q must be torch.bfloat16"):
        ops.attention_decode_slots(q.float(), kc, kc.clone(), [0, 0], 1, 0.125)
    what = "tribe_attention_extend_slots_fwd"
    with pytest.raises(ValueError, match=rf"^{what}: pos\[1\]=6 .. \+k=9 outside"):
        ops.attention_extend_slots(qkv, kc, kc.clone(), [-1, 6], 3, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: k=0 must be at least 1"):
        ops.attention_extend_slots(qkv, kc, kc.clone(), [0, 0], 0, 0.125)
    with pytest.raises(ValueError, match=rf"^{what}: q must be \[B\*k=6, >= 128\]"):
        ops.attention_extend_slots(qkv[:5], kc, kc.clone(), [0, 0], 3, 0.125)
    pack = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12, causal=True)
    plain = ops.EncoderPack(256, 1, 4, 64, 1024, 32, True, 16.0, 1e-12)
    caches = torch.zeros(1, 2, 4, 8, 64, dtype=bf)
    what = "tribe_encoder_step_slots_fwd"
    x1 = torch.zeros(2, 256, dtype=f)
    with pytest.raises(ValueError, match=rf"^{what}: the encoder is bidirectional"):
        ops.encoder_step_slots(x1, plain, caches, caches.clone(), [0, 0])
    with pytest.raises(ValueError, match=rf"^{what}: pos\[1\]=8 "):
        ops.encoder_step_slots(x1, pack, caches, caches.clone(), [0, 8])
    with pytest.raises(ValueError, match=rf"^{what}: x must be contiguous \[B=2, dim=256\]"):
        ops.encoder_step_slots(torch.zeros(2, 512, dtype=f)[:, :256], pack, caches, caches.clone(), [0, 0])
    what = "tribe_encoder_extend_slots_fwd"
    x = torch.zeros(6, 256, dtype=f)
    with pytest.raises(ValueError, match=rf"^{what}: the encoder is bidirectional"):
        ops.encoder_extend_slots(x, plain, caches, caches.clone(), [0, 0], 3)
    with pytest.raises(ValueError, match=rf"^{what}: pos\[0\]=6 .. \+k=9 outside"):
        ops.encoder_extend_slots(x, pack, caches, caches.clone(), [6, 0], 3)
    with pytest.raises(ValueError, match=rf"^{what}: x must be contiguous \[B\*k=6, 256\]"):
        ops.encoder_extend_slots(x[:4], pack, caches, caches.clone(), [0, 0], 3)


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
def _encoder(causal=True, **kw):
    from modeling_utils.models.transformer import TransformerEncoderConfig

    return TransformerEncoderConfig(depth=2, heads=4, causal=causal, **kw).build(256)


def test_encoder_slots_bookkeeping():
    from modeling_utils.models.transformer import EncoderCache, EncoderSlots

    enc = _encoder()
    slots = enc.new_slots(3, 8)
    assert isinstance(slots, EncoderSlots) and not isinstance(slots, EncoderCache) and not issubclass(EncoderSlots, EncoderCache)
    assert slots.k.shape == slots.v.shape == (2, 3, 4, 8, 64) and slots.k.dtype == slots.v.dtype == torch.bfloat16
    assert (slots.batch_size, slots.max_len, slots.device) == (3, 8, torch.device("cpu"))
    assert slots.positions == [0, 0, 0] and not hasattr(slots, "pos")
    slots.positions = [4, 5, 6]
    slots.reset([1])
    assert slots.positions == [4, 0, 6]
    slots.reset([0, 2])
    assert slots.positions == [0, 0, 0]
    slots.positions = [4, 5, 6]
    slots.reset()
    assert slots.positions == [0, 0, 0]
    slots.positions = [1, 2, 3]
    for bad in ([3], [-1], [True]):
        with pytest.raises(ValueError, match=r"EncoderSlots.reset: slot index .* outside \[0, 3\)"):
            slots.reset(bad)
    assert slots.positions == [1, 2, 3]                                               # a refused reset resets nothing
    # `active` as indices and as a mask select the same slots
    assert slots.select("t", [0, 2]) == slots.select("t", [True, False, True]) == slots.select("t", (2, 0)) == [True, False, True]
    assert slots.select("t", torch.tensor([True, False, True])) == [True, False, True]
    assert slots.select("t", None) == slots.select("t", [0, 1, 2]) == slots.select("t", [True] * 3) == [True, True, True]
    with pytest.raises(ValueError, match=r"new_slots: batch_size=0"):
        enc.new_slots(0, 8)
    with pytest.raises(ValueError, match="no incremental form"):
        _encoder(causal=False).new_slots(2, 8)


def test_slot_call_value_errors():
    from modeling_utils.models.transformer import EncoderSlots

    enc = _encoder()
    slots = enc.new_slots(3, 8)
    x, xb = torch.zeros(3, 256), torch.zeros(3, 2, 256)
    slots.positions = [0, 8, 7]
    with pytest.raises(ValueError, match=r"HipEncoder.step_slots: slot 1: 8 positions filled \+ 1 would run past max_len=8"):
        enc.step_slots(x, slots)
    with pytest.raises(ValueError, match=r"HipEncoder.extend_slots: slot 2: 7 positions filled \+ 2 would run past max_len=8"):
        enc.extend_slots(xb, slots, active=[0, 2])
    with pytest.raises(ValueError, match=r"HipEncoder.extend_slots: slot 1: 8 positions filled \+ 2"):
        enc.extend_slots(xb, slots, active=[False, True, False])
    for name, call in (("step_slots", lambda a: enc.step_slots(x, slots, a)), ("extend_slots", lambda a: enc.extend_slots(xb, slots, a))):
        with pytest.raises(ValueError, match=rf"HipEncoder.{name}: active is empty"):
            call([])
        with pytest.raises(ValueError, match=rf"HipEncoder.{name}: active is empty"):
            call([False, False, False])
        with pytest.raises(ValueError, match=rf"HipEncoder.{name}: active slot index 3 outside \[0, 3\)"):
            call([0, 3])
        with pytest.raises(ValueError, match=rf"HipEncoder.{name}: active slot index -1 outside \[0, 3\)"):
            call([-1])
        with pytest.raises(ValueError, match=rf"HipEncoder.{name}: the active mask holds 2 flags for 3 slots"):
            call([True, False])
    with pytest.raises(ValueError, match="no incremental form"):
        _encoder(causal=False).step_slots(x, slots)
    with pytest.raises(ValueError, match="no incremental form"):
        _encoder(causal=False).extend_slots(xb, slots)
    with pytest.raises(ValueError, match=r"HipEncoder.step_slots: expected \[B, dim\]"):
        enc.step_slots(xb, slots)
    with pytest.raises(ValueError, match=r"HipEncoder.extend_slots: expected \[B, k, dim\]"):
        enc.extend_slots(x, slots)
    with pytest.raises(ValueError, match="batch size 2 does not match the 3 slots"):
        enc.step_slots(x[:2], slots, [0])
    with pytest.raises(ValueError, match="expected last dim 256"):
        enc.step_slots(torch.zeros(3, 128), slots, [0])
    with pytest.raises(ValueError, match="x is on meta, the slots on cpu"):
        enc.step_slots(torch.zeros(3, 256, device="meta"), slots, [0])
    with pytest.raises(ValueError, match="k must be at least 1"):
        enc.extend_slots(torch.zeros(3, 0, 256), slots, [0])
    from modeling_utils.models.transformer import EncoderSlots

    with pytest.raises(ValueError, match="were not made for this encoder"):
        enc.step_slots(x, EncoderSlots(1, 3, 4, 8, 64, None), [0])
    with pytest.raises(TypeError, match="slots must be an EncoderSlots"):
        enc.step_slots(x, enc.new_cache(3, 8))
    assert slots.positions == [0, 8, 7]                                               # a refused call leaves the slots where they were
    assert "nference only" in enc.step_slots.__doc__ and "nference only" in enc.extend_slots.__doc__


def test_uniform_entry_points_refuse_slots():
    enc = _encoder()
    slots = enc.new_slots(2, 8)
    with pytest.raises(TypeError, match="HipEncoder.step: cache must be an EncoderCache"):
        enc.step(torch.zeros(2, 256), slots)
    with pytest.raises(TypeError, match="HipEncoder.extend: cache must be an EncoderCache"):
        enc.extend(torch.zeros(2, 3, 256), slots)
    with pytest.raises(TypeError, match="HipEncoder.prefill: cache must be an EncoderCache"):
        enc.prefill(torch.zeros(2, 3, 256), slots)


def test_stream_kinds_and_slot_stream_value_errors():
    from algonauts2025.model import EncoderStream, FmriEncoderConfig, SlotStream

    fdims = {"text": (1, 24), "audio": (1, 16)}
    model = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32, causal=True).build(fdims, 12, 5)
    assert type(model.stream(2)) is EncoderStream and type(model.stream(2, 16)) is EncoderStream
    assert type(model.stream(2, independent=False)) is EncoderStream
    stream = model.stream(3, independent=True)
    assert type(stream) is SlotStream and not isinstance(stream, EncoderStream)
    assert stream.positions == [0, 0, 0] and stream.slots.max_len == 32 and model.stream(3, 16, independent=True).slots.max_len == 16
    sid = torch.zeros(3, 1, dtype=torch.int64)
    step = {"text": torch.zeros(3, 1, 24, 1), "audio": torch.zeros(3, 16, 1), "subject_id": sid}
    block = {"text": torch.zeros(3, 1, 24, 3), "audio": torch.zeros(3, 16, 3), "subject_id": sid}
    with pytest.raises(ValueError, match="SlotStream.push: text: batch size 2 does not match the stream's 3 slots"):
        stream.push({**step, "text": torch.zeros(2, 1, 24, 1)})
    with pytest.raises(ValueError, match=r"SlotStream.push: expected one time step per call"):
        stream.push(block)
    with pytest.raises(ValueError, match="SlotStream.push_block: modalities disagree on the number of time steps"):
        stream.push_block({**block, "text": torch.zeros(3, 1, 24, 4)})
    with pytest.raises(ValueError, match="none of the modalities"):
        stream.push({"subject_id": sid})
    with pytest.raises(ValueError, match="SlotStream.push: active is empty"):
        stream.push(step, active=[])
    with pytest.raises(ValueError, match=r"SlotStream.push_block: active slot index 3 outside \[0, 3\)"):
        stream.push_block(block, active=[3])
    stream.slots.positions = [0, 30, 32]
    with pytest.raises(ValueError, match=r"SlotStream.push: slot 2: 32 steps seen \+ 1 would run past max_len=32"):
        stream.push(step)
    with pytest.raises(ValueError, match=r"SlotStream.push_block: slot 1: 30 steps seen \+ 3 would run past max_len=32"):
        stream.push_block(block, active=[True, True, False])
    assert stream.positions == [0, 30, 32]
    stream.reset([2])
    assert stream.positions == [0, 30, 0]
    stream.reset()
    assert stream.positions == [0, 0, 0]
    got = stream.positions
    got[0] = 5
    assert stream.positions == [0, 0, 0]                                              # `positions` hands out a copy
    with pytest.raises(ValueError, match="exceeds the positional table"):
        model.stream(2, 33, independent=True)
    plain = FmriEncoderConfig(n_subjects=2, hidden=256, depth=1, heads=4, max_timesteps=32).build(fdims, 12, 5)
    with pytest.raises(ValueError, match="no incremental form"):
        plain.stream(2, independent=True)
