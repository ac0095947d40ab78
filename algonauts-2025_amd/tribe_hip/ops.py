"""torch-tensor front end of the C ABI: validates shapes / devices on the host (mirroring
the reference's assert-style checks), hands raw device pointers + the current HIP
stream to libtribe_hip.so.  torch is used for memory, streams and nothing else."""

from __future__ import annotations

import ctypes as C
import functools as _functools
import math as _math
import typing as tp

import numpy as _np
import torch

from . import _lib
from ._lib import BF16, F32, F64, AttentionDesc, EncoderDesc, EncoderLayer, GemmDesc, LlamaDesc, LlamaLayer, check, lib

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float64: F64}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _cuda(t: torch.Tensor, dtype: torch.dtype | tuple[torch.dtype, ...] | None, name: str, contiguous: bool = True) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.TribeHipError(f"{name}: tensor is on {t.device}; the TRIBE hot path runs on the GPU only (no CPU fallback)")
    if dtype is not None:
        ok = t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype
        if not ok:
            raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# --------------------------------------------------------------------------------------
# workspace: one grow-only byte buffer per device, owned by the torch caching allocator
# --------------------------------------------------------------------------------------
_WS: dict[tuple[int, str], torch.Tensor] = {}


def workspace(nbytes: int, device: torch.device, tag: str = "main") -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# --------------------------------------------------------------------------------------
# generic MFMA GEMM
# --------------------------------------------------------------------------------------
_ACT = {"gelu": _lib.ACT_GELU, "swiglu": _lib.ACT_SWIGLU, "silu": _lib.ACT_SILU, "glu": _lib.ACT_GLU, None: _lib.ACT_NONE}


def _gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, lda=None, ldb=None, ldc=None, M=None, N=None, K=None, alpha=1.0,
          bias=None, act=_lib.ACT_NONE, aux=None, res=None, ldres=None, res_scale=None, batch1=1, batch0=1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
          gather1=None, gather_a=False, gather_b=False, a_off=0, b_off=0, c_off=0, role=_lib.ROLE["generic"], trans_ab=False,
          row_bias=None, row_bias_off=0, sBias=(0, 0), ld_aux=None, stream_k=False, sRes=None, rowadd=None, rowadd_period=0,
          gadd=None, gadd_index=None, gadd_div=0, tile_hint=0, fp8=False) -> bool:
    """The one place a tribe_gemm_desc is filled and launched (tribe_gemm_bf16; fp8: tribe_gemm_fp8 on e4m3 bytes).  Element offsets and
    batch strides allow strided views without copies.  N is the width of the product: a gated activation (SwiGLU / GLU) stores N / 2
    columns, so its caller passes ldc (and sC) for the stored width while the residual keeps ldres / sRes (default: ldc / sC).
    bias: f32 per output column; row_bias: f32 per output row, batch strides sBias (elements).
    stream_k: let the launcher share the reduction of tiles out over workgroups (workspace taken from `workspace`); returns whether it did."""
    d = GemmDesc(M=M, N=N, K=K, batch1=batch1, batch0=batch0,
                 A=a.data_ptr() + a.element_size() * a_off, lda=lda, sA1=sA[0], sA0=sA[1],
                 B=b.data_ptr() + b.element_size() * b_off, ldb=ldb, sB1=sB[0], sB0=sB[1],
                 C=out.data_ptr() + out.element_size() * c_off, ldc=ldc, sC1=sC[0], sC0=sC[1],
                 c_dtype=_DT[out.dtype], alpha=alpha, act=act, role=role, tile_hint=tile_hint, trans_ab=int(trans_ab), stream_k=int(stream_k))
    if bias is not None:
        d.bias, d.bias_mode = bias.data_ptr(), _lib.BIAS_COL
    if row_bias is not None:
        d.bias, d.bias_mode, d.sBias1, d.sBias0 = row_bias.data_ptr() + 4 * row_bias_off, _lib.BIAS_ROW, sBias[0], sBias[1]
    if aux is not None:
        d.aux, d.ld_aux = aux.data_ptr(), (ld_aux if ld_aux is not None else N)
    if res is not None:
        d.res, d.ldres = res.data_ptr() + 4 * c_off, (ldres if ldres is not None else ldc)
        d.sRes1, d.sRes0 = sC if sRes is None else sRes
    if res_scale is not None:
        d.res_scale = res_scale.data_ptr()
    if gather1 is not None:
        d.gather1, d.gather_a, d.gather_b = gather1.data_ptr(), int(gather_a), int(gather_b)
    if rowadd is not None:
        d.rowadd, d.ld_rowadd, d.rowadd_period = rowadd.data_ptr(), rowadd.shape[-1], rowadd_period
    if gadd is not None:
        d.gadd, d.gadd_index, d.gadd_div, d.ld_gadd = gadd.data_ptr(), gadd_index.data_ptr(), gadd_div, gadd.shape[-1]
    split = False
    if stream_k:
        nbytes = lib().tribe_gemm_stream_k_workspace_bytes(C.byref(d))
        split = nbytes > 0
        if split:   # parts of split tiles travel through the workspace; a second launch sums them in order
            ws = workspace(nbytes, out.device, tag="streamk")
            d.stream_k_ws, d.stream_k_ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    what = "tribe_gemm_fp8" if fp8 else "tribe_gemm_bf16"
    check(getattr(lib(), what)(C.byref(d), _stream()), what)
    return split


def gemm_nt(
    a: torch.Tensor, b: torch.Tensor, *, bias: torch.Tensor | None = None, bias_row: bool = False, act: str | None = None,
    res: torch.Tensor | None = None, res_scale: torch.Tensor | None = None, alpha: float = 1.0,
    out_dtype: torch.dtype = torch.float32, out: torch.Tensor | None = None,
    rowadd: torch.Tensor | None = None, rowadd_period: int = 0,
    gadd: torch.Tensor | None = None, gadd_index: torch.Tensor | None = None, gadd_div: int = 0, tile_hint: int = 0,
    split_k: bool = False,
) -> torch.Tensor:
    """out[..., m, n] = epi(alpha * sum_k a[..., m, k] * b[..., n, k]); a, b bf16 with equal leading batch dim (or 2-D).
    split_k: let the launcher share the reduction of a small grid out over several workgroups per tile (tribe_gemm_desc.stream_k);
    gemm_nt.last_split tells whether it did."""
    _cuda(a, torch.bfloat16, "a")
    _cuda(b, torch.bfloat16, "b")
    if a.ndim == 2:
        a3, b3 = a[None], b[None]
    else:
        a3, b3 = a, b
    if a3.ndim != 3 or b3.ndim != 3 or a3.shape[0] != b3.shape[0] or a3.shape[2] != b3.shape[2]:
        raise ValueError(f"gemm_nt: incompatible shapes {tuple(a.shape)} x {tuple(b.shape)}")
    Z, M, K = a3.shape
    N = b3.shape[1]
    n_out = N // 2 if act in ("swiglu", "glu") else N  # SwiGLU / GLU fold adjacent column pairs
    if out is None:
        out = torch.empty((Z, M, n_out) if a.ndim == 3 else (M, n_out), dtype=out_dtype, device=a.device)
    _cuda(out, (torch.float32, torch.bfloat16), "out")
    for name, t, dtype in (("bias", bias, torch.float32), ("res", res, torch.float32), ("res_scale", res_scale, torch.float32),
                           ("rowadd", rowadd, torch.float32), ("gadd", gadd, torch.float32),
                           ("gadd_index", gadd_index if gadd is not None else None, torch.int64)):
        if t is not None:
            _cuda(t, dtype, name)
    gemm_nt.last_split = _gemm(
        a3, b3, out, M=M, N=N, K=K, batch1=Z, lda=K, ldb=K, ldc=n_out, sA=(M * K, 0), sB=(N * K, 0), sC=(M * n_out, 0), alpha=alpha,
        bias=None if bias_row else bias, row_bias=bias if bias_row else None, act=_ACT[act], res=res, ldres=N, sRes=(M * N, 0),
        res_scale=res_scale, rowadd=rowadd, rowadd_period=rowadd_period, gadd=gadd, gadd_index=gadd_index, gadd_div=gadd_div,
        tile_hint=tile_hint, stream_k=split_k)
    return out


gemm_nt.last_split = False


def gemm_tn(at: torch.Tensor, bt: torch.Tensor, *, out_dtype: torch.dtype = torch.float32, alpha: float = 1.0,
            bias: torch.Tensor | None = None, stream_k: bool = False) -> torch.Tensor:
    """out[m, n] = alpha * sum_k at[k, m] * bt[k, n] (+ bias[n]); at bf16 [K, M], bt bf16 [K, N], K % 64 == 0, M and N multiples of 8
    (tribe_gemm_desc.trans_ab: the weight-gradient form dW = dY^T X without explicit transposes).  stream_k: the launcher may cut the
    last partial round of tiles over all CUs (plain f32 product only); gemm_tn.last_split tells whether it did."""
    _cuda(at, torch.bfloat16, "at")
    _cuda(bt, torch.bfloat16, "bt")
    if at.ndim != 2 or bt.ndim != 2 or at.shape[0] != bt.shape[0]:
        raise ValueError(f"gemm_tn: incompatible shapes {tuple(at.shape)} x {tuple(bt.shape)}")
    K, M = at.shape
    N = bt.shape[1]
    out = torch.empty(M, N, dtype=out_dtype, device=at.device)
    if bias is not None:
        _cuda(bias, torch.float32, "bias")
    gemm_tn.last_split = _gemm(at, bt, out, M=M, N=N, K=K, lda=M, ldb=N, ldc=N, alpha=alpha, bias=bias, trans_ab=True, stream_k=stream_k)
    return out


gemm_tn.last_split = False


# --------------------------------------------------------------------------------------
# packing
# --------------------------------------------------------------------------------------
def pack_weight(w: torch.Tensor, rows_pad: int | None = None, cols_pad: int | None = None) -> torch.Tensor:
    """f32 [rows, cols] -> bf16 [rows_pad, cols_pad] zero padded (cols padded to 64 by default: the GEMM's K step)."""
    _cuda(w, torch.float32, "w")
    rows, cols = w.shape
    rows_pad = rows if rows_pad is None else rows_pad
    cols_pad = round_up(cols, 64) if cols_pad is None else cols_pad
    out = torch.empty(rows_pad, cols_pad, dtype=torch.bfloat16, device=w.device)
    check(lib().tribe_pack_weight_bf16(w.data_ptr(), rows, cols, cols, out.data_ptr(), rows_pad, cols_pad, _stream()),
          "tribe_pack_weight_bf16")
    return out


def pack_subject_weights(w: torch.Tensor) -> torch.Tensor:
    """SubjectLayers.weights f32 [S, C, V] -> bf16 [S, V_pad, C_pad] (V_pad % 128 == 0, C_pad % 64 == 0)."""
    _cuda(w, torch.float32, "weights")
    S, Cc, V = w.shape
    V_pad, C_pad = round_up(V, 128), round_up(Cc, 64)
    out = torch.empty(S, V_pad, C_pad, dtype=torch.bfloat16, device=w.device)
    check(lib().tribe_pack_subject_weights(w.data_ptr(), S, Cc, V, out.data_ptr(), V_pad, C_pad, _stream()),
          "tribe_pack_subject_weights")
    return out


def pack_features(feat: torch.Tensor, layer_mean: bool, K_pad: int | None = None) -> torch.Tensor:
    """[B, L, D, T] or [B, D, T] (f32 / bf16 / f64) -> bf16 [B*T, K_pad] (model.py:146-155)."""
    _cuda(feat, (torch.float32, torch.bfloat16, torch.float64), "feat")
    if feat.ndim == 3:
        feat = feat[:, None]
    if feat.ndim != 4:
        raise ValueError(f"pack_features: expected [B, L, D, T] or [B, D, T], got {tuple(feat.shape)}")
    B, L, D, T = feat.shape
    K = D if layer_mean else L * D
    K_pad = round_up(K, 64) if K_pad is None else K_pad
    out = torch.empty(B * T, K_pad, dtype=torch.bfloat16, device=feat.device)
    check(lib().tribe_pack_features(feat.data_ptr(), _DT[feat.dtype], B, L, D, T, int(layer_mean), out.data_ptr(), K_pad, _stream()),
          "tribe_pack_features")
    return out


def projector_fwd(feat_packed: torch.Tensor, T: int, w_packed: torch.Tensor, bias: torch.Tensor | None, n_out: int,
                  x: torch.Tensor, col0: int, accumulate: bool, pos_embed: torch.Tensor | None,
                  subj_embed: torch.Tensor | None, subject_id: torch.Tensor | None) -> None:
    _cuda(feat_packed, torch.bfloat16, "feat_packed")
    _cuda(w_packed, torch.bfloat16, "w_packed")
    _cuda(x, torch.float32, "x")
    BT, K_pad = feat_packed.shape
    if w_packed.shape[1] != K_pad or w_packed.shape[0] < n_out:
        raise ValueError(f"projector_fwd: packed weight {tuple(w_packed.shape)} does not match K_pad={K_pad}, n_out={n_out}")
    if pos_embed is not None and (pos_embed.shape[-1] != x.shape[-1] or pos_embed.shape[-2] < T):
        raise ValueError(f"projector_fwd: time_pos_embed {tuple(pos_embed.shape)} shorter than T={T}")
    check(lib().tribe_projector_fwd(feat_packed.data_ptr(), BT, T, K_pad, w_packed.data_ptr(), _p(bias), n_out, x.data_ptr(),
                                    x.shape[-1], col0, int(accumulate), _p(pos_embed), _p(subj_embed), _p(subject_id), _stream()),
          "tribe_projector_fwd")


def projector_zero_fwd(BT: int, T: int, n_out: int, x: torch.Tensor, col0: int, pos_embed: torch.Tensor | None,
                       subj_embed: torch.Tensor | None, subject_id: torch.Tensor | None) -> None:
    _cuda(x, torch.float32, "x")
    check(lib().tribe_projector_zero_fwd(BT, T, n_out, x.data_ptr(), x.shape[-1], col0, _p(pos_embed), _p(subj_embed),
                                         _p(subject_id), _stream()), "tribe_projector_zero_fwd")


# --------------------------------------------------------------------------------------
# encoder pieces
# --------------------------------------------------------------------------------------
def _norm_params(what: str, x: torch.Tensor, w: torch.Tensor | None = None, b: torch.Tensor | None = None,
                 g: torch.Tensor | None = None) -> int:
    """Row width of a norm's input, checked against the lengths of its parameters before anything else: the kernels read dim
    weights (and biases) per row and the gain g[0], so a short vector would be an out-of-bounds read on the device."""
    for name, t in (("x", x), ("w", w), ("b", b), ("g", g)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(t)}")
    dim = x.shape[-1] if x.ndim > 0 else 0
    if dim == 0:
        raise ValueError(f"{what}: x must have a non-empty last dimension, got shape {tuple(x.shape)}")
    for name, t in (("w", w), ("b", b)):
        if t is not None and t.numel() != dim:
            raise ValueError(f"{what}: {name} must have dim={dim} elements, got shape {tuple(t.shape)}")
    if g is not None and g.numel() == 0:
        raise ValueError(f"{what}: g must hold the gain, got an empty tensor")
    return dim


def scalenorm(x: torch.Tensor, g: torch.Tensor, gain_scale: float, eps: float, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    dim = _norm_params("scalenorm", x, g=g)
    _cuda(x, torch.float32, "x")
    _cuda(g, torch.float32, "g")
    rows = x.numel() // dim
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib().tribe_scalenorm_fwd(x.data_ptr(), rows, dim, g.data_ptr(), gain_scale, eps, y.data_ptr(), _DT[out_dtype], _stream()),
          "tribe_scalenorm_fwd")
    return y


def rotary_(qkv: torch.Tensor, T: int, heads: int, dim_head: int, rot_dim: int, cos: torch.Tensor, sin: torch.Tensor,
            interleaved: bool, heads_kv: int | None = None) -> torch.Tensor:
    """In-place rotary on the q heads and k heads of a fused [rows, (heads + 2*heads_kv) * dim_head] buffer."""
    _cuda(qkv, torch.bfloat16, "qkv")
    heads_kv = heads if heads_kv is None else heads_kv
    row_stride = (heads + 2 * heads_kv) * dim_head
    rows = qkv.numel() // row_stride
    if cos.shape != (T, rot_dim // 2) or sin.shape != cos.shape:
        raise ValueError(f"rotary_: tables must be [T, rot_dim/2] = {(T, rot_dim // 2)}, got {tuple(cos.shape)}")
    check(lib().tribe_rotary_fwd(qkv.data_ptr(), rows, T, row_stride, heads + heads_kv, dim_head, rot_dim,
                                 _cuda(cos, torch.float32, "cos").data_ptr(), _cuda(sin, torch.float32, "sin").data_ptr(),
                                 int(interleaved), _stream()), "tribe_rotary_fwd")
    return qkv


def _qkv_attention(qkv: torch.Tensor, B: int, T: int, heads_q: int, heads_kv: int, dim_head: int, scale: float, *, causal: bool = False,
                   lse: torch.Tensor | None = None, rel_qe: torch.Tensor | None = None, rel_left: int = 0, rel_right: int = 0) -> torch.Tensor:
    """tribe_attention_fwd_ex on a fused bf16 [B*T, (heads_q + 2*heads_kv) * dim_head] q|k|v buffer -> bf16 [B*T, heads_q * dim_head]:
    the one place a tribe_attention_desc is filled.  lse: f32 [B, heads, T] to receive the base-2 log-sum-exp; rel_qe: f32
    [B*T, heads, stride] relative-key bias table, clamped to offsets -rel_left .. rel_right."""
    out = torch.empty(B * T, heads_q * dim_head, dtype=torch.bfloat16, device=qkv.device)
    base, width = qkv.data_ptr(), (heads_q + 2 * heads_kv) * dim_head
    d = AttentionDesc(q=base, k=base + 2 * heads_q * dim_head, v=base + 2 * (heads_q + heads_kv) * dim_head, ld_q=width, ld_k=width, ld_v=width,
                      out=out.data_ptr(), ld_out=heads_q * dim_head, B=B, T=T, heads_q=heads_q, heads_kv=heads_kv, dim_head=dim_head,
                      causal=int(causal), scale=scale, lse=_p(lse))
    if rel_qe is not None:
        d.rel_qe, d.ld_rel_qe, d.rel_stride_h, d.rel_left, d.rel_right = rel_qe.data_ptr(), heads_q * rel_qe.shape[2], rel_qe.shape[2], rel_left, rel_right
    check(lib().tribe_attention_fwd_ex(C.byref(d), _stream()), "tribe_attention_fwd_ex")
    return out


def attention_gqa(qkv: torch.Tensor, B: int, T: int, heads_q: int, heads_kv: int, dim_head: int, scale: float,
                  causal: bool) -> torch.Tensor:
    """Fused attention on a [B*T, (heads_q + 2*heads_kv) * dim_head] q|k|v buffer (grouped-query, optional causal mask)."""
    _cuda(qkv, torch.bfloat16, "qkv")
    width = (heads_q + 2 * heads_kv) * dim_head
    if qkv.numel() != B * T * width:
        raise ValueError("attention_gqa: qkv has the wrong number of elements")
    return _qkv_attention(qkv, B, T, heads_q, heads_kv, dim_head, scale, causal=causal)


def attention_relative_key(qkv: torch.Tensor, B: int, T: int, heads: int, dim_head: int, scale: float, qe: torch.Tensor,
                           left: int, right: int) -> torch.Tensor:
    """Bidirectional attention with the Wav2Vec-BERT relative_key bias (modeling_wav2vec2_bert.py:308-320):
    score[i, j] = (q_i . k_j + qe[i, h, clamp(j - i, -left, right) + left]) * scale, on a fused [B*T, 3*heads*dim_head] buffer.
    `qe` = q . E^T per query row and head, f32 [B*T, heads, stride >= left + right + 1]."""
    _cuda(qkv, torch.bfloat16, "qkv")
    _cuda(qe, torch.float32, "qe")
    if qkv.numel() != B * T * 3 * heads * dim_head or qe.dim() != 3 or qe.shape[0] != B * T or qe.shape[1] != heads:
        raise ValueError("attention_relative_key: qkv / qe have the wrong shape")
    return _qkv_attention(qkv, B, T, heads, heads, dim_head, scale, rel_qe=qe, rel_left=left, rel_right=right)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    dim = _norm_params("rmsnorm", x, w)
    _cuda(x, torch.float32, "x")
    _cuda(w, torch.float32, "w")
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib().tribe_rmsnorm_fwd(x.data_ptr(), x.numel() // dim, dim, w.data_ptr(), eps, y.data_ptr(), _DT[out_dtype], _stream()),
          "tribe_rmsnorm_fwd")
    return y


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, eps: float, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    dim = _norm_params("layernorm", x, w, b)
    _cuda(x, torch.float32, "x")
    _cuda(w, torch.float32, "w")
    if b is not None:
        _cuda(b, torch.float32, "b")
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib().tribe_layernorm_fwd(x.data_ptr(), x.numel() // dim, dim, w.data_ptr(), _p(b), eps, y.data_ptr(), _DT[out_dtype],
                                    _stream()), "tribe_layernorm_fwd")
    return y


# hidden block of an MLP: LayerNorm (optional) + activation in one row kernel each way (csrc/mlp.hip)
NORM_ACT_ACTS = {None: _lib.ACT_NONE, "gelu": _lib.ACT_GELU, "relu": _lib.ACT_RELU, "elu": _lib.ACT_ELU}
NORM_ACT_PATHS = ("reg4", "reg16", "walk4", "elem")       # tribe_norm_act_path's codes


def _row_view(t: torch.Tensor, dtype: torch.dtype | tuple[torch.dtype, ...], name: str, rows: int | None = None,
              dim: int | None = None) -> tuple[int, int, int]:
    """(rows, dim, row pitch) of a 2-D tensor whose rows are contiguous (a column slice of a wider buffer is fine)."""
    _cuda(t, dtype, name, contiguous=False)
    if t.ndim != 2 or t.shape[0] == 0 or t.shape[1] == 0 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a non-empty 2-D tensor with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    if (rows is not None and t.shape[0] != rows) or (dim is not None and t.shape[1] < dim):
        raise ValueError(f"{name}: shape {tuple(t.shape)} does not hold [{rows}, {dim}]")
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:
        raise ValueError(f"{name}: row pitch {ld} is below the row width {t.shape[1]}")
    return t.shape[0], t.shape[1], ld


def _norm_act_args(what: str, z: torch.Tensor, gamma: torch.Tensor | None, beta: torch.Tensor | None, act: str | None, norm: bool):
    if act not in NORM_ACT_ACTS:
        raise ValueError(f"{what}: activation must be one of {list(NORM_ACT_ACTS)}, got {act!r}")
    rows, dim, ld_z = _row_view(z, torch.float32, "z")
    if not norm:
        gamma = beta = None
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _cuda(t, torch.float32, name)
            if t.numel() != dim:
                raise ValueError(f"{what}: {name} must have dim={dim} elements, got shape {tuple(t.shape)}")
    return rows, dim, ld_z, gamma, beta


def norm_act(z: torch.Tensor, gamma: torch.Tensor | None, beta: torch.Tensor | None, eps: float, act: str | None, *, norm: bool = True,
             out_dtype: torch.dtype = torch.bfloat16, ld_out: int | None = None, out: torch.Tensor | None = None,
             want_stats: bool = False) -> tuple[torch.Tensor, torch.Tensor | None, torch.Tensor | None]:
    """(y, mean, rstd): y = act(LayerNorm(z)) (norm=False: act(z)) for z f32 [rows, dim] (row pitch = z.stride(0)) as f32 or bf16
    [rows, ld_out], columns >= dim zero -- ld_out defaults to dim padded to 64, the K-padded operand of the next GEMM.  `out`: write
    into this contiguous [rows, ld_out] tensor.  mean / rstd f32 [rows] with want_stats (what the backward needs), else None."""
    rows, dim, ld_z, gamma, beta = _norm_act_args("norm_act", z, gamma, beta, act, norm)
    if out is None:
        out = torch.empty(rows, round_up(dim, 64) if ld_out is None else ld_out, dtype=out_dtype, device=z.device)
    _cuda(out, (torch.float32, torch.bfloat16), "out")
    if out.ndim != 2 or out.shape[0] != rows or out.shape[1] < dim:
        raise ValueError(f"norm_act: out {tuple(out.shape)} does not hold [{rows}, >= {dim}]")
    mean = torch.empty(rows, dtype=torch.float32, device=z.device) if (want_stats and norm) else None
    rstd = torch.empty(rows, dtype=torch.float32, device=z.device) if (want_stats and norm) else None
    check(lib().tribe_norm_act_fwd(z.data_ptr(), rows, dim, ld_z, _p(gamma), _p(beta), eps, int(norm), NORM_ACT_ACTS[act], out.data_ptr(),
                                   _DT[out.dtype], out.shape[1], _p(mean), _p(rstd), _stream()), "tribe_norm_act_fwd")
    return out, mean, rstd


def norm_act_bwd(dy: torch.Tensor, z: torch.Tensor, mean: torch.Tensor | None, rstd: torch.Tensor | None, gamma: torch.Tensor | None,
                 beta: torch.Tensor | None, act: str | None, *, norm: bool = True, dz_dtype: torch.dtype = torch.float32,
                 ld_dz: int | None = None, out: torch.Tensor | None = None,
                 param_grads: bool = True) -> tuple[torch.Tensor, torch.Tensor | None, torch.Tensor | None]:
    """(dz, dgamma, dbeta) of norm_act from dy (f32 or bf16, [rows, >= dim] with contiguous rows) and the saved z, mean, rstd.
    dz f32 or bf16 [rows, ld_dz] (default dim), pad columns zero; dgamma / dbeta f32 [dim] for norm=True with param_grads."""
    rows, dim, ld_z, gamma, beta = _norm_act_args("norm_act_bwd", z, gamma, beta, act, norm)
    _, _, ld_dy = _row_view(dy, (torch.float32, torch.bfloat16), "dy", rows, dim)
    if norm:
        for name, t in (("mean", mean), ("rstd", rstd)):
            if t is None or _cuda(t, torch.float32, name).numel() != rows:
                raise ValueError(f"norm_act_bwd: {name} must be the forward's f32 [{rows}] statistics")
    if out is None:
        out = torch.empty(rows, dim if ld_dz is None else ld_dz, dtype=dz_dtype, device=z.device)
    _cuda(out, (torch.float32, torch.bfloat16), "out")
    if out.ndim != 2 or out.shape[0] != rows or out.shape[1] < dim:
        raise ValueError(f"norm_act_bwd: out {tuple(out.shape)} does not hold [{rows}, >= {dim}]")
    dgamma = dbeta = ws = None
    nbytes = 0
    if norm and param_grads:
        dgamma = torch.empty(dim, dtype=torch.float32, device=z.device)
        dbeta = torch.empty(dim, dtype=torch.float32, device=z.device)
        nbytes = lib().tribe_norm_act_bwd_workspace_bytes(rows, dim)
        ws = workspace(nbytes, z.device, tag="norm_act")
    check(lib().tribe_norm_act_bwd(dy.data_ptr(), _DT[dy.dtype], ld_dy, z.data_ptr(), rows, dim, ld_z, _p(mean) if norm else None,
                                   _p(rstd) if norm else None, _p(gamma), _p(beta), int(norm), NORM_ACT_ACTS[act], out.data_ptr(),
                                   _DT[out.dtype], out.shape[1], _p(dgamma), _p(dbeta), _p(ws), nbytes, _stream()), "tribe_norm_act_bwd")
    return out, dgamma, dbeta


def norm_act_path(z: torch.Tensor, gamma: torch.Tensor | None, beta: torch.Tensor | None, y: torch.Tensor,
                  dy: torch.Tensor | None = None) -> str:
    """Name of the row kernel the launcher picks for these tensors (y: the forward's output or the backward's dz)."""
    _, dim, ld_z = _row_view(z, torch.float32, "z")
    ld_dy = 0 if dy is None else _row_view(dy, (torch.float32, torch.bfloat16), "dy")[2]
    return NORM_ACT_PATHS[lib().tribe_norm_act_path(z.data_ptr(), dim, ld_z, _p(gamma), _p(beta), y.data_ptr(), _DT[y.dtype], y.shape[1],
                                                    _p(dy), 0 if dy is None else _DT[dy.dtype], ld_dy)]


# dropout with a counter-based mask (csrc/dropout.hip)
DROPOUT_PATHS = ("vec16", "vec8", "elem")                 # tribe_dropout_path's codes


def dropout_params(p: float) -> tuple[int, _np.float32]:
    """(threshold, scale) of tribe_dropout_apply for drop probability p: an element is kept iff its Philox word >= threshold =
    trunc(p * 2^32); kept values are multiplied by scale = float32(1 / (1 - p))."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p must satisfy 0 <= p < 1, got {p}")
    return int(p * 4294967296.0), _np.float32(1.0 / (1.0 - p))


def dropout_apply(x: torch.Tensor, p: float, seed: int, site: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """y = keep ? x * scale : +0.0 for x f32 or bf16 [rows, dim] with contiguous rows (a column slice of a wider buffer is fine: the mask
    is indexed by (row, column, dim), never by the pitch).  Element (r, c) is kept iff word (r * dim + c) & 3 of Philox4x32-10 with
    counter ((r * dim + c) >> 2, site) and key `seed` is >= trunc(p * 2^32).  A dropped NaN or negative value is +0.0 (a select, where
    torch.dropout multiplies).  `out`: same shape and dtype, rows contiguous; `out is x` works in place; None = a new contiguous
    tensor.  The backward of dropout is this call on the gradient with the same (p, seed, site).  p == 0 launches nothing: x itself
    (or `out` after a copy) comes back."""
    threshold, scale = dropout_params(p)
    rows, dim, ld_x = _row_view(x, (torch.float32, torch.bfloat16), "x")
    for name, v in (("seed", seed), ("site", site)):
        if not 0 <= int(v) < 1 << 64:
            raise ValueError(f"dropout_apply: {name} must fit 64 unsigned bits, got {v}")
    ld_y = ld_x
    if out is not None and out is not x:
        ld_y = _row_view(out, x.dtype, "out", rows, dim)[2]
        if out.shape[1] != dim:
            raise ValueError(f"dropout_apply: out {tuple(out.shape)} must have the shape of x {tuple(x.shape)}")
    if p == 0.0:
        if out is None or out is x:
            return x
        out.copy_(x)
        return out
    if out is None:
        out = torch.empty(rows, dim, dtype=x.dtype, device=x.device)
        ld_y = dim
    check(lib().tribe_dropout_apply(x.data_ptr(), out.data_ptr(), _DT[x.dtype], rows, dim, ld_x, ld_y, threshold, float(scale), int(seed),
                                    int(site), _stream()), "tribe_dropout_apply")
    return out


def dropout_path(x: torch.Tensor, out: torch.Tensor | None = None) -> str:
    """Name of the kernel tribe_dropout_apply picks for these tensors (out None: in place)."""
    _, dim, ld_x = _row_view(x, (torch.float32, torch.bfloat16), "x")
    ld_y = ld_x if out is None else _row_view(out, x.dtype, "out")[2]
    y = x if out is None else out
    return DROPOUT_PATHS[lib().tribe_dropout_path(x.data_ptr(), y.data_ptr(), _DT[x.dtype], dim, ld_x, ld_y)]


# attention dropout: the softmax row kernels with the mask drawn in registers (csrc/attn_softmax.hip)
def _mask_args(what: str, p: float, seed: int, site: int, row0: int) -> tuple[int, float, int, int, int]:
    threshold, keep = dropout_params(p)
    for name, v in (("seed", seed), ("site", site)):
        if not 0 <= int(v) < 1 << 64:
            raise ValueError(f"{what}: {name} must fit 64 unsigned bits, got {v}")
    if int(row0) < 0:
        raise ValueError(f"{what}: row0 must be >= 0, got {row0}")
    return int(row0), threshold, float(keep), int(seed), int(site)


def _softmax_rows_fwd(what: str, S: torch.Tensor, p: float, seed: int, site: int, T: int | None, row0: int, out: torch.Tensor | None,
                      lse: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
    """The body of softmax_dropout_fwd and softmax_causal_fwd: one validation, the entry point tribe_<what>."""
    rows, width, ld_s = _row_view(S, torch.float32, "S")
    T = width if T is None else int(T)
    if not 0 < T <= width:
        raise ValueError(f"{what}: T={T} outside (0, {width}]")
    mask = _mask_args(what, p, seed, site, row0)
    if out is None:
        out = torch.empty(rows, round_up(T, 64), dtype=torch.bfloat16, device=S.device)
    T_pad, ld_p = _row_view(out, torch.bfloat16, "out", rows, T)[1:]
    if lse is None:
        lse = torch.empty(rows, dtype=torch.float32, device=S.device)
    _cuda(lse, torch.float32, "lse")
    if lse.numel() != rows:
        raise ValueError(f"{what}: lse has {lse.numel()} elements for {rows} rows")
    check(getattr(lib(), "tribe_" + what)(S.data_ptr(), out.data_ptr(), lse.data_ptr(), rows, T, T_pad, ld_s, ld_p, *mask, _stream()),
          "tribe_" + what)
    return out, lse


def _softmax_rows_bwd(what: str, P: torch.Tensor, dPd: torch.Tensor, negD: torch.Tensor, scale: float, p: float, seed: int, site: int,
                      T: int | None, row0: int, dS: torch.Tensor | None, Pd: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
    """The body of softmax_dropout_bwd and softmax_causal_bwd."""
    rows, T_pad, ld_p = _row_view(P, torch.bfloat16, "P")
    width, ld_dp = _row_view(dPd, torch.float32, "dPd", rows)[1:]
    T = width if T is None else int(T)
    if not 0 < T <= min(width, T_pad):
        raise ValueError(f"{what}: T={T} outside (0, min({width}, {T_pad})]")
    mask = _mask_args(what, p, seed, site, row0)
    _cuda(negD, torch.float32, "negD")
    if negD.numel() != rows:
        raise ValueError(f"{what}: negD has {negD.numel()} elements for {rows} rows")
    if dS is None:
        dS = torch.empty(rows, T_pad, dtype=torch.bfloat16, device=P.device)
    if Pd is None:
        Pd = P
    ld_ds, ld_pd = (_row_view(t, torch.bfloat16, name, rows, T_pad)[2] for t, name in ((dS, "dS"), (Pd, "Pd")))
    if dS.shape[1] != T_pad or Pd.shape[1] != T_pad:
        raise ValueError(f"{what}: dS {tuple(dS.shape)} and Pd {tuple(Pd.shape)} must have the shape of P {tuple(P.shape)}")
    check(getattr(lib(), "tribe_" + what)(P.data_ptr(), dPd.data_ptr(), negD.data_ptr(), dS.data_ptr(), Pd.data_ptr(), rows, T, T_pad, ld_p,
                                           ld_dp, ld_ds, ld_pd, float(scale), *mask, _stream()), "tribe_" + what)
    return dS, Pd


def softmax_dropout_fwd(S: torch.Tensor, p: float, seed: int, site: int, *, T: int | None = None, row0: int = 0,
                        out: torch.Tensor | None = None, lse: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """(Pd, lse2) of attention dropout's forward (tribe_softmax_dropout_fwd): S f32 [rows, >= T] with contiguous rows holds the scaled
    scores in its leading T columns (default: all); Pd bf16 [rows, T_pad] = softmax(S) * m, m = dropout_apply's mask factor on the logical
    [row0 + rows, T] tensor (element (r, j): idx = (row0 + r) * T + j), pad columns zero; lse2 f32 [rows] = the base-2 log-sum-exp of
    attention_with_lse.  `out`: bf16 [rows, T_pad >= T], rows contiguous (default: a new tensor, T_pad = round_up(T, 64)); `lse`: f32
    [rows].  p == 0 still runs the kernel (keep everything, scale 1): Pd then has tribe_softmax_fwd's bits."""
    return _softmax_rows_fwd("softmax_dropout_fwd", S, p, seed, site, T, row0, out, lse)


def softmax_dropout_bwd(P: torch.Tensor, dPd: torch.Tensor, negD: torch.Tensor, scale: float, p: float, seed: int, site: int, *,
                        T: int | None = None, row0: int = 0, dS: torch.Tensor | None = None,
                        Pd: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """(dS, Pd) of attention dropout's backward (tribe_softmax_dropout_bwd): P bf16 [rows, T_pad] the undropped softmax, dPd f32
    [rows, >= T] = dO V^T in its leading T columns (default: all), negD f32 [rows] = -scale * rowsum(dO * O) (rowdot_heads with -scale);
    the mask is drawn again from (p, seed, site, row0).  dS bf16 [rows, T_pad] = scale * P * (m * dPd - D), Pd = bf16(P * m), pad columns of
    both zero.  `Pd` None: P is overwritten in place and handed back; `dS` None: a new tensor."""
    return _softmax_rows_bwd("softmax_dropout_bwd", P, dPd, negD, scale, p, seed, site, T, row0, dS, Pd)


def softmax_causal_fwd(S: torch.Tensor, p: float, seed: int, site: int, *, T: int | None = None, row0: int = 0,
                       out: torch.Tensor | None = None, lse: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """softmax_dropout_fwd under a causal mask (tribe_softmax_causal_fwd): row r of S is query i = (row0 + r) % T of the logical
    [B * heads * T, T] tensor.  Pd[r, j <= i] = softmax(S[r, :i + 1])[j] * m with softmax_dropout_fwd's mask m, +0.0 in every other column of
    `out` (pad columns included); lse2 = the base-2 log-sum-exp of the visible scores.  S above the diagonal is not used.  p == 0 is causal
    attention without dropout.  Same arguments, validation and defaults as softmax_dropout_fwd."""
    return _softmax_rows_fwd("softmax_causal_fwd", S, p, seed, site, T, row0, out, lse)


def softmax_causal_bwd(P: torch.Tensor, dPd: torch.Tensor, negD: torch.Tensor, scale: float, p: float, seed: int, site: int, *,
                       T: int | None = None, row0: int = 0, dS: torch.Tensor | None = None,
                       Pd: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """softmax_dropout_bwd under a causal mask (tribe_softmax_causal_bwd): for j <= i = (row0 + r) % T, dS = scale * P * (m * dPd - D) and
    Pd = bf16(P * m); +0.0 in every other column of both.  P and dPd above the diagonal are neither used nor kept: P may come from an
    ACT_EXP2 epilogue that knows no mask (and holds inf there).  Same arguments, validation and defaults as softmax_dropout_bwd."""
    return _softmax_rows_bwd("softmax_causal_bwd", P, dPd, negD, scale, p, seed, site, T, row0, dS, Pd)


def embedding(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    _cuda(table, (torch.float32, torch.bfloat16), "table")
    _cuda(ids, torch.int64, "ids")
    vocab, dim = table.shape
    x = torch.empty(ids.numel(), dim, dtype=torch.float32, device=table.device)
    check(lib().tribe_embedding_fwd(table.data_ptr(), _DT[table.dtype], ids.data_ptr(), ids.numel(), dim, vocab, x.data_ptr(), _stream()),
          "tribe_embedding_fwd")
    return x


def dwconv_ln_swish(x: torch.Tensor, B: int, T: int, w_kc: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float) -> torch.Tensor:
    """Causal depthwise Conv1d over time (left pad K - 1, no bias) + LayerNorm over channels + swish (Wav2Vec2BertConvolutionModule,
    modeling_wav2vec2_bert.py:214-222): x bf16 [B*T, C], w_kc f32 [K, C] (tap-major) -> bf16 [B*T, C]."""
    _cuda(x, torch.bfloat16, "x")
    _cuda(w_kc, torch.float32, "w_kc")
    K, Cc = w_kc.shape
    if x.shape != (B * T, Cc):
        raise ValueError(f"dwconv_ln_swish: x must be [{B * T}, {Cc}], got {tuple(x.shape)}")
    y = torch.empty_like(x)
    check(lib().tribe_dwconv_ln_swish_fwd(x.data_ptr(), B, T, Cc, K, w_kc.data_ptr(), _cuda(ln_w, torch.float32, "ln_w").data_ptr(),
                                          _cuda(ln_b, torch.float32, "ln_b").data_ptr(), eps, y.data_ptr(), _stream()), "tribe_dwconv_ln_swish_fwd")
    return y


def segment_mean(x: torch.Tensor, B: int, T: int, start: torch.Tensor | None, length: torch.Tensor | None) -> torch.Tensor:
    _cuda(x, torch.float32, "x")
    dim = x.shape[-1]
    out = torch.empty(B, dim, dtype=torch.float32, device=x.device)
    check(lib().tribe_segment_mean_fwd(x.data_ptr(), B, T, dim, _p(start), _p(length), out.data_ptr(), dim, _stream()),
          "tribe_segment_mean_fwd")
    return out


def window_mean(x: torch.Tensor, B: int, T: int, win_row: torch.Tensor, win_start: torch.Tensor, win_len: torch.Tensor) -> torch.Tensor:
    """Means over a list of windows of x f32 [B*T, dim]: out[w] = mean of rows [win_start[w], win_start[w] + win_len[w]) of sequence win_row[w]
    (int64 [W] each; windows may share a sequence, overlap or repeat) -> f32 [W, dim].  Clamped into [0, T]; an empty window or a sequence
    outside [0, B) gives zeros.  Deterministic: the same bits on every launch."""
    _cuda(x, torch.float32, "x")
    row, start, length = (_cuda(t, torch.int64, name) for t, name in ((win_row, "win_row"), (win_start, "win_start"), (win_len, "win_len")))
    dim, W = x.shape[-1], row.numel()
    if x.numel() != B * T * dim or start.numel() != W or length.numel() != W:
        raise ValueError(f"window_mean: x must hold {B * T} rows and the three window arrays one length, got {tuple(x.shape)} and "
                         f"{W} / {start.numel()} / {length.numel()}")
    out = torch.empty(W, dim, dtype=torch.float32, device=x.device)
    check(lib().tribe_window_mean_fwd(x.data_ptr(), B, T, dim, row.data_ptr(), start.data_ptr(), length.data_ptr(), W, out.data_ptr(), dim,
                                      _stream()), "tribe_window_mean_fwd")
    return out


def attention_set_mode(mode: int) -> None:
    """0 = fused kernels, picked per head size and grid (default); 1 = materialised-scores path (cross-check); 2 = the 16-row-per-wave
    kernel at every head size; 3 = dim_head 384 on the key-split kernel; 4 / 5 = dim_head 64 on the 4-wave / the anti-phase 8-wave kernel."""
    check(lib().tribe_attention_set_mode(mode), "tribe_attention_set_mode")


def encoder_set_residual_planes(on: bool) -> None:
    """True (default): encoder_fwd keeps the residual stream between its first out-proj and last FF2 as 16-bit hi / lo planes where the
    kernels allow; False: f32 stream + bf16 copy.  Process-wide."""
    check(lib().tribe_encoder_set_residual_planes(int(on)), "tribe_encoder_set_residual_planes")


def encoder_set_residual_tile_hint(hint: int) -> None:
    """tile_hint of encoder_fwd's out-proj / FF2 launches: 0 (default) or 2 (256 x 256 role kernel at any shape; tests, A/B runs)."""
    check(lib().tribe_encoder_set_residual_tile_hint(hint), "tribe_encoder_set_residual_tile_hint")


def f32_to_planes(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """f32 -> (hi, lo) int16 planes of the residual role kernels' stream format (hi = the bf16 bits); debugging and tests."""
    _cuda(x, torch.float32, "x")
    x = x.contiguous()
    hi, lo = torch.empty(x.shape, dtype=torch.int16, device=x.device), torch.empty(x.shape, dtype=torch.int16, device=x.device)
    check(lib().tribe_f32_to_planes(x.data_ptr(), x.numel(), hi.data_ptr(), lo.data_ptr(), _stream()), "tribe_f32_to_planes")
    return hi, lo


def planes_to_f32(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    _cuda(hi, torch.int16, "hi")
    _cuda(lo, torch.int16, "lo")
    if hi.shape != lo.shape or not hi.is_contiguous() or not lo.is_contiguous():
        raise ValueError("planes_to_f32: hi and lo must be contiguous and of one shape")
    x = torch.empty(hi.shape, dtype=torch.float32, device=hi.device)
    check(lib().tribe_planes_to_f32(hi.data_ptr(), lo.data_ptr(), hi.numel(), x.data_ptr(), _stream()), "tribe_planes_to_f32")
    return x


def attention(qkv: torch.Tensor, B: int, T: int, heads: int, dim_head: int, scale: float) -> torch.Tensor:
    _cuda(qkv, torch.bfloat16, "qkv")
    if qkv.numel() != B * T * 3 * heads * dim_head:
        raise ValueError("attention: qkv has the wrong number of elements")
    out = torch.empty(B * T, heads * dim_head, dtype=torch.bfloat16, device=qkv.device)
    nbytes = lib().tribe_attention_workspace_bytes(B, T, heads, dim_head)
    ws = workspace(nbytes, qkv.device)
    check(lib().tribe_attention_fwd(qkv.data_ptr(), B, T, heads, dim_head, scale, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "tribe_attention_fwd")
    return out


def attention_lse_supported(dim_head: int) -> bool:
    """True when the fused bidirectional kernel of this head size can also write the base-2 log-sum-exp of its scores (attention_with_lse)."""
    return bool(lib().tribe_attention_lse_supported(dim_head, 0))


def attention_with_lse(qkv: torch.Tensor, B: int, T: int, heads: int, dim_head: int, scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    """attention() plus lse2 [B, heads, T] f32 = log2 sum_j 2^(q.k_j * scale * log2 e): what a backward pass needs to rebuild
    P = exp2(q.k * scale * log2 e - lse2) inside a GEMM epilogue (ACT_EXP2) instead of materialising f32 scores and a softmax."""
    _cuda(qkv, torch.bfloat16, "qkv")
    inner = heads * dim_head
    if qkv.numel() != B * T * 3 * inner:
        raise ValueError("attention_with_lse: qkv has the wrong number of elements")
    lse = torch.empty(B, heads, T, dtype=torch.float32, device=qkv.device)
    return _qkv_attention(qkv, B, T, heads, heads, dim_head, scale, lse=lse), lse


def rowdot_heads(a: torch.Tensor, b: torch.Tensor, B: int, T: int, heads: int, dim_head: int, scale: float) -> torch.Tensor:
    """out[b, h, t] = scale * sum_d a[b T + t, h dh + d] * b[b T + t, h dh + d] (bf16 [B*T, heads*dim_head] inputs, f32 output)."""
    _cuda(a, torch.bfloat16, "a")
    _cuda(b, torch.bfloat16, "b")
    inner = heads * dim_head
    if a.shape != (B * T, inner) or b.shape != (B * T, inner) or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError(f"rowdot_heads: operands must be contiguous [{B * T}, {inner}]")
    out = torch.empty(B, heads, T, dtype=torch.float32, device=a.device)
    check(lib().tribe_rowdot_heads_bf16(a.data_ptr(), inner, b.data_ptr(), inner, B, T, heads, dim_head, scale, out.data_ptr(), _stream()),
          "tribe_rowdot_heads_bf16")
    return out


class EncoderPack:
    """Device-resident bf16 weights + f32 vectors of one x_transformers-style encoder, laid out for
    tribe_encoder_fwd.  Built from (and kept alive next to) the fp32 master parameters."""

    def __init__(self, dim: int, depth: int, heads: int, dim_head: int, ff_inner: int, rot_dim: int, rotary_interleaved: bool,
                 norm_gain_scale: float, norm_eps: float, causal: bool = False):
        self.causal = bool(causal)   # tribe_encoder_fwd_ex with TRIBE_ENCODER_CAUSAL
        self.dim, self.depth, self.heads, self.dim_head, self.ff_inner = dim, depth, heads, dim_head, ff_inner
        self.rot_dim, self.rotary_interleaved = rot_dim, rotary_interleaved
        self.norm_gain_scale, self.norm_eps = norm_gain_scale, norm_eps
        self.layers = (EncoderLayer * max(depth, 1))()
        self.keep: list[torch.Tensor] = []  # owns every tensor the pointer table refers to
        self.final_norm_g: torch.Tensor | None = None
        self._tabs: dict[tuple[int, int], tuple[torch.Tensor, torch.Tensor]] = {}
        self.inv_freq: torch.Tensor | None = None

    def tables(self, T: int, device: torch.device) -> tuple[torch.Tensor | None, torch.Tensor | None]:
        if self.rot_dim == 0:
            return None, None
        key = (T, device.index or 0)
        if key not in self._tabs:
            t = torch.arange(T, device=device, dtype=torch.float32)
            freqs = torch.einsum("i,j->ij", t, self.inv_freq.to(device=device, dtype=torch.float32))
            self._tabs[key] = (freqs.cos().contiguous(), freqs.sin().contiguous())
        return self._tabs[key]


def _encoder_desc(pack: EncoderPack, B: int, T: int, cos: torch.Tensor | None, sin: torch.Tensor | None) -> EncoderDesc:
    d = EncoderDesc()
    d.B, d.T = B, T
    d.dim, d.depth, d.heads, d.dim_head, d.ff_inner = pack.dim, pack.depth, pack.heads, pack.dim_head, pack.ff_inner
    d.rot_dim, d.rotary_interleaved = pack.rot_dim, int(pack.rotary_interleaved)
    d.norm_gain_scale, d.norm_eps = pack.norm_gain_scale, pack.norm_eps
    d.layers_host = C.cast(pack.layers, C.POINTER(EncoderLayer))
    d.final_norm_g = pack.final_norm_g.data_ptr()
    d.cos_tab, d.sin_tab = _p(cos), _p(sin)
    return d


def encoder_fwd(x: torch.Tensor, pack: EncoderPack, B: int, T: int, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """x f32 [B*T, dim] is consumed (updated in place); returns final-normed y [B*T, dim]."""
    _cuda(x, torch.float32, "x")
    if x.shape != (B * T, pack.dim):
        raise ValueError(f"encoder_fwd: x must be [{B * T}, {pack.dim}], got {tuple(x.shape)}")
    d = _encoder_desc(pack, B, T, *pack.tables(T, x.device))
    y = torch.empty(B * T, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_workspace_bytes(C.byref(d))
    ws = workspace(nbytes, x.device)
    if pack.causal:
        check(lib().tribe_encoder_fwd_ex(C.byref(d), _lib.ENCODER_CAUSAL, x.data_ptr(), y.data_ptr(), _DT[out_dtype], ws.data_ptr(), ws.numel(),
                                         _stream()), "tribe_encoder_fwd_ex")
        return y
    check(lib().tribe_encoder_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], ws.data_ptr(), ws.numel(), _stream()),
          "tribe_encoder_fwd")
    return y


# --------------------------------------------------------------------------------------
# streaming a causal encoder: KV cache, single-query attention, one-position encoder step
# --------------------------------------------------------------------------------------
DECODE_DIM_HEADS = (64, 128, 192, 384)


def _kv_caches(what: str, k_cache: torch.Tensor, v_cache: torch.Tensor, ndim: int) -> tuple[int, ...]:
    """Shape of a K / V cache pair ([B, heads, cap, dim_head], or with a leading depth), checked before any device work."""
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(t)}")
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{what}: {name} must be bfloat16, got {t.dtype}")
        if t.ndim != ndim or not t.is_contiguous():
            lead = "depth, " if ndim == 5 else ""
            raise ValueError(f"{what}: {name} must be a contiguous [{lead}B, heads, cap, dim_head] tensor, got shape {tuple(t.shape)}")
    if k_cache.shape != v_cache.shape or k_cache.device != v_cache.device:
        raise ValueError(f"{what}: k_cache {tuple(k_cache.shape)} on {k_cache.device} and v_cache {tuple(v_cache.shape)} on {v_cache.device} differ")
    return tuple(k_cache.shape)


def _step_rows(what: str, t: torch.Tensor, name: str, dtype: torch.dtype, B: int, min_width: int, device: torch.device) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(t)}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if t.ndim != 2 or t.shape[0] != B or t.shape[1] < min_width or t.stride(1) != 1:
        raise ValueError(f"{what}: {name} must be [B={B}, >= {min_width}] with unit column stride, got shape {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device}, the caches on {device}")


def kv_append(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int, rot_dim: int, cos: torch.Tensor | None,
              sin: torch.Tensor | None, interleaved: bool) -> torch.Tensor:
    """tribe_kv_append: rotates the q and k heads of the step's fused bf16 qkv [B, 3*heads*dim_head] in place at position `pos`
    (ops.rotary_'s bits; cos / sin f32 [> pos, rot_dim/2], unused at rot_dim == 0) and stores the rotated k heads and the v heads into slot
    `pos` of the bf16 caches [B, heads, cap, dim_head].  Returns qkv."""
    what = "tribe_kv_append"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    _step_rows(what, qkv, "qkv", torch.bfloat16, B, 3 * heads * dim_head, k_cache.device)
    if qkv.shape[1] != 3 * heads * dim_head or not qkv.is_contiguous():
        raise ValueError(f"{what}: qkv must be contiguous [B={B}, 3*heads*dim_head={3 * heads * dim_head}], got shape {tuple(qkv.shape)}")
    if not 0 <= pos < cap:
        raise ValueError(f"{what}: pos={pos} outside the cache capacity {cap}")
    if rot_dim:
        for name, t in (("cos", cos), ("sin", sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != rot_dim // 2 or t.shape[0] <= pos \
                    or not t.is_contiguous() or t.device != k_cache.device:
                raise ValueError(f"{what}: {name} must be a contiguous f32 [> pos={pos}, rot_dim/2={rot_dim // 2}] table on {k_cache.device}")
    _cuda(qkv, torch.bfloat16, "qkv")
    check(lib().tribe_kv_append(qkv.data_ptr(), B, heads, dim_head, rot_dim, int(interleaved), _p(cos) if rot_dim else None,
                                _p(sin) if rot_dim else None, pos, k_cache.data_ptr(), v_cache.data_ptr(), cap, _stream()), what)
    return qkv


def attention_decode_splits(B: int, heads: int, n: int) -> int:
    """Workgroups the keys of one (sequence, head) are split over (tribe_attention_decode_splits): a function of B, heads and n alone."""
    return int(lib().tribe_attention_decode_splits(B, heads, n))


def attention_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n: int, scale: float) -> torch.Tensor:
    """tribe_attention_decode_fwd: one query row per (sequence, head) against the first n slots of the bf16 caches [B, heads, cap, dim_head]:
    softmax(scale q K[0:n]^T) V[0:n] -> bf16 [B, heads*dim_head].  q: bf16 [B, >= heads*dim_head] rows whose first heads*dim_head columns
    are the (rotated) q heads -- the fused qkv buffer of the step serves as it is."""
    what = "tribe_attention_decode_fwd"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    if dim_head not in DECODE_DIM_HEADS:
        raise ValueError(f"{what}: dim_head={dim_head} must be one of {DECODE_DIM_HEADS}")
    _step_rows(what, q, "q", torch.bfloat16, B, heads * dim_head, k_cache.device)
    if not 1 <= n <= cap:
        raise ValueError(f"{what}: n={n} keys outside 1 .. capacity {cap}")
    _cuda(q, torch.bfloat16, "q", contiguous=False)
    out = torch.empty(B, heads * dim_head, dtype=torch.bfloat16, device=q.device)
    nbytes = lib().tribe_attention_decode_workspace_bytes(B, heads, dim_head, n)
    ws = workspace(nbytes, q.device, tag="decode")
    check(lib().tribe_attention_decode_fwd(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), B, heads, dim_head, cap, n, scale,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), what)
    return out


def _encoder_caches(what: str, pack: EncoderPack, x: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor) -> tuple[int, int]:
    depth, B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 5)
    if (depth, heads, dim_head) != (pack.depth, pack.heads, pack.dim_head):
        raise ValueError(f"{what}: caches {tuple(k_cache.shape)} do not match depth={pack.depth}, heads={pack.heads}, dim_head={pack.dim_head}")
    if not pack.causal:
        raise ValueError(f"{what}: the encoder is bidirectional (causal=False): it has no incremental form")
    if dim_head not in DECODE_DIM_HEADS:
        raise ValueError(f"{what}: dim_head={dim_head} must be one of {DECODE_DIM_HEADS}")
    return B, cap


def encoder_step(x: torch.Tensor, pack: EncoderPack, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int,
                 out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """tribe_encoder_step_fwd: the causal encoder at position `pos`.  x f32 [B, dim] is consumed; the bf16 caches
    [depth, B, heads, cap, dim_head] hold positions 0 .. pos-1 and receive slot pos; returns final-normed y [B, dim]."""
    what = "tribe_encoder_step_fwd"
    B, cap = _encoder_caches(what, pack, x, k_cache, v_cache)
    _step_rows(what, x, "x", torch.float32, B, pack.dim, k_cache.device)
    if x.shape[1] != pack.dim or not x.is_contiguous():
        raise ValueError(f"{what}: x must be contiguous [B={B}, dim={pack.dim}], got shape {tuple(x.shape)}")
    if not 0 <= pos < cap:
        raise ValueError(f"{what}: pos={pos} outside the cache capacity {cap}")
    _cuda(x, torch.float32, "x")
    d = _encoder_desc(pack, B, 1, *pack.tables(cap, x.device))
    y = torch.empty(B, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_step_workspace_bytes(C.byref(d), cap)
    ws = workspace(nbytes, x.device)
    check(lib().tribe_encoder_step_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], k_cache.data_ptr(), v_cache.data_ptr(), cap, pos,
                                       ws.data_ptr(), ws.numel(), _stream()), what)
    return y


def encoder_prefill(x: torch.Tensor, pack: EncoderPack, k_cache: torch.Tensor, v_cache: torch.Tensor, T: int,
                    out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """tribe_encoder_prefill_fwd: the causal forward over T positions from an empty cache, which also fills slots 0 .. T-1 of the caches.
    x f32 [B*T, dim] is consumed; returns final-normed y [B*T, dim]."""
    what = "tribe_encoder_prefill_fwd"
    B, cap = _encoder_caches(what, pack, x, k_cache, v_cache)
    if not 1 <= T <= cap:
        raise ValueError(f"{what}: T={T} positions do not fit the cache capacity {cap}")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.shape != (B * T, pack.dim) or not x.is_contiguous():
        raise ValueError(f"{what}: x must be a contiguous f32 [B*T={B * T}, dim={pack.dim}] tensor")
    if x.device != k_cache.device:
        raise ValueError(f"{what}: x is on {x.device}, the caches on {k_cache.device}")
    _cuda(x, torch.float32, "x")
    d = _encoder_desc(pack, B, T, *pack.tables(T, x.device))
    y = torch.empty(B * T, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_workspace_bytes(C.byref(d))
    ws = workspace(nbytes, x.device)
    check(lib().tribe_encoder_prefill_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], k_cache.data_ptr(), v_cache.data_ptr(), cap,
                                          ws.data_ptr(), ws.numel(), _stream()), what)
    return y


# ---- block append: k positions at once onto a cache that holds `pos` ----
def _block_rows(what: str, t: torch.Tensor, name: str, dtype: torch.dtype, B: int, k: int, width: int, exact: bool, device: torch.device) -> None:
    """A block's rows [B*k, width] (row b*k + t = step t of sequence b), checked before any device work."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(t)}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if t.ndim != 2 or t.shape[0] != B * k or t.stride(1) != 1 or (t.shape[1] != width if exact else t.shape[1] < width) \
            or (exact and not t.is_contiguous()):
        shape = f"contiguous [B*k={B * k}, {width}]" if exact else f"[B*k={B * k}, >= {width}] with unit column stride"
        raise ValueError(f"{what}: {name} must be {shape}, got shape {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device}, the caches on {device}")


def _block_range(what: str, pos: int, k: int, cap: int) -> None:
    if k < 1:
        raise ValueError(f"{what}: k={k} must be at least 1")
    if pos < 0 or pos + k > cap:
        raise ValueError(f"{what}: positions pos={pos} .. pos+k={pos + k} outside the cache capacity {cap}")


def kv_append_block(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int, k: int, rot_dim: int, cos: torch.Tensor | None,
                    sin: torch.Tensor | None, interleaved: bool) -> torch.Tensor:
    """tribe_kv_append_block: kv_append for k rows per sequence.  Rotates the q and k heads of the fused bf16 qkv [B*k, 3*heads*dim_head] in
    place, row b*k + t at position pos + t (ops.rotary_'s bits; cos / sin f32 [>= pos+k, rot_dim/2], unused at rot_dim == 0), and stores the
    rotated k heads and the v heads into slots pos .. pos+k-1 of the bf16 caches [B, heads, cap, dim_head].  Returns qkv."""
    what = "tribe_kv_append_block"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    _block_range(what, pos, k, cap)
    _block_rows(what, qkv, "qkv", torch.bfloat16, B, k, 3 * heads * dim_head, True, k_cache.device)
    if rot_dim:
        for name, t in (("cos", cos), ("sin", sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != rot_dim // 2 or t.shape[0] < pos + k \
                    or not t.is_contiguous() or t.device != k_cache.device:
                raise ValueError(f"{what}: {name} must be a contiguous f32 [>= pos+k={pos + k}, rot_dim/2={rot_dim // 2}] table on {k_cache.device}")
    _cuda(qkv, torch.bfloat16, "qkv")
    check(lib().tribe_kv_append_block(qkv.data_ptr(), B, k, heads, dim_head, rot_dim, int(interleaved), _p(cos) if rot_dim else None,
                                      _p(sin) if rot_dim else None, pos, k_cache.data_ptr(), v_cache.data_ptr(), cap, _stream()), what)
    return qkv


def attention_extend(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int, k: int, scale: float) -> torch.Tensor:
    """tribe_attention_extend_fwd: k query rows per (sequence, head) at positions pos .. pos+k-1 against the first pos+k slots of the bf16
    caches [B, heads, cap, dim_head], query t under the mask key <= pos + t -> bf16 [B*k, heads*dim_head].  q: bf16 [B*k, >= heads*dim_head]
    rows (row b*k + t) whose first heads*dim_head columns are the rotated q heads -- the block's fused qkv buffer serves as it is.  The
    caches must already hold the block's own slots (kv_append_block)."""
    what = "tribe_attention_extend_fwd"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    if dim_head not in DECODE_DIM_HEADS:
        raise ValueError(f"{what}: dim_head={dim_head} must be one of {DECODE_DIM_HEADS}")
    _block_range(what, pos, k, cap)
    _block_rows(what, q, "q", torch.bfloat16, B, k, heads * dim_head, False, k_cache.device)
    _cuda(q, torch.bfloat16, "q", contiguous=False)
    out = torch.empty(B * k, heads * dim_head, dtype=torch.bfloat16, device=q.device)
    check(lib().tribe_attention_extend_fwd(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), B, heads, dim_head, cap, pos, k,
                                           scale, out.data_ptr(), _stream()), what)
    return out


def encoder_extend(x: torch.Tensor, pack: EncoderPack, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int, k: int,
                   out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """tribe_encoder_extend_fwd: the causal encoder at positions pos .. pos+k-1.  x f32 [B*k, dim] (row b*k + t) is consumed; the bf16
    caches [depth, B, heads, cap, dim_head] hold positions 0 .. pos-1 and receive slots pos .. pos+k-1; returns final-normed y [B*k, dim]."""
    what = "tribe_encoder_extend_fwd"
    B, cap = _encoder_caches(what, pack, x, k_cache, v_cache)
    _block_range(what, pos, k, cap)
    _block_rows(what, x, "x", torch.float32, B, k, pack.dim, True, k_cache.device)
    _cuda(x, torch.float32, "x")
    d = _encoder_desc(pack, B, k, *pack.tables(cap, x.device))
    y = torch.empty(B * k, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_extend_workspace_bytes(C.byref(d), cap)
    ws = workspace(nbytes, x.device)
    check(lib().tribe_encoder_extend_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], k_cache.data_ptr(), v_cache.data_ptr(), cap, pos,
                                         ws.data_ptr(), ws.numel(), _stream()), what)
    return y


# ---- slots: every sequence of a cache at a position of its own ----
def _slot_positions(what: str, pos: tp.Sequence[int], B: int, k: int, cap: int) -> list[int]:
    """The host copy of a call's positions, checked before any launch: one int per sequence, -1 (takes no part) or 0 .. cap - k."""
    if isinstance(pos, torch.Tensor) or not isinstance(pos, (list, tuple)):
        raise TypeError(f"{what}: pos must be a list or tuple of ints (the wrapper builds the device array), got {type(pos)}")
    if len(pos) != B:
        raise ValueError(f"{what}: pos holds {len(pos)} positions for B={B} sequences")
    if k < 1:
        raise ValueError(f"{what}: k={k} must be at least 1")
    out = []
    for b, p in enumerate(pos):
        if isinstance(p, bool) or not isinstance(p, int):
            raise TypeError(f"{what}: pos[{b}] must be an int, got {type(p)}")
        if p != -1 and not 0 <= p <= cap - k:
            raise ValueError(f"{what}: pos[{b}]={p} .. +k={p + k} outside the cache capacity {cap} (-1 marks a sequence that takes no part)")
        out.append(p)
    return out


def _slot_array(pos: list[int], device: torch.device) -> torch.Tensor:
    """int32 [B] on the device.  Staged through pinned memory and copied on the current stream: the host does not wait for the device."""
    return torch.tensor(pos, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def _slot_tables(what: str, rot_dim: int, cos: torch.Tensor | None, sin: torch.Tensor | None, cap: int, device: torch.device) -> None:
    if rot_dim:
        for name, t in (("cos", cos), ("sin", sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != rot_dim // 2 or t.shape[0] < cap \
                    or not t.is_contiguous() or t.device != device:
                raise ValueError(f"{what}: {name} must be a contiguous f32 [>= cap={cap}, rot_dim/2={rot_dim // 2}] table on {device}")


def kv_append_slots(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: tp.Sequence[int], k: int, rot_dim: int,
                    cos: torch.Tensor | None, sin: torch.Tensor | None, interleaved: bool) -> torch.Tensor:
    """tribe_kv_append_slots: kv_append_block with a position per sequence.  Row b*k + t of the fused bf16 qkv [B*k, 3*heads*dim_head] is
    rotated in place at position pos[b] + t and stored into slot pos[b] + t of sequence b (cos / sin f32 [>= cap, rot_dim/2]); pos[b] == -1:
    neither the rows nor the cache run of sequence b are touched.  Returns qkv."""
    what = "tribe_kv_append_slots"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    pos = _slot_positions(what, pos, B, k, cap)
    _block_rows(what, qkv, "qkv", torch.bfloat16, B, k, 3 * heads * dim_head, True, k_cache.device)
    _slot_tables(what, rot_dim, cos, sin, cap, k_cache.device)
    _cuda(qkv, torch.bfloat16, "qkv")
    dpos = _slot_array(pos, qkv.device)
    check(lib().tribe_kv_append_slots(qkv.data_ptr(), B, k, heads, dim_head, rot_dim, int(interleaved), _p(cos) if rot_dim else None,
                                      _p(sin) if rot_dim else None, dpos.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), cap, _stream()),
          what)
    return qkv


def attention_decode_slots(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: tp.Sequence[int], n_max: int,
                           scale: float) -> torch.Tensor:
    """tribe_attention_decode_slots_fwd: attention_decode with n_b = pos[b] + 1 keys for sequence b (pos[b] == -1: takes no part, its row
    comes back as zeros); n_max bounds every n_b and fixes the key split (attention_decode_splits(B, heads, n_max)) -> bf16 [B, heads*dim_head]."""
    what = "tribe_attention_decode_slots_fwd"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    if dim_head not in DECODE_DIM_HEADS:
        raise ValueError(f"{what}: dim_head={dim_head} must be one of {DECODE_DIM_HEADS}")
    _step_rows(what, q, "q", torch.bfloat16, B, heads * dim_head, k_cache.device)
    pos = _slot_positions(what, pos, B, 1, cap)
    if not 1 <= n_max <= cap:
        raise ValueError(f"{what}: n_max={n_max} keys outside 1 .. capacity {cap}")
    if max(pos) + 1 > n_max:
        raise ValueError(f"{what}: n_max={n_max} is no upper bound of the key counts pos[b] + 1 (largest: {max(pos) + 1})")
    _cuda(q, torch.bfloat16, "q", contiguous=False)
    dpos = _slot_array(pos, q.device)
    out = torch.empty(B, heads * dim_head, dtype=torch.bfloat16, device=q.device)
    nbytes = lib().tribe_attention_decode_workspace_bytes(B, heads, dim_head, n_max)
    ws = workspace(nbytes, q.device, tag="decode")
    check(lib().tribe_attention_decode_slots_fwd(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), B, heads, dim_head, cap,
                                                 dpos.data_ptr(), n_max, scale, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), what)
    return out


def attention_extend_slots(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: tp.Sequence[int], k: int,
                           scale: float) -> torch.Tensor:
    """tribe_attention_extend_slots_fwd: attention_extend with the k query rows of sequence b at positions pos[b] .. pos[b]+k-1 against its
    first pos[b]+k slots (kv_append_slots first); pos[b] == -1: takes no part, its rows come back as zeros -> bf16 [B*k, heads*dim_head]."""
    what = "tribe_attention_extend_slots_fwd"
    B, heads, cap, dim_head = _kv_caches(what, k_cache, v_cache, 4)
    if dim_head not in DECODE_DIM_HEADS:
        raise ValueError(f"{what}: dim_head={dim_head} must be one of {DECODE_DIM_HEADS}")
    pos = _slot_positions(what, pos, B, k, cap)
    _block_rows(what, q, "q", torch.bfloat16, B, k, heads * dim_head, False, k_cache.device)
    _cuda(q, torch.bfloat16, "q", contiguous=False)
    dpos = _slot_array(pos, q.device)
    out = torch.empty(B * k, heads * dim_head, dtype=torch.bfloat16, device=q.device)
    check(lib().tribe_attention_extend_slots_fwd(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), B, heads, dim_head, cap,
                                                 dpos.data_ptr(), k, scale, out.data_ptr(), _stream()), what)
    return out


def encoder_step_slots(x: torch.Tensor, pack: EncoderPack, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: tp.Sequence[int],
                       out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """tribe_encoder_step_slots_fwd: encoder_step with sequence b at position pos[b] (-1: takes no part; its row still runs through the norms
    and GEMMs -- pass finite values -- and its output row is to be discarded).  x f32 [B, dim] is consumed; returns final-normed y [B, dim].
    No host-device synchronisation: the positions travel as a pinned int32 array on the current stream."""
    what = "tribe_encoder_step_slots_fwd"
    B, cap = _encoder_caches(what, pack, x, k_cache, v_cache)
    _step_rows(what, x, "x", torch.float32, B, pack.dim, k_cache.device)
    if x.shape[1] != pack.dim or not x.is_contiguous():
        raise ValueError(f"{what}: x must be contiguous [B={B}, dim={pack.dim}], got shape {tuple(x.shape)}")
    pos = _slot_positions(what, pos, B, 1, cap)
    _cuda(x, torch.float32, "x")
    dpos = _slot_array(pos, x.device)
    d = _encoder_desc(pack, B, 1, *pack.tables(cap, x.device))
    y = torch.empty(B, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_step_workspace_bytes(C.byref(d), cap)
    ws = workspace(nbytes, x.device)
    check(lib().tribe_encoder_step_slots_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], k_cache.data_ptr(), v_cache.data_ptr(), cap,
                                             dpos.data_ptr(), max(max(pos) + 1, 1), ws.data_ptr(), ws.numel(), _stream()), what)
    return y


def encoder_extend_slots(x: torch.Tensor, pack: EncoderPack, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: tp.Sequence[int], k: int,
                         out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """tribe_encoder_extend_slots_fwd: encoder_extend with the k rows of sequence b at positions pos[b] .. pos[b]+k-1 (-1: takes no part, as in
    encoder_step_slots).  x f32 [B*k, dim] (row b*k + t) is consumed; returns final-normed y [B*k, dim]."""
    what = "tribe_encoder_extend_slots_fwd"
    B, cap = _encoder_caches(what, pack, x, k_cache, v_cache)
    pos = _slot_positions(what, pos, B, k, cap)
    _block_rows(what, x, "x", torch.float32, B, k, pack.dim, True, k_cache.device)
    _cuda(x, torch.float32, "x")
    dpos = _slot_array(pos, x.device)
    d = _encoder_desc(pack, B, k, *pack.tables(cap, x.device))
    y = torch.empty(B * k, pack.dim, dtype=out_dtype, device=x.device)
    nbytes = lib().tribe_encoder_extend_workspace_bytes(C.byref(d), cap)
    ws = workspace(nbytes, x.device)
    check(lib().tribe_encoder_extend_slots_fwd(C.byref(d), x.data_ptr(), y.data_ptr(), _DT[out_dtype], k_cache.data_ptr(), v_cache.data_ptr(),
                                               cap, dpos.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), what)
    return y


# --------------------------------------------------------------------------------------
# voxel head, pool, losses
# --------------------------------------------------------------------------------------
def voxel_head(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, subjects: torch.Tensor, V: int) -> torch.Tensor:
    """x bf16 [B, T, C_pad]; returns f32 [B, V, T] (SubjectLayers.forward, common.py:45-67)."""
    _cuda(x, torch.bfloat16, "x")
    _cuda(w_packed, torch.bfloat16, "w_packed")
    _cuda(subjects, torch.int64, "subjects")
    B, T, C_pad = x.shape
    S, V_pad, C_pad2 = w_packed.shape
    if C_pad != C_pad2 or subjects.numel() != B:
        raise ValueError(f"voxel_head: x {tuple(x.shape)} / weights {tuple(w_packed.shape)} / subjects {tuple(subjects.shape)} mismatch")
    y = torch.empty(B, V, T, dtype=torch.float32, device=x.device)
    check(lib().tribe_voxel_head_fwd(x.data_ptr(), B, T, C_pad, w_packed.data_ptr(), S, V, V_pad, _p(bias), subjects.data_ptr(),
                                     y.data_ptr(), _stream()), "tribe_voxel_head_fwd")
    return y


def adaptive_avg_pool(x: torch.Tensor, t_out: int) -> torch.Tensor:
    _cuda(x, torch.float32, "x")
    t_in = x.shape[-1]
    rows = x.numel() // t_in
    y = torch.empty(*x.shape[:-1], t_out, dtype=torch.float32, device=x.device)
    check(lib().tribe_adaptive_avg_pool_fwd(x.data_ptr(), rows, t_in, y.data_ptr(), t_out, _stream()), "tribe_adaptive_avg_pool_fwd")
    return y


ELEM_LOSS_KINDS = {"l1": 0, "smooth_l1": 1, "huber": 2, "mse": 3}        # enum tribe_loss_kind
ELEM_LOSS_REDUCTIONS = {"mean": 0, "sum": 1}                             # enum tribe_loss_reduction


def elem_loss(pred: torch.Tensor, true: torch.Tensor, kind: str, param: float = 1.0, reduction: str = "mean") -> torch.Tensor:
    """nn.L1Loss / SmoothL1Loss(beta=param) / HuberLoss(delta=param) / MSELoss over all elements of two equal-shape contiguous f32 tensors
    (f32 scalar).  The element order does not matter, so a [B, V, T'] pair is read in place."""
    _cuda(pred, torch.float32, "pred")
    _cuda(true, torch.float32, "true")
    if pred.shape != true.shape:
        raise ValueError(f"elem_loss: shape mismatch {tuple(pred.shape)} vs {tuple(true.shape)}")
    if kind not in ELEM_LOSS_KINDS:
        raise ValueError(f"elem_loss: kind must be one of {sorted(ELEM_LOSS_KINDS)}, got {kind!r}")
    if reduction not in ELEM_LOSS_REDUCTIONS:
        raise ValueError(f"elem_loss: reduction must be 'mean' or 'sum', got {reduction!r}")
    n = pred.numel()
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = workspace(lib().tribe_elem_loss_workspace_bytes(n), pred.device, "loss")
    check(lib().tribe_elem_loss_fwd(pred.data_ptr(), true.data_ptr(), n, ELEM_LOSS_KINDS[kind], float(param), ELEM_LOSS_REDUCTIONS[reduction],
                                    out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "tribe_elem_loss_fwd")
    return out


def _bvt_strides(pred: torch.Tensor, true: torch.Tensor, what: str) -> tuple[int, int, int, int, int, int]:
    """Accept any strided 3-D [B, V, T] view (e.g. the transpose of a '(b t) d' matrix) -- no copy is made."""
    if pred.shape != true.shape or pred.ndim != 3:
        raise ValueError(f"{what}: expected equal [B, V, T] shapes, got {tuple(pred.shape)} / {tuple(true.shape)}")
    if pred.stride() != true.stride():
        raise ValueError(f"{what}: pred and true must share strides, got {pred.stride()} / {true.stride()}")
    B, V, T = pred.shape
    sb, sv, st = pred.stride()
    return B, V, T, sb, sv, st


def _bvt_stats_update(what: str, stats: torch.Tensor, pred: torch.Tensor, true: torch.Tensor, group: torch.Tensor | None) -> None:
    """The checks and the C call of `what` = pearson_stats_update / regression_stats_update (csrc/bvt_stats.h: one kernel pair)."""
    _cuda(stats, torch.float64, "stats")
    _cuda(pred, torch.float32, "pred", contiguous=False)
    _cuda(true, torch.float32, "true", contiguous=False)
    B, V, T, sb, sv, st = _bvt_strides(pred, true, what)
    G = stats.shape[0]
    if stats.shape != (G, V, 6):
        raise ValueError(f"{what}: stats must be [G, {V}, 6], got {tuple(stats.shape)}")
    if group is not None:
        _cuda(group, torch.int64, "group")
        if group.numel() != B:
            raise ValueError(f"{what}: group must have B entries")
    check(getattr(lib(), f"tribe_{what}")(pred.data_ptr(), true.data_ptr(), B, V, T, sb, sv, st, _p(group), G, stats.data_ptr(), _stream()),
          f"tribe_{what}")


def pearson_stats_update(stats: torch.Tensor, pred: torch.Tensor, true: torch.Tensor, group: torch.Tensor | None = None) -> None:
    """stats f64 [G, V, 6] += sufficient statistics of pred/true [B, V, T]; group int64 [B] or None."""
    _bvt_stats_update("pearson_stats_update", stats, pred, true, group)


def pearson_from_stats(stats: torch.Tensor) -> torch.Tensor:
    _cuda(stats, torch.float64, "stats")
    G, V, _ = stats.shape
    r = torch.empty(G, V, dtype=torch.float32, device=stats.device)
    check(lib().tribe_pearson_from_stats(stats.data_ptr(), G, V, r.data_ptr(), _stream()), "tribe_pearson_from_stats")
    return r


def pearson_loss(pred: torch.Tensor, true: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """PearsonLoss over the '(b t) d' view of [B, V, T] tensors (losses.py:17-42); any strided view is accepted."""
    _cuda(pred, torch.float32, "pred", contiguous=False)
    _cuda(true, torch.float32, "true", contiguous=False)
    if reduction not in ("mean", "sum"):
        raise ValueError(f"Invalid reduction: {reduction}")
    B, V, T, sb, sv, st = _bvt_strides(pred, true, "pearson_loss")
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = workspace(lib().tribe_pearson_loss_workspace_bytes(V), pred.device, "loss")
    check(lib().tribe_pearson_loss_fwd(pred.data_ptr(), true.data_ptr(), B, V, T, sb, sv, st, int(reduction == "sum"),
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "tribe_pearson_loss_fwd")
    return out


# --------------------------------------------------------------------------------------
# regression metrics MSE / RMSE / MAE / R2 / explained variance (csrc/regression_metrics.hip)
# --------------------------------------------------------------------------------------
REGRESSION_KINDS = {"mse": 0, "rmse": 1, "mae": 2, "r2": 3, "explained_variance": 4}     # enum tribe_regression_kind
REGRESSION_MODES = {"pooled": 0, "uniform_average": 1, "variance_weighted": 2}           # enum tribe_regression_mode


def regression_stats_update(stats: torch.Tensor, pred: torch.Tensor, true: torch.Tensor, group: torch.Tensor | None = None) -> None:
    """stats f64 [G, V, 6] += {sum d, sum d^2, sum |d|, sum t, sum t^2, n} of d = true - pred over [B, V, T] views (any common
    strides); group int64 [B] or None."""
    _bvt_stats_update("regression_stats_update", stats, pred, true, group)


def _regression_stats(stats: torch.Tensor, kind: str, what: str) -> tuple[int, int]:
    _cuda(stats, torch.float64, "stats")
    if stats.ndim != 3 or stats.shape[2] != 6:
        raise ValueError(f"{what}: stats must be [G, V, 6], got {tuple(stats.shape)}")
    if kind not in REGRESSION_KINDS:
        raise ValueError(f"{what}: kind must be one of {sorted(REGRESSION_KINDS)}, got {kind!r}")
    return stats.shape[0], stats.shape[1]


def regression_from_stats(stats: torch.Tensor, kind: str) -> torch.Tensor:
    """Raw per-output scores f32 [G, V] of the statistics (computed in f64, rounded once)."""
    G, V = _regression_stats(stats, kind, "regression_from_stats")
    out = torch.empty(G, V, dtype=torch.float32, device=stats.device)
    check(lib().tribe_regression_from_stats(stats.data_ptr(), G, V, REGRESSION_KINDS[kind], out.data_ptr(), _stream()),
          "tribe_regression_from_stats")
    return out


def regression_reduce(stats: torch.Tensor, kind: str, mode: str) -> torch.Tensor:
    """One f64 score per group [G]: 'pooled' (mse / rmse / mae over every element), 'uniform_average' or 'variance_weighted' over the
    outputs.  The sums run in a fixed order: equal statistics give equal bits."""
    G, V = _regression_stats(stats, kind, "regression_reduce")
    if mode not in REGRESSION_MODES:
        raise ValueError(f"regression_reduce: mode must be one of {sorted(REGRESSION_MODES)}, got {mode!r}")
    if mode == "pooled" and kind not in ("mse", "rmse", "mae"):
        raise ValueError(f"regression_reduce: 'pooled' is defined for mse, rmse and mae, not {kind!r}")
    out = torch.empty(G, dtype=torch.float64, device=stats.device)
    check(lib().tribe_regression_reduce(stats.data_ptr(), G, V, REGRESSION_KINDS[kind], REGRESSION_MODES[mode], out.data_ptr(), _stream()),
          "tribe_regression_reduce")
    return out


# --------------------------------------------------------------------------------------
# retrieval metrics Rank / TopkAcc (csrc/metrics.hip)
# --------------------------------------------------------------------------------------
_NORM_KINDS = {None: 0, "x": 1, "y": 2, "xy": 3}


def _nvt(x: torch.Tensor, what: str) -> torch.Tensor:
    """[N, V] -> [N, V, 1] view (T = 1); [N, V, T] as is."""
    if x.ndim == 2:
        return x.unsqueeze(-1)
    if x.ndim != 3:
        raise ValueError(f"{what}: expected [N, V] or [N, V, T], got {tuple(x.shape)}")
    return x


def retrieval_prep(x: torch.Tensor, y: torch.Tensor | None = None, *, mean: bool = True, norm_x: bool = False,
                   norm_y: bool = False) -> tuple[torch.Tensor | None, torch.Tensor | None, torch.Tensor | None, torch.Tensor | None]:
    """Strided f32 [N, V, T] views (or [N, V]) -> (x_mean [N, V], y_mean, x_norm [N], y_norm): means over T and the L2 norms of
    the mean rows, in one launch for both tensors (y: same shape and strides as x).  Outputs not asked for are None."""
    _cuda(x, torch.float32, "x", contiguous=False)
    x3 = _nvt(x, "retrieval_prep")
    if y is not None:
        _cuda(y, torch.float32, "y", contiguous=False)
        N, V, T, sn, sv, st = _bvt_strides(x3, _nvt(y, "retrieval_prep"), "retrieval_prep")
    else:
        N, V, T = x3.shape
        sn, sv, st = x3.stride()
    if N == 0 or V == 0 or T == 0:
        raise ValueError(f"retrieval_prep: empty input {tuple(x.shape)}")
    dev = x.device
    xm = torch.empty(N, V, dtype=torch.float32, device=dev) if mean else None
    ym = torch.empty(N, V, dtype=torch.float32, device=dev) if mean and y is not None else None
    xn = torch.empty(N, dtype=torch.float32, device=dev) if norm_x else None
    yn = torch.empty(N, dtype=torch.float32, device=dev) if norm_y and y is not None else None
    check(lib().tribe_retrieval_prep(x.data_ptr(), _p(y), N, V, T, sn, sv, st, _p(xm), _p(ym), _p(xn), _p(yn), _stream()),
          "tribe_retrieval_prep")
    return xm, ym, xn, yn


def _rows(x: torch.Tensor, name: str) -> torch.Tensor:
    _cuda(x, torch.float32, name, contiguous=False)
    if x.ndim != 2 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        raise ValueError(f"{name}: expected an f32 [rows, V] matrix with unit column stride, got {tuple(x.shape)} / {x.stride()}")
    return x


def retrieval_ranks(x: torch.Tensor, y: torch.Tensor, y_norm: torch.Tensor, true_idx: torch.Tensor | None = None,
                    relative: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """Rank of every query x [N, V] among the gallery y [M, V] (y_norm [M] from retrieval_prep), true row t(n) = true_idx[n]
    (int64 [N]) or n.  Writes f32 [N] into `out` (e.g. a slice of a metric's state buffer) or a new tensor."""
    _rows(x, "x")
    _rows(y, "y")
    _cuda(y_norm, torch.float32, "y_norm")
    (N, V), M = x.shape, y.shape[0]
    if y.shape[1] != V or y_norm.shape != (M,):
        raise ValueError(f"retrieval_ranks: x {tuple(x.shape)}, y {tuple(y.shape)}, y_norm {tuple(y_norm.shape)}")
    if true_idx is None and N != M:
        raise ValueError(f"retrieval_ranks: without labels queries and gallery must have the same length, got {N} and {M}")
    if true_idx is not None:
        _cuda(true_idx, torch.int64, "true_idx")
        if true_idx.shape != (N,):
            raise ValueError(f"retrieval_ranks: true_idx must be [{N}], got {tuple(true_idx.shape)}")
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
    _cuda(out, torch.float32, "out")
    if out.shape != (N,):
        raise ValueError(f"retrieval_ranks: out must be [{N}], got {tuple(out.shape)}")
    check(lib().tribe_retrieval_ranks(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), y_norm.data_ptr(), N, M, V, _p(true_idx),
                                      int(bool(relative)), out.data_ptr(), _stream()), "tribe_retrieval_ranks")
    return out


def retrieval_scores(x: torch.Tensor, y: torch.Tensor, norm_kind: str | None = "y") -> torch.Tensor:
    """Materialised f32 [N, M] similarity of Rank._compute_sim (norm_kind None | "x" | "y" | "xy"); diagnostic path."""
    if norm_kind not in _NORM_KINDS:
        raise ValueError(f"norm must be None, x, y or xy, got {norm_kind}.")
    _rows(x, "x")
    _rows(y, "y")
    (N, V), M = x.shape, y.shape[0]
    if y.shape[1] != V:
        raise ValueError(f"retrieval_scores: x {tuple(x.shape)} vs y {tuple(y.shape)}")
    xn = retrieval_prep(x, mean=False, norm_x=True)[2] if norm_kind in ("x", "xy") else None
    yn = retrieval_prep(y, mean=False, norm_x=True)[2] if norm_kind in ("y", "xy") else None
    out = torch.empty(N, M, dtype=torch.float32, device=x.device)
    check(lib().tribe_retrieval_scores(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), N, M, V, _p(xn), _p(yn),
                                       _NORM_KINDS[norm_kind], out.data_ptr(), _stream()), "tribe_retrieval_scores")
    return out


def rank_reduce(ranks: torch.Tensor, topk: float = 1.0) -> torch.Tensor:
    """f32 [4] = {mean, unbiased std, lower median, mean(ranks < topk)} of f32 ranks [n], n > 0 (one launch)."""
    _cuda(ranks, torch.float32, "ranks")
    n = ranks.numel()
    if n == 0:
        raise ValueError("rank_reduce: no ranks")
    out = torch.empty(4, dtype=torch.float32, device=ranks.device)
    check(lib().tribe_rank_reduce(ranks.data_ptr(), n, float(topk), out.data_ptr(), _stream()), "tribe_rank_reduce")
    return out


# --------------------------------------------------------------------------------------
# Spearman rank correlation (csrc/rank_corr.hip)
# --------------------------------------------------------------------------------------
SPEARMAN_MAX_SAMPLES = 1 << 20   # tribe_spearman_max_samples(): the int64 rank sums are exact up to here


def spearman_default_chunk() -> int:
    """The largest column one workgroup sorts and ranks in LDS (`chunk=0` of spearman_columns)."""
    return int(lib().tribe_spearman_default_chunk())


def rank_append(pred_state: torch.Tensor, true_state: torch.Tensor, counts: torch.Tensor, pred: torch.Tensor, true: torch.Tensor,
                group: torch.Tensor | None = None) -> None:
    """Append the samples of pred / true [B, V, T] (any common strides) to the sample state f32 [G, V, capacity]: the T samples of
    batch row b go behind the counts[group[b]] samples its group holds (group int64 [B], None: group 0), and counts (int64 [G], on
    the device) advance.  The caller keeps capacity at or above the number of samples it has appended: a row that would not fit is
    dropped.  No host synchronisation."""
    _cuda(pred_state, torch.float32, "pred_state")
    _cuda(true_state, torch.float32, "true_state")
    _cuda(counts, torch.int64, "counts")
    _cuda(pred, torch.float32, "pred", contiguous=False)
    _cuda(true, torch.float32, "true", contiguous=False)
    B, V, T, sb, sv, st = _bvt_strides(pred, true, "rank_append")
    G, cap = pred_state.shape[0], pred_state.shape[-1]
    if pred_state.shape != (G, V, cap) or true_state.shape != (G, V, cap) or counts.shape != (G,):
        raise ValueError(f"rank_append: states must be [G, {V}, capacity] and counts [G], got {tuple(pred_state.shape)} / "
                         f"{tuple(true_state.shape)} / {tuple(counts.shape)}")
    if B == 0 or T == 0:
        return
    if group is not None:
        _cuda(group, torch.int64, "group")
        if group.numel() != B:
            raise ValueError("rank_append: group must have B entries")
    positions = torch.empty(B, dtype=torch.int64, device=pred.device)
    check(lib().tribe_rank_append(pred.data_ptr(), true.data_ptr(), B, V, T, sb, sv, st, _p(group), G, cap, counts.data_ptr(),
                                  positions.data_ptr(), pred_state.data_ptr(), true_state.data_ptr(), _stream()), "tribe_rank_append")


def _spearman_state(pred_cols: torch.Tensor, true_cols: torch.Tensor, n: int, chunk: int, want_ranks: bool
                    ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None, torch.Tensor | None]:
    """Columns as the state holds them: f32 [V, ld] with the first n of every row filled."""
    V, ld = pred_cols.shape
    if n > SPEARMAN_MAX_SAMPLES:
        raise ValueError(f"spearman: {n} samples in one group exceed 2^20")
    dev = pred_cols.device
    rho = torch.empty(V, dtype=torch.float32, device=dev)
    sums = torch.empty(V, 3, dtype=torch.int64, device=dev)
    rp = torch.empty(V, n, dtype=torch.float32, device=dev) if want_ranks else None
    rt = torch.empty(V, n, dtype=torch.float32, device=dev) if want_ranks and true_cols is not pred_cols else None
    ws = workspace(lib().tribe_spearman_workspace_bytes(n, V, chunk), dev, "spearman")
    check(lib().tribe_spearman_columns(pred_cols.data_ptr(), true_cols.data_ptr(), ld, n, V, chunk, rho.data_ptr(), sums.data_ptr(),
                                       _p(rp), _p(rt), ws.data_ptr(), ws.numel(), _stream()), "tribe_spearman_columns")
    return rho, sums, rp, rt


def spearman_from_state(pred_state: torch.Tensor, true_state: torch.Tensor, n: int, chunk: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """(rho f32 [V], sums int64 [V, 3]) of one group's sample state f32 [V, capacity] (a row of rank_append's state), n samples
    per column."""
    _cuda(pred_state, torch.float32, "pred_state")
    _cuda(true_state, torch.float32, "true_state")
    if pred_state.ndim != 2 or pred_state.shape != true_state.shape or not 1 <= n <= pred_state.shape[1]:
        raise ValueError(f"spearman_from_state: states {tuple(pred_state.shape)} / {tuple(true_state.shape)}, n = {n}")
    return _spearman_state(pred_state, true_state, int(n), int(chunk), False)[:2]


def _sample_columns(x: torch.Tensor, y: torch.Tensor, what: str) -> tuple[torch.Tensor, torch.Tensor, int]:
    """[N, V] matrices -> their [V, N] column-contiguous copies, through the append kernel."""
    _cuda(x, torch.float32, "x", contiguous=False)
    _cuda(y, torch.float32, "y", contiguous=False)
    if x.ndim != 2 or x.shape != y.shape or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError(f"{what}: expected equal non-empty [N, V] matrices, got {tuple(x.shape)} / {tuple(y.shape)}")
    N, V = x.shape
    if N > SPEARMAN_MAX_SAMPLES:
        raise ValueError(f"{what}: {N} samples exceed 2^20")
    if x.stride() != y.stride():
        x, y = x.contiguous(), y.contiguous()
    xs = torch.empty(1, V, N, dtype=torch.float32, device=x.device)
    ys = torch.empty_like(xs)
    rank_append(xs, ys, torch.zeros(1, dtype=torch.int64, device=x.device), x.t().unsqueeze(0), y.t().unsqueeze(0))
    return xs[0], ys[0], N


def spearman_columns(x: torch.Tensor, y: torch.Tensor, chunk: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """Spearman's rho of every column of x / y f32 [N, V] (scipy.stats.spearmanr per column, nan_policy "propagate"): (rho f32 [V],
    sums int64 [V, 3] = {sum a b, sum a^2, sum b^2} of the doubled centred ranks a, b).  chunk: 0 = default; a power of two in
    [64, spearman_default_chunk()] moves the border between the one-workgroup route (N <= chunk) and the merge route."""
    xs, ys, N = _sample_columns(x, y, "spearman_columns")
    return _spearman_state(xs, ys, N, int(chunk), False)[:2]


def rank_columns(x: torch.Tensor, chunk: int = 0) -> torch.Tensor:
    """Average ranks (1-based, ties share the mean of their positions) of every column of x f32 [N, V], as
    scipy.stats.rankdata(x, "average", axis=0); f32 [N, V] (a transposed view of the [V, N] the kernel writes).  A column with a NaN
    is NaN."""
    xs, _, N = _sample_columns(x, x, "rank_columns")
    return _spearman_state(xs, xs, N, int(chunk), True)[2].t()


# --------------------------------------------------------------------------------------
# block bootstrap of the per-parcel Pearson r (csrc/bootstrap.hip)
# --------------------------------------------------------------------------------------
BOOTSTRAP_MAX_BLOCKS = 32768       # n_sel: one replicate's int32 histogram lives in LDS (128 KiB)
BOOTSTRAP_MAX_REPLICATES = 16384   # one column of replicates is sorted in LDS (64 KiB of keys)


def bootstrap_counts(seed: int, n_boot: int, n_sel: int, device: torch.device | str) -> torch.Tensor:
    """int32 [n_boot, n_sel]: how often replicate r draws each of n_sel blocks.  Draw k of replicate r is word k & 3 of Philox4x32-10
    with counter (k >> 2, r, 0, 0) and key (seed & 0xffffffff, seed >> 32), mapped to the index (u * n_sel) >> 32.  The map is not
    rejection-corrected: an index is over-represented by less than n_sel / 2^32 (< 8e-6 at the limit of 32768 blocks).  The draw
    depends on (seed, r, k, n_sel) alone, so equal seeds resample two models identically."""
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"bootstrap_counts: seed must be an integer in [0, 2^64), got {seed!r}")
    if not 1 <= n_boot <= BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"bootstrap_counts: n_boot = {n_boot} outside [1, {BOOTSTRAP_MAX_REPLICATES}]")
    if not 1 <= n_sel <= BOOTSTRAP_MAX_BLOCKS:
        raise ValueError(f"bootstrap_counts: n_sel = {n_sel} blocks outside [1, {BOOTSTRAP_MAX_BLOCKS}]")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.TribeHipError(f"bootstrap_counts: device {device}; the TRIBE hot path runs on the GPU only (no CPU fallback)")
    counts = torch.empty(n_boot, n_sel, dtype=torch.int32, device=device)
    check(lib().tribe_bootstrap_counts(seed, n_boot, n_sel, counts.data_ptr(), _stream()), "tribe_bootstrap_counts")
    return counts


def bootstrap_pearson(stats: torch.Tensor, blocks: torch.Tensor, counts: torch.Tensor | None
                      ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """stats f64 [n_blocks, V, 6] (pearson_stats_update with one group per block), blocks int64 [n_sel] (the resampled blocks),
    counts int32 [n_boot, n_sel] or None (the observed values alone) -> (observed f32 [V], replicates f32 [n_boot, V], mean_observed
    f32 [], mean_replicates f32 [n_boot]).  Replicate r of parcel v is pearson_from_stats' rule on sum_j counts[r, j] *
    stats[blocks[j], v] (f64, j ascending); `observed` takes every count as 1 through the same kernel.  The means are over parcels
    (NaN when one parcel is NaN).  The four results are views of one [n_boot + 1, V + 1] table."""
    _cuda(stats, torch.float64, "stats")
    _cuda(blocks, torch.int64, "blocks")
    if stats.ndim != 3 or stats.shape[2] != 6 or stats.shape[0] == 0 or stats.shape[1] == 0:
        raise ValueError(f"bootstrap_pearson: stats must be a non-empty [n_blocks, V, 6], got {tuple(stats.shape)}")
    n_blocks, V, _ = stats.shape
    n_sel = blocks.numel()
    if blocks.ndim != 1 or not 1 <= n_sel <= BOOTSTRAP_MAX_BLOCKS:
        raise ValueError(f"bootstrap_pearson: blocks must be int64 [n_sel], 1 <= n_sel <= {BOOTSTRAP_MAX_BLOCKS}, got {tuple(blocks.shape)}")
    n_boot = 0
    if counts is not None:
        _cuda(counts, torch.int32, "counts")
        if counts.ndim != 2 or counts.shape[1] != n_sel or not 1 <= counts.shape[0] <= BOOTSTRAP_MAX_REPLICATES:
            raise ValueError(f"bootstrap_pearson: counts must be [n_boot <= {BOOTSTRAP_MAX_REPLICATES}, {n_sel}], got {tuple(counts.shape)}")
        n_boot = counts.shape[0]
    table = torch.empty(n_boot + 1, V + 1, dtype=torch.float32, device=stats.device)
    check(lib().tribe_bootstrap_pearson(stats.data_ptr(), n_blocks, V, blocks.data_ptr(), n_sel, _p(counts), n_boot, table.data_ptr(), V + 1,
                                        table.data_ptr() + 4 * V, V + 1, _stream()), "tribe_bootstrap_pearson")
    return table[n_boot, :V], table[:n_boot, :V], table[n_boot, V], table[:n_boot, V]


@_functools.lru_cache(maxsize=16)
def _quantile_tensor(qs: tuple[float, ...], device: torch.device) -> torch.Tensor:
    return torch.tensor(qs, dtype=torch.float64, device=device)   # read by the kernel only: one upload per (quantiles, device)


def bootstrap_summary(replicates: torch.Tensor, quantiles: tp.Sequence[float]
                      ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per column of replicates f32 [n, C] (rows may be strided, n <= 16384), over the column's m non-NaN values: (quantile values
    f32 [n_q, C] by numpy's "linear" rule, std f32 [C] with ddof = 1 (NaN for m < 2), n_le int32 [C] = #{x <= 0}, n_ge int32 [C] =
    #{x >= 0}, n_valid int32 [C] = m).  A column without a valid value has NaN quantiles."""
    _cuda(replicates, torch.float32, "replicates", contiguous=False)
    if replicates.ndim != 2 or replicates.shape[0] == 0 or replicates.shape[1] == 0:
        raise ValueError(f"bootstrap_summary: expected a non-empty [n, C] table, got {tuple(replicates.shape)}")
    n, Cn = replicates.shape
    if n > BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"bootstrap_summary: {n} replicates exceed {BOOTSTRAP_MAX_REPLICATES}")
    if Cn > 1 and replicates.stride(1) != 1 or replicates.stride(0) < Cn:
        replicates = replicates.contiguous()
    qs = [float(q) for q in quantiles]
    if not qs or not all(0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"bootstrap_summary: quantiles must be a non-empty sequence of values in [0, 1], got {quantiles!r}")
    dev = replicates.device
    q_dev = _quantile_tensor(tuple(qs), dev)
    qv = torch.empty(len(qs), Cn, dtype=torch.float32, device=dev)
    sd = torch.empty(Cn, dtype=torch.float32, device=dev)
    cnt = torch.empty(3, Cn, dtype=torch.int32, device=dev)
    check(lib().tribe_bootstrap_summary(replicates.data_ptr(), n, Cn, replicates.stride(0), q_dev.data_ptr(), len(qs), qv.data_ptr(),
                                        sd.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(), _stream()),
          "tribe_bootstrap_summary")
    return qv, sd, cnt[0], cnt[1], cnt[2]


def bootstrap_p_values(n_le: torch.Tensor, n_ge: torch.Tensor, n_valid: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(p_le, p_ge, two-sided) f32 from bootstrap_summary's counts: p_le = (1 + #{x <= 0}) / (m + 1) (H0: the value is <= 0),
    p_ge = (1 + #{x >= 0}) / (m + 1), two-sided = min(1, 2 min(p_le, p_ge)); f64 ratios rounded once; NaN for m = 0."""
    m = n_valid.double()
    p = (1.0 + torch.stack([n_le, n_ge]).double()) / (m + 1.0)
    p = torch.cat([p, torch.clamp(2.0 * p.min(0, keepdim=True).values, max=1.0)])
    p = torch.where(m > 0, p, float("nan")).float()
    return p[0], p[1], p[2]


# --------------------------------------------------------------------------------------
# measurement hook: HIP events around every GEMM launch, summed per operator role
# --------------------------------------------------------------------------------------
def prof_begin(max_records: int = 4096) -> None:
    check(lib().tribe_prof_begin(max_records), "tribe_prof_begin")


def prof_end() -> dict[str, dict[str, float]]:
    n = len(_lib.ROLES)
    ms, cnt, fl = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)()
    check(lib().tribe_prof_end(n, ms, cnt, fl), "tribe_prof_end")
    return {role: {"ms": ms[i], "launches": int(cnt[i]), "flops": fl[i]} for i, role in enumerate(_lib.ROLES) if cnt[i]}


__all__ = [n for n in dir() if not n.startswith("_")]
_ = tp


# --------------------------------------------------------------------------------------
# segment assembly from HBM-resident extractor outputs (csrc/features.hip)
# --------------------------------------------------------------------------------------
def group_mean(states: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """states f32 [batch, n_states, plane...] -> f32 [batch, n_groups, plane...]: mean over layers lo[g]..hi[g]-1
    (`_aggregate_layers`, text.py:129-149).  lo / hi int32 device tensors."""
    _cuda(states, torch.float32, "states")
    _cuda(lo, torch.int32, "lo")
    _cuda(hi, torch.int32, "hi")
    if states.ndim < 3 or lo.shape != hi.shape or lo.ndim != 1:
        raise ValueError(f"group_mean: states {tuple(states.shape)} / bounds {tuple(lo.shape)}, {tuple(hi.shape)}")
    batch, n_states = states.shape[:2]
    plane = states[0, 0].numel()
    out = torch.empty((batch, lo.numel()) + tuple(states.shape[2:]), dtype=torch.float32, device=states.device)
    check(lib().tribe_group_mean_fwd(states.data_ptr(), batch, n_states, plane, lo.data_ptr(), hi.data_ptr(), lo.numel(), out.data_ptr(),
                                     _stream()), "tribe_group_mean_fwd")
    return out


def segment_gather(pieces: torch.Tensor, seg_ptr: torch.Tensor, B: int, C: int, T: int, packed: bool, C_pad: int | None = None) -> torch.Tensor:
    """Sum time slices of cached arrays into segment outputs.  pieces: uint8 device tensor holding `tribe_feature_piece`
    records, seg_ptr int32 [B + 1].  packed -> bf16 [B*T, C_pad]; else f32 [B, C, T]."""
    _cuda(pieces, torch.uint8, "pieces")
    _cuda(seg_ptr, torch.int32, "seg_ptr")
    if seg_ptr.numel() != B + 1 or pieces.numel() % _lib.FEATURE_PIECE_DTYPE.itemsize:
        raise ValueError("segment_gather: seg_ptr must hold B + 1 offsets and pieces whole records")
    if packed:
        C_pad = round_up(C, 64) if C_pad is None else C_pad
        out = torch.empty(B * T, C_pad, dtype=torch.bfloat16, device=pieces.device)
    else:
        C_pad = C
        out = torch.empty(B, C, T, dtype=torch.float32, device=pieces.device)
    check(lib().tribe_segment_gather_fwd(pieces.data_ptr(), seg_ptr.data_ptr(), B, C, T, out.data_ptr(), BF16 if packed else F32, C_pad,
                                         _stream()), "tribe_segment_gather_fwd")
    return out


def word_bag(table: torch.Tensor, row_ptr: torch.Tensor, word_idx: torch.Tensor, rows: int, C_pad: int | None = None,
             f32: bool = False) -> torch.Tensor:
    """table f32 [n_words, C]; CSR (row_ptr int32 [rows + 1], word_idx int32) -> bf16 [rows, C_pad] row sums
    (f32=True: the unrounded sums, f32 [rows, C])."""
    _cuda(table, torch.float32, "table")
    _cuda(row_ptr, torch.int32, "row_ptr")
    _cuda(word_idx, torch.int32, "word_idx")
    if table.ndim != 2 or row_ptr.numel() != rows + 1:
        raise ValueError(f"word_bag: table {tuple(table.shape)}, row_ptr {tuple(row_ptr.shape)} for {rows} rows")
    n_words, C = table.shape
    if f32:
        out = torch.empty(rows, C, dtype=torch.float32, device=table.device)
        if word_idx.numel() == 0:
            return out.zero_()
        check(lib().tribe_word_bag_f32_fwd(table.data_ptr(), n_words, C, row_ptr.data_ptr(), word_idx.data_ptr(), rows, out.data_ptr(),
                                           _stream()), "tribe_word_bag_f32_fwd")
        return out
    C_pad = round_up(C, 64) if C_pad is None else C_pad
    out = torch.empty(rows, C_pad, dtype=torch.bfloat16, device=table.device)
    if word_idx.numel() == 0:   # no word overlaps any row: the output is all zeros (and the kernel would get a null list)
        return out.zero_()
    check(lib().tribe_word_bag_fwd(table.data_ptr(), n_words, C, row_ptr.data_ptr(), word_idx.data_ptr(), rows, out.data_ptr(), C_pad,
                                   _stream()), "tribe_word_bag_fwd")
    return out


# --------------------------------------------------------------------------------------
# after the model: submission rows, ensemble averaging (csrc/features.hip)
# --------------------------------------------------------------------------------------
def transpose_f32(x: torch.Tensor) -> torch.Tensor:
    """f32 [Z, R, C] -> [Z, C, R] (predictions [B, V, T'] -> [B, T', V], callbacks.py:63-64)."""
    _cuda(x, torch.float32, "x")
    if x.ndim != 3:
        raise ValueError(f"transpose_f32: expected [Z, R, C], got {tuple(x.shape)}")
    Z, R, Cc = x.shape
    out = torch.empty(Z, Cc, R, dtype=torch.float32, device=x.device)
    check(lib().tribe_transpose_f32_fwd(x.data_ptr(), Z, R, Cc, out.data_ptr(), _stream()), "tribe_transpose_f32_fwd")
    return out


def weighted_sum(preds: torch.Tensor, w_column: torch.Tensor | None = None, w_set: torch.Tensor | None = None) -> torch.Tensor:
    """preds f32 [N, ..., V] -> sum over N of preds * w: w_column f32 [N, V] (f32 result) or w_set f64 [N] (f64 result)."""
    _cuda(preds, torch.float32, "preds")
    N, V = preds.shape[0], preds.shape[-1]
    M = preds[0].numel()
    if (w_column is None) == (w_set is None):
        raise ValueError("weighted_sum: give exactly one of w_column / w_set")
    if w_column is not None:
        _cuda(w_column, torch.float32, "w_column")
        if tuple(w_column.shape) != (N, V):
            raise ValueError(f"weighted_sum: w_column {tuple(w_column.shape)} != ({N}, {V})")
        out = torch.empty(preds.shape[1:], dtype=torch.float32, device=preds.device)
    else:
        _cuda(w_set, torch.float64, "w_set")
        if tuple(w_set.shape) != (N,):
            raise ValueError(f"weighted_sum: w_set {tuple(w_set.shape)} != ({N},)")
        out = torch.empty(preds.shape[1:], dtype=torch.float64, device=preds.device)
    check(lib().tribe_weighted_sum_fwd(preds.data_ptr(), N, M, V, _p(w_column), _p(w_set), out.data_ptr(), _stream()), "tribe_weighted_sum_fwd")
    return out


def corr_matrix(x: torch.Tensor) -> torch.Tensor:
    """np.corrcoef over the rows of x f32 [N, K] -> f64 [N, N]."""
    _cuda(x, torch.float32, "x")
    if x.ndim != 2:
        raise ValueError(f"corr_matrix: expected [N, K], got {tuple(x.shape)}")
    N, K = x.shape
    out = torch.empty(N, N, dtype=torch.float64, device=x.device)
    nbytes = lib().tribe_corr_matrix_workspace_bytes(N)
    ws = workspace(nbytes, x.device, tag="corr")
    check(lib().tribe_corr_matrix_fwd(x.data_ptr(), N, K, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "tribe_corr_matrix_fwd")
    return out


# --------------------------------------------------------------------------------------
# fp8 (e4m3) GEMM + per-tensor quantisation (csrc/gemm_fp8.hip)
# --------------------------------------------------------------------------------------
FP8_MAX = 448.0


def absmax(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """max |x| of a 2-D f32 / bf16 tensor as a device float (accumulates into `out` when given)."""
    _cuda(x, (torch.float32, torch.bfloat16), "x")
    x2 = x.reshape(-1, x.shape[-1])
    acc = out is not None
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().tribe_absmax_fwd(x2.data_ptr(), _DT[x.dtype], x2.shape[0], x2.shape[1], x2.shape[1], out.data_ptr(), int(acc), _stream()),
          "tribe_absmax_fwd")
    return out


def quantize_fp8(x: torch.Tensor, scale: float, K_pad: int | None = None) -> torch.Tensor:
    """x f32 / bf16 [M, K] -> uint8 [M, K_pad] holding e4m3(clamp(x / scale)); K_pad defaults to K rounded up to 128."""
    _cuda(x, (torch.float32, torch.bfloat16), "x")
    if x.ndim != 2 or not scale > 0:
        raise ValueError(f"quantize_fp8: expected a 2-D tensor and a positive scale, got {tuple(x.shape)}, {scale}")
    M, K = x.shape
    K_pad = round_up(K, 128) if K_pad is None else K_pad
    out = torch.empty(M, K_pad, dtype=torch.uint8, device=x.device)
    check(lib().tribe_quantize_fp8_fwd(x.data_ptr(), _DT[x.dtype], M, K, K, 1.0 / scale, out.data_ptr(), K_pad, _stream()),
          "tribe_quantize_fp8_fwd")
    return out


def norm_quantize_fp8(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, eps: float, scale: float, layernorm: bool) -> torch.Tensor:
    """quantize_fp8(rmsnorm(x) | layernorm(x) in bf16, scale) in one pass: x f32 [..., dim] -> uint8 [rows, dim] of e4m3 bytes."""
    dim = _norm_params("norm_quantize_fp8", x, w, b)
    _cuda(x, torch.float32, "x")
    _cuda(w, torch.float32, "w")
    if b is not None:
        _cuda(b, torch.float32, "b")
    if not scale > 0:
        raise ValueError(f"norm_quantize_fp8: scale must be positive, got {scale}")
    rows = x.numel() // dim
    out = torch.empty(rows, dim, dtype=torch.uint8, device=x.device)
    check(lib().tribe_norm_quantize_fp8_fwd(x.data_ptr(), rows, dim, w.data_ptr(), _p(b), int(layernorm), eps, 1.0 / scale, out.data_ptr(),
                                            _stream()), "tribe_norm_quantize_fp8_fwd")
    return out


def gemm_fp8_nt(a: torch.Tensor, b: torch.Tensor, alpha: float, *, bias: torch.Tensor | None = None, act: str | None = None,
                res: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[m, n] = epi(alpha * sum_k a[m, k] * b[n, k]) with a, b uint8 tensors of e4m3 bytes ([M, K], [N, K], K % 128 == 0)."""
    _cuda(a, torch.uint8, "a")
    _cuda(b, torch.uint8, "b")
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"gemm_fp8_nt: incompatible shapes {tuple(a.shape)} x {tuple(b.shape)}")
    M, K = a.shape
    N = b.shape[0]
    n_out = N // 2 if act in ("swiglu", "glu") else N
    if out is None:
        out = torch.empty(M, n_out, dtype=out_dtype, device=a.device)
    _cuda(out, (torch.float32, torch.bfloat16), "out")
    for name, t in (("bias", bias), ("res", res)):
        if t is not None:
            _cuda(t, torch.float32, name)
    _gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=n_out, alpha=alpha, bias=bias, act=_ACT[act], res=res, ldres=N, fp8=True)
    return out


# --------------------------------------------------------------------------------------
# Wav2Vec-BERT audio front end: waveform -> filterbank features (csrc/fbank.hip)
# --------------------------------------------------------------------------------------
FBANK_WIN, FBANK_HOP, FBANK_NFFT, FBANK_MEL, FBANK_STRIDE = 400, 160, 512, 80, 2    # SeamlessM4TFeatureExtractor defaults, 16 kHz
FBANK_MAX_CHUNKS = 32                                                               # TRIBE_FBANK_MAX_CHUNKS


def fbank_frame_count(n: int) -> int:
    """Frames of 400 samples every 160 in a waveform of n samples (no centring); the features have ceil(F / 2) rows."""
    if n < FBANK_WIN:
        raise ValueError(f"fbank: a waveform of {n} samples is shorter than one frame ({FBANK_WIN})")
    return 1 + (n - FBANK_WIN) // FBANK_HOP


def povey_window() -> _np.ndarray:
    """Kaldi's Povey window, f64 [400]: hann(400, symmetric) ** 0.85."""
    return _np.power(_np.hanning(FBANK_WIN), 0.85)


def kaldi_mel_filters() -> _np.ndarray:
    """80 triangular filters on Kaldi's mel scale 1127 ln(1 + f / 700), 20 Hz to 8 kHz, triangles drawn in mel space, no
    area normalisation: f64 [257, 80] over the bins of a 512-point DFT at 16 kHz."""
    def to_mel(f):
        return 1127.0 * _np.log(1.0 + f / 700.0)

    n_bins = FBANK_NFFT // 2 + 1
    centres = _np.linspace(to_mel(20.0), to_mel(8000.0), FBANK_MEL + 2)
    bins = to_mel(16_000 / FBANK_NFFT * _np.arange(n_bins))
    width = _np.diff(centres)
    slopes = centres[None, :] - bins[:, None]
    down, up = -slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]
    return _np.maximum(0.0, _np.minimum(down, up))


_FBANK_TABLES: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}


def _fbank_tables(device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _FBANK_TABLES:
        _FBANK_TABLES[key] = (torch.from_numpy(povey_window().astype(_np.float32)).to(device),
                              torch.from_numpy(_np.ascontiguousarray(kaldi_mel_filters().astype(_np.float32))).to(device))
    return _FBANK_TABLES[key]


def w2vbert_fbank(wavs: torch.Tensor | tp.Sequence[torch.Tensor], zscore: bool = True) -> tuple[torch.Tensor, list[int]]:
    """16 kHz waveform chunk(s) f32 [n] or [n, C] (sample-major) -> (input_features f32 [B, T_max, 160], each chunk's T).
    zscore: the reference's `_preprocess_wav` first (mean over channels, z-score over the chunk); without it a multi-channel
    chunk is still averaged over its channels.  Chunks of different lengths run in one launch sequence; rows past a chunk's T
    are zero, and a chunk's rows are the same bits whatever else is in the batch."""
    chunks = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
    if not 1 <= len(chunks) <= FBANK_MAX_CHUNKS:
        raise ValueError(f"w2vbert_fbank: {len(chunks)} chunks (1 to {FBANK_MAX_CHUNKS} per call)")
    for i, w in enumerate(chunks):
        _cuda(w, torch.float32, f"wavs[{i}]")
        if w.ndim not in (1, 2) or w.device != chunks[0].device:
            raise ValueError(f"w2vbert_fbank: wavs[{i}] must be [n] or [n, channels] on one device, got {tuple(w.shape)} on {w.device}")
    channels = {1 if w.ndim == 1 else int(w.shape[1]) for w in chunks}
    if len(channels) != 1 or min(channels) < 1:
        raise ValueError(f"w2vbert_fbank: chunks of one call share a channel count >= 1, got {sorted(channels)}")
    lengths = [(fbank_frame_count(int(w.shape[0])) + 1) // 2 for w in chunks]
    B, device = len(chunks), chunks[0].device
    window, mel = _fbank_tables(device)
    n = (C.c_int64 * B)(*[int(w.shape[0]) for w in chunks])
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in chunks])
    got = (C.c_int32 * B)()
    out = torch.empty(B, max(lengths), FBANK_STRIDE * FBANK_MEL, dtype=torch.float32, device=device)
    ws = workspace(lib().tribe_fbank_workspace_bytes(n, B), device, tag="fbank")
    check(lib().tribe_fbank_fwd(ptrs, n, B, channels.pop(), int(bool(zscore)), window.data_ptr(), mel.data_ptr(), out.data_ptr(), out.shape[1],
                                got, ws.data_ptr(), ws.numel(), _stream()), "tribe_fbank_fwd")
    assert list(got) == lengths
    return out, lengths


# --------------------------------------------------------------------------------------
# Wav2Vec-BERT audio front end: native-rate waveform -> 16 kHz, julius' windowed-sinc filter (csrc/resample.hip)
# --------------------------------------------------------------------------------------
RESAMPLE_MAX_CHUNKS = 32                      # TRIBE_RESAMPLE_MAX_CHUNKS
RESAMPLE_TABLE_MAX_BYTES = 64 << 20           # the cap of tribe_resample_frac_fwd


@_functools.lru_cache(maxsize=16)
def julius_resample_kernels(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945) -> tuple[int, int, int, torch.Tensor]:
    """The polyphase filter bank of `julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff)` (julius 0.2.7, the reference's
    audio.py:129-138): (old, new, width, table f32 [new, 2 * width + old]) with old / new the rates divided by their gcd.  Row i
    filters output phase i: a sinc low-pass at min(old, new) * rolloff, cut at `zeros` zero crossings by a squared-cosine window,
    normalised to sum 1.  It is built in FLOAT32 WITH THE TORCH OPS JULIUS USES, in its order, because the precision is part of what
    the reference computes: a float64 table differs by up to 3.4e-5 per tap at 441 / 160.  julius is not installed here: this is a
    restatement of its published source, and parity with the package itself is not executed.  Equal rates give an empty table of
    width 0 (nothing to filter); a table above 64 MiB (44100 -> 16001 asks for gigabytes) is a ValueError."""
    old_sr, new_sr = int(old_sr), int(new_sr)
    if old_sr < 1 or new_sr < 1:
        raise ValueError(f"julius_resample_kernels: rates must be >= 1, got {old_sr} -> {new_sr}")
    g = _math.gcd(old_sr, new_sr)
    old, new = old_sr // g, new_sr // g
    if old == new:
        return old, new, 0, torch.zeros(new, 0, dtype=torch.float32)
    sr = min(new, old) * rolloff
    width = _math.ceil(zeros * old / sr)
    taps = 2 * width + old
    if new * taps * 4 > RESAMPLE_TABLE_MAX_BYTES:
        raise ValueError(f"julius_resample_kernels: {old_sr} -> {new_sr} reduces to {old} / {new}: a table of {new} x {taps} float32 "
                         f"is above {RESAMPLE_TABLE_MAX_BYTES >> 20} MiB")
    idx = torch.arange(-width, width + old).float()
    rows = []
    for i in range(new):
        t = (-i / new + idx / old) * sr
        t.clamp_(-zeros, zeros)
        t *= _math.pi
        window = torch.cos(t / zeros / 2) ** 2
        kernel = torch.where(t == 0, torch.tensor(1.0, dtype=t.dtype), torch.sin(t) / t) * window
        kernel.div_(kernel.sum())
        rows.append(kernel)
    return old, new, width, torch.stack(rows).contiguous()


def resample_output_length(n: int, old_sr: int, new_sr: int) -> int:
    """Samples julius returns for n input samples: `floor(float32(new * n / old))` -- the division is a Python double and
    `torch.as_tensor` rounds it to float32 before the floor, so this is NOT `new * n // old` (441 / 160: n = 299993 gives 108841,
    one more) -- and never more than the (n // old + 1) * new samples its strided convolution produces."""
    n, g = int(n), _math.gcd(int(old_sr), int(new_sr))
    old, new = int(old_sr) // g, int(new_sr) // g
    if old == new or n <= 0:
        return max(n, 0)
    return min(int(_math.floor(float(_np.float32(new * n / old)))), (n // old + 1) * new)


_RESAMPLE_TABLES: dict[tuple[int, int, int], torch.Tensor] = {}


def resample_frac(wavs: torch.Tensor | tp.Sequence[torch.Tensor], old_sr: int, new_sr: int) -> list[torch.Tensor]:
    """Waveform chunk(s) f32 [n] or [n, channels] (sample-major, on the GPU) at old_sr -> the same at new_sr, each channel through
    julius' `ResampleFrac` filter (`julius_resample_kernels`), `resample_output_length(n)` samples per chunk.  One launch for all
    chunks; a chunk's samples are the same bits alone or in a batch, and a channel's the same bits whatever the channel count.
    Equal rates return the inputs themselves.  A chunk too short to yield a sample (n = 1 at 3 / 1) comes back empty."""
    chunks = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
    if not 1 <= len(chunks) <= RESAMPLE_MAX_CHUNKS:
        raise ValueError(f"resample_frac: {len(chunks)} chunks (1 to {RESAMPLE_MAX_CHUNKS} per call)")
    for i, w in enumerate(chunks):
        if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError(f"resample_frac: wavs[{i}] must be a contiguous float32 tensor on the GPU (there is no host path)")
        if w.ndim not in (1, 2) or w.device != chunks[0].device:
            raise ValueError(f"resample_frac: wavs[{i}] must be [n] or [n, channels] on one device, got {tuple(w.shape)} on {w.device}")
        if w.shape[0] < 1:
            raise ValueError(f"resample_frac: wavs[{i}] is empty")
    channels = {1 if w.ndim == 1 else int(w.shape[1]) for w in chunks}
    if len(channels) != 1 or min(channels) < 1:
        raise ValueError(f"resample_frac: chunks of one call share a channel count >= 1, got {sorted(channels)}")
    old, new, width, table = julius_resample_kernels(int(old_sr), int(new_sr))
    if old == new:
        return chunks
    device = chunks[0].device
    key = (device.index if device.index is not None else torch.cuda.current_device(), old, new)
    if key not in _RESAMPLE_TABLES:
        _RESAMPLE_TABLES[key] = table.to(device)
    n_out = [resample_output_length(int(w.shape[0]), old, new) for w in chunks]
    outs = [torch.empty((m,) + tuple(w.shape[1:]), dtype=torch.float32, device=device) for w, m in zip(chunks, n_out)]
    run = [i for i, m in enumerate(n_out) if m > 0]
    if run:
        B = len(run)
        check(lib().tribe_resample_frac_fwd((C.c_void_p * B)(*[chunks[i].data_ptr() for i in run]), (C.c_int64 * B)(*[int(chunks[i].shape[0]) for i in run]),
                                            B, channels.pop(), old, new, width, _RESAMPLE_TABLES[key].data_ptr(),
                                            (C.c_void_p * B)(*[outs[i].data_ptr() for i in run]), (C.c_int64 * B)(*[n_out[i] for i in run]), _stream()),
              "tribe_resample_frac_fwd")
    return outs


# --------------------------------------------------------------------------------------
# V-JEPA2 video front end: decoded uint8 frames -> pixel_values_videos (csrc/vidproc.hip)
# --------------------------------------------------------------------------------------
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def aa_resize_taps(n_in: int, n_out: int, start: int = 0, count: int | None = None) -> tuple[_np.ndarray, _np.ndarray]:
    """The separable antialiased triangle filter of `F.interpolate(mode="bilinear", align_corners=False, antialias=True)` along
    one axis of n_in samples resized to n_out, for output positions start .. start + count - 1: (first int32 [count], weights
    f32 [count, taps]) with out[i] = sum_k weights[i, k] * in[first[i] + k].  With scale = n_in / n_out and support =
    max(scale, 1), position i is centred on scale * (i + 0.5), its window is [max(0, int(centre - support + 0.5)), min(n_in,
    int(centre + support + 0.5))), tap j weighs max(0, 1 - |(j - centre + 0.5) / max(scale, 1)|), and the weights are divided by
    their sum: float64 throughout, rounded to f32 once.  Taps of weight exactly 0 at either end of a window are dropped (identity
    is one tap of 1.0).  `taps` is the widest window of the table; a narrower row is padded with
    zero weights behind, or, where that would pass the end of the axis, `first` moves down and the zeros go in front, so every row
    has first >= 0 and first + taps <= n_in."""
    count = n_out - start if count is None else count
    if n_in < 1 or n_out < 1 or start < 0 or count < 1 or start + count > n_out:
        raise ValueError(f"aa_resize_taps: positions [{start}, {start} + {count}) of an axis of {n_in} resized to {n_out}")
    scale = n_in / n_out
    support = max(scale, 1.0)
    rows = []
    for i in range(start, start + count):
        centre = scale * (i + 0.5)
        lo, hi = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
        w = _np.maximum(0.0, 1.0 - _np.abs((_np.arange(lo, hi, dtype=_np.float64) - centre + 0.5) / support))
        keep = _np.flatnonzero(w)                                   # the window's end positions may weigh exactly 0 (always, at scale <= 1)
        rows.append((lo + int(keep[0]), (w / w.sum())[keep[0]:keep[-1] + 1]))
    taps = max(len(w) for _, w in rows)
    first = _np.empty(count, _np.int32)
    weights = _np.zeros((count, taps), _np.float64)
    for r, (lo, w) in enumerate(rows):
        first[r] = min(lo, n_in - taps)
        weights[r, lo - first[r]:lo - first[r] + len(w)] = w
    return first, weights.astype(_np.float32)


def video_resized_size(H: int, W: int, crop: int) -> tuple[int, int]:
    """The size `default_video_processor` resizes an H x W frame to: shortest edge int(crop * 256 / 224), aspect kept."""
    short = int(crop * 256 / 224)
    scale = short / min(H, W)
    return max(short, int(round(H * scale))), max(short, int(round(W * scale)))


_VIDEO_TABLES: dict[tuple[int, int, int], tuple[tp.Any, ...]] = {}


def _video_tables(H: int, W: int, crop: int) -> tuple[tp.Any, ...]:
    key = (H, W, crop)
    if key not in _VIDEO_TABLES:
        nh, nw = video_resized_size(H, W, crop)
        first_h, w_h = aa_resize_taps(H, nh, (nh - crop) // 2, crop)
        first_w, w_w = aa_resize_taps(W, nw, (nw - crop) // 2, crop)
        _VIDEO_TABLES[key] = (nh, nw, first_h, _np.ascontiguousarray(w_h), first_w, _np.ascontiguousarray(w_w))
    return _VIDEO_TABLES[key]


def video_preprocess(frames_u8: torch.Tensor, src_index: tp.Any, crop: int) -> torch.Tensor:
    """What `data_utils.features.video.default_video_processor` computes, on the GPU: frames_u8 uint8 [n_src, H, W, 3] (device,
    contiguous) are resized (antialiased bilinear, shortest edge to int(crop * 256 / 224)), centre-cropped, divided by 255 and
    ImageNet-normalised.  src_index (ints, any shape, flattened) names the source frame of every output slot, so a frame several
    clips share is stored once: -> f32 [n_out, 3, crop, crop] from one launch, each slot the same bits whatever else is in the batch."""
    _cuda(frames_u8, None, "frames_u8", contiguous=False)
    if frames_u8.dtype != torch.uint8:
        raise ValueError(f"video_preprocess: frames must be uint8, got {frames_u8.dtype}")
    if frames_u8.ndim != 4 or frames_u8.shape[-1] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"video_preprocess: frames must be [n_src, H, W, 3], got {tuple(frames_u8.shape)}")
    if not frames_u8.is_contiguous():
        raise ValueError("video_preprocess: frames must be contiguous")
    src = _np.ascontiguousarray(_np.asarray(src_index.cpu() if isinstance(src_index, torch.Tensor) else src_index).reshape(-1))
    if src.size < 1 or src.dtype.kind not in "iu":
        raise ValueError("video_preprocess: src_index must hold at least one integer")
    n_src, H, W = (int(v) for v in frames_u8.shape[:3])
    if int(src.min()) < 0 or int(src.max()) >= n_src:
        raise ValueError(f"video_preprocess: src_index must lie in [0, {n_src}), got [{int(src.min())}, {int(src.max())}]")
    src = src.astype(_np.int32)
    crop = int(crop)
    if crop < 1:
        raise ValueError(f"video_preprocess: crop {crop}")
    nh, nw, first_h, w_h, first_w, w_w = _video_tables(H, W, crop)
    mean, std = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    out = torch.empty(src.size, 3, crop, crop, dtype=torch.float32, device=frames_u8.device)
    ws = workspace(lib().tribe_video_preprocess_workspace_bytes(src.size, crop, w_h.shape[1], w_w.shape[1]), frames_u8.device, tag="vidproc")
    check(lib().tribe_video_preprocess_fwd(frames_u8.data_ptr(), n_src, H, W, src.ctypes.data, src.size, nh, nw, crop, first_h.ctypes.data,
                                           w_h.ctypes.data, w_h.shape[1], first_w.ctypes.data, w_w.ctypes.data, w_w.shape[1], mean, std,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "tribe_video_preprocess_fwd")
    return out


# --------------------------------------------------------------------------------------
# optimiser work list and gradient clipping (csrc/backward.hip, csrc/grad_clip.hip)
# --------------------------------------------------------------------------------------
def chunk_work_list(numels: tp.Sequence[int], device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
    """(chunk_tensor int32, chunk_start int64) on `device`: tensor i of numels[i] elements cut into chunks of
    tribe_adam_chunk_elems() -- the work list of tribe_adam_step, tribe_swa_update and tribe_grad_*."""
    chunk = int(lib().tribe_adam_chunk_elems())
    owner, start = [], []
    for i, n in enumerate(numels):
        s = _np.arange(0, n, chunk, dtype=_np.int64)
        owner.append(_np.full(len(s), i, dtype=_np.int32))
        start.append(s)
    return torch.from_numpy(_np.concatenate(owner)).to(device), torch.from_numpy(_np.concatenate(start)).to(device)


_GRAD_WORK: dict[tuple, tuple[torch.Tensor, torch.Tensor]] = {}


def _grad_table(grads: tp.Sequence[torch.Tensor], what: str) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None:
    """(table bytes, chunk_tensor, chunk_start) over the gradients (g and n filled, the other fields NULL); None when there is no element."""
    grads = [_cuda(g, torch.float32, f"{what}: gradient") for g in grads]
    grads = [g for g in grads if g.numel()]
    if not grads:
        return None
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        raise ValueError(f"{what}: gradients must live on one GPU")
    sig = (dev.index,) + tuple(g.numel() for g in grads)
    work = _GRAD_WORK.get(sig)
    if work is None:
        if len(_GRAD_WORK) >= 16:            # parameter subsets change with modality dropout; keep the cache bounded
            _GRAD_WORK.pop(next(iter(_GRAD_WORK)))
        work = _GRAD_WORK[sig] = chunk_work_list(sig[1:], dev)
    table = _np.zeros(len(grads), dtype=_lib.ADAM_TENSOR_DTYPE)
    table["g"] = [g.data_ptr() for g in grads]
    table["n"] = sig[1:]
    return torch.from_numpy(table.view(_np.uint8).reshape(-1)).to(dev), work[0], work[1]


def grad_norm(grads: tp.Sequence[torch.Tensor], max_norm: float, norm_type: float = 2.0) -> tuple[torch.Tensor, torch.Tensor]:
    """(norm, coef), 0-dim f32 on the gradients' device: the L2 (norm_type 2) or max-abs (inf) norm of all `grads` (contiguous f32, one
    GPU) as one vector, accumulated in f64 in a fixed order, and torch's clip coefficient min(1, max_norm / (norm + 1e-6)).  Nothing is
    read back: hand `coef` to grad_scale_ or to HipAdam.step(grad_scale=coef)."""
    norm_type = float(norm_type)
    if norm_type not in (2.0, _math.inf):
        raise ValueError(f"grad_norm: norm_type must be 2 or inf on the HIP route, got {norm_type}")
    built = _grad_table(grads, "grad_norm")
    if built is None:
        if not len(grads):
            raise ValueError("grad_norm: no gradients")
        out = torch.tensor([0.0, min(1.0, float(max_norm) / 1e-6)], dtype=torch.float32, device=grads[0].device)
        return out[0], out[1]
    table, owner, start = built
    partials = torch.empty(owner.numel(), dtype=torch.float64, device=table.device)
    out = torch.empty(2, dtype=torch.float32, device=table.device)
    check(lib().tribe_grad_norm(table.data_ptr(), owner.data_ptr(), start.data_ptr(), owner.numel(), 0 if norm_type == 2.0 else 1,
                                float(max_norm), partials.data_ptr(), out.data_ptr(), _stream()), "tribe_grad_norm")
    return out[0], out[1]


def grad_scale_(grads: tp.Sequence[torch.Tensor], coef: torch.Tensor | None = None, clip_value: float | None = None) -> None:
    """In place: g = clamp(g * coef, -clip_value, clip_value) for every g in `grads`.  coef: f32 device scalar (grad_norm's) or None = 1;
    clip_value None or <= 0 = no clamp.  NaN stays NaN."""
    built = _grad_table(grads, "grad_scale_")
    if built is None:
        return
    table, owner, start = built
    if coef is not None:
        _cuda(coef, torch.float32, "grad_scale_: coef")
        if coef.numel() != 1 or coef.device != table.device:
            raise ValueError("grad_scale_: coef must be one f32 value on the gradients' device")
    check(lib().tribe_grad_scale(table.data_ptr(), owner.data_ptr(), start.data_ptr(), owner.numel(), _p(coef),
                                 0.0 if clip_value is None else float(clip_value), _stream()), "tribe_grad_scale")
    torch.autograd.graph.increment_version(list(grads))      # written through raw pointers: version-keyed caches must see it
