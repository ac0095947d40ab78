"""Transformer encoder config + HIP-backed encoder module.

API mirror of /root/reference/modeling_utils/modeling_utils/models/transformer.py:16-61:
`TransformerEncoderConfig(...).build(dim)` validates `dim % heads == 0`, `dim >= 256` and returns
an `nn.Module` mapping [B, T, dim] -> [B, T, dim].  The reference returns
`x_transformers.Encoder(dim=dim, attn_dim_head=dim // heads, **fields)`; this build returns
`HipEncoder`, which keeps the library's parameter names (so a TRIBE checkpoint's `encoder.*`
keys load unchanged) and runs the arithmetic in gfx950 HIP kernels (tribe_encoder_fwd).

Encoder semantics (third-party, restated -- see oracle/xt_encoder.py for the definition and
its "parity unpinned" status): pre-ScaleNorm, bias-free q/k/v/out projections, partial rotary on
the first max(dim_head // 2, 32) dims, fp32 softmax, scaled residual, GELU(erf) feed-forward,
final ScaleNorm.

Dropout fields: `attn_dropout` (0 <= p < 1, on the attention probabilities after the softmax: out = dropout(softmax(.)) v), `ff_dropout`
(0 <= p < 1, on the feed-forward hidden after the GELU) and `layer_dropout` (0 <= p <= 1, x_transformers' stochastic depth: per sub-layer
`random.random() < layer_dropout` skips norm, block and residual) are stored on the module and act on the autograd training path of
FmriEncoder only (algonauts2025/model.py); `HipEncoder.forward` / `forward_tokens`, the fused inference entry points, apply none of them.
An active `attn_dropout` takes the training path's attention off the flash kernel onto materialised scores and the softmax-dropout row
kernels (modeling_utils.autograd.Attention); its masks are this build's counter-based ones, not torch's.

`causal=True` is x_transformers' `Decoder`: the `Encoder` plus a mask -- scores with key index > query index are filled with -finfo.max before
the softmax -- with the same parameters, `state_dict` keys and rotary.  `HipEncoder(causal=True)` hands the flag to its EncoderPack: the
fused inference path runs tribe_encoder_fwd_ex with TRIBE_ENCODER_CAUSAL (q and k heads through the stand-alone rotary, then the causal
flash kernel).  The training path (FmriEncoder) passes it to modeling_utils.autograd.Attention / RotaryAttention, which then take the
materialised route at every attn_dropout, 0 included, with the causal softmax row kernels (csrc/attn_softmax.hip); the three dropout fields
compose with it unchanged.  dim_head must be one the flash kernel is built for (64, 128, 192, 384).

A causal encoder can also be followed one position at a time: `new_cache(batch_size, max_len)` makes an `EncoderCache` (every layer's
rotated keys and values, bf16 [depth, B, heads, max_len, dim_head]), `step(x[B, dim], cache)` gives the output at position `cache.pos` from
one row per GEMM and a single-query attention against the cache (tribe_encoder_step_fwd: tribe_kv_append + tribe_attention_decode_fwd per
layer, csrc/attn_decode.hip), and `prefill(x[B, T0, dim], cache)` is the causal forward over the first T0 positions that also fills the
cache (tribe_encoder_prefill_fwd).  `extend(x[B, k, dim], cache)` appends a block of k positions to a cache that holds any number of them
(tribe_encoder_extend_fwd: k rows per sequence through every GEMM, tribe_kv_append_block, and the rectangular causal flash kernel
tribe_attention_extend_fwd, csrc/attention.hip, against the cache plus the block itself).  Inference only, like `forward`.

Independent timelines share one cache through slots: `new_slots(batch_size, max_len)` makes an `EncoderSlots` (the same k / v tensors plus one
position per sequence), and `step_slots(x[B, dim], slots, active)` / `extend_slots(x[B, k, dim], slots, active)` advance any subset of the
slots, each from its own position (tribe_encoder_step_slots_fwd / tribe_encoder_extend_slots_fwd: the launches of `step` / `extend` with
the cache write and the attention in their position-per-sequence forms); `slots.reset([b])` frees a finished slot for the next timeline.
"""

from __future__ import annotations

import logging
import typing as tp

import pydantic
import torch
from torch import nn

from tribe_hip import ops

from .._pack import PackCache, f32c

logger = logging.getLogger(__name__)


class ScaleNorm(nn.Module):
    def __init__(self, dim: int, legacy: bool = False):
        super().__init__()
        self.dim, self.legacy = dim, legacy
        self.g = nn.Parameter(torch.ones(1) * (dim**-0.5 if legacy else 1.0))

    @property
    def gain_scale(self) -> float:
        return 1.0 if self.legacy else self.dim**0.5

    @property
    def eps(self) -> float:
        return 1e-5 if self.legacy else 1e-12


class _Attention(nn.Module):  # parameter holder with the library's names
    def __init__(self, dim: int, heads: int, dim_head: int):
        super().__init__()
        inner = heads * dim_head
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_k = nn.Linear(dim, inner, bias=False)
        self.to_v = nn.Linear(dim, inner, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)


class _FeedForward(nn.Module):
    def __init__(self, dim: int, mult: int):
        super().__init__()
        inner = int(dim * mult)
        self.ff = nn.Sequential(nn.Sequential(nn.Linear(dim, inner), nn.GELU()), nn.Dropout(0.0), nn.Linear(inner, dim))


class _Residual(nn.Module):
    def __init__(self, dim: int, scale_residual: bool):
        super().__init__()
        self.residual_scale = nn.Parameter(torch.ones(dim)) if scale_residual else None


class _Rotary(nn.Module):
    def __init__(self, dim: int, base: float = 10000.0):
        super().__init__()
        self.register_buffer("inv_freq", 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim)))


class EncoderCache:
    """The keys and values of a streamed causal encoder (HipEncoder.new_cache): `k`, `v` bf16 [depth, B, heads, max_len, dim_head] -- the
    rotated k heads and the v heads of every position seen so far, each (layer, sequence, head) one contiguous run -- and `pos`, the
    number of positions filled.  2 * depth * B * heads * max_len * dim_head * 2 bytes."""

    def __init__(self, depth: int, batch_size: int, heads: int, max_len: int, dim_head: int, device: torch.device | str | None):
        shape = (depth, batch_size, heads, max_len, dim_head)
        self.k = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.v = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.pos = 0

    @property
    def batch_size(self) -> int:
        return self.k.shape[1]

    @property
    def max_len(self) -> int:
        return self.k.shape[3]

    @property
    def device(self) -> torch.device:
        return self.k.device

    def reset(self) -> None:
        """Forget every position: the next step is position 0 again.  (The slots are not cleared: nothing at or beyond `pos` is read.)"""
        self.pos = 0


class EncoderSlots:
    """The keys and values of independent timelines streamed through one causal encoder (HipEncoder.new_slots): `k`, `v` as in EncoderCache,
    bf16 [depth, B, heads, max_len, dim_head], and `positions`, the number of positions each of the B slots holds.  A call of
    `step_slots` / `extend_slots` advances any subset of the slots; a finished slot is reset and refilled while the others carry on."""

    def __init__(self, depth: int, batch_size: int, heads: int, max_len: int, dim_head: int, device: torch.device | str | None):
        shape = (depth, batch_size, heads, max_len, dim_head)
        self.k = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.v = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.positions: list[int] = [0] * batch_size

    @property
    def batch_size(self) -> int:
        return self.k.shape[1]

    @property
    def max_len(self) -> int:
        return self.k.shape[3]

    @property
    def device(self) -> torch.device:
        return self.k.device

    def reset(self, slots: tp.Sequence[int] | None = None) -> None:
        """Forget every position of the given slots (None: of all): their next step is position 0 again.  (Nothing is cleared: no cache slot
        at or beyond a position is read.)"""
        B = self.batch_size
        if slots is None:
            self.positions = [0] * B
            return
        for b in slots:
            if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < B:
                raise ValueError(f"EncoderSlots.reset: slot index {b!r} outside [0, {B})")
        for b in slots:
            self.positions[b] = 0

    def select(self, what: str, active: tp.Sequence[int] | tp.Sequence[bool] | None) -> list[bool]:
        """`active` -- None (all slots), slot indices, or a bool sequence of length B -- as one flag per slot."""
        B = self.batch_size
        if active is None:
            return [True] * B
        if isinstance(active, torch.Tensor):
            active = active.tolist()
        active = list(active)
        if active and all(isinstance(a, bool) for a in active):
            if len(active) != B:
                raise ValueError(f"{what}: the active mask holds {len(active)} flags for {B} slots")
            flags = active
        else:
            flags = [False] * B
            for b in active:
                if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < B:
                    raise ValueError(f"{what}: active slot index {b!r} outside [0, {B})")
                flags[b] = True
        if not any(flags):
            raise ValueError(f"{what}: active is empty: a call advances at least one slot")
        return flags


class HipEncoder(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, dim_head: int, ff_mult: int = 4, rotary_pos_emb: bool = True,
                 scale_residual: bool = True, rotary_interleaved: bool = True, legacy_scalenorm: bool = False, ff_dropout: float = 0.0,
                 layer_dropout: float = 0.0, attn_dropout: float = 0.0, causal: bool = False):
        super().__init__()
        self.causal = bool(causal)   # x_transformers' Decoder mask (module docstring); no parameter depends on it
        self.dim, self.depth, self.heads, self.dim_head, self.ff_mult = dim, depth, heads, dim_head, ff_mult
        self.ff_dropout, self.layer_dropout = float(ff_dropout), float(layer_dropout)   # training path only (module docstring)
        self.attn_dropout = float(attn_dropout)
        self.rotary_interleaved = rotary_interleaved
        self.rotary_emb_dim = max(dim_head // 2, 32) if rotary_pos_emb else 0
        if rotary_pos_emb:
            self.rotary_pos_emb = _Rotary(self.rotary_emb_dim)
        layers = []
        for _ in range(depth):
            for kind in ("a", "f"):
                block = _Attention(dim, heads, dim_head) if kind == "a" else _FeedForward(dim, ff_mult)
                layers.append(nn.ModuleList([nn.ModuleList([ScaleNorm(dim, legacy_scalenorm), None, None]), block,
                                             _Residual(dim, scale_residual)]))
        self.layers = nn.ModuleList(layers)
        for i in range(depth):
            self.layers[2 * i + 1][1].ff[1].p = self.ff_dropout
        self.final_norm = ScaleNorm(dim, legacy_scalenorm)
        self._packs = PackCache()

    # -- packed weights ---------------------------------------------------------------------
    def _sources(self) -> list[torch.Tensor | None]:
        return [p for p in self.parameters()]

    def rotary_tables(self, T: int, device: torch.device) -> tuple[torch.Tensor | None, torch.Tensor | None, torch.Tensor | None]:
        """(cos, sin, -sin) f32 [T, rot_dim / 2] for the training path: the same tables EncoderPack.tables builds, WITHOUT packing the weights
        (asking `packed()` for them re-packed every encoder weight after every optimiser step -- 32 casts and 8 f32 q|k|v concatenations
        per step that only the inference entry point needs)."""
        if not self.rotary_emb_dim:
            return None, None, None
        key = (T, device.index or 0)
        cache = self.__dict__.setdefault("_rotary_tabs", {})
        if key not in cache:
            t = torch.arange(T, device=device, dtype=torch.float32)
            freqs = torch.einsum("i,j->ij", t, self.rotary_pos_emb.inv_freq.to(device=device, dtype=torch.float32))
            cos, sin = freqs.cos().contiguous(), freqs.sin().contiguous()
            cache[key] = (cos, sin, (-sin).contiguous())
        return cache[key]

    def packed(self) -> ops.EncoderPack:
        def build() -> ops.EncoderPack:
            pack = ops.EncoderPack(self.dim, self.depth, self.heads, self.dim_head, int(self.dim * self.ff_mult),
                                   self.rotary_emb_dim, self.rotary_interleaved, self.final_norm.gain_scale, self.final_norm.eps,
                                   causal=self.causal)
            keep = pack.keep

            def own(t: torch.Tensor) -> int:
                keep.append(t)
                return t.data_ptr()

            for i in range(self.depth):
                norms_a, attn, ares = self.layers[2 * i]
                norms_f, ff, fres = self.layers[2 * i + 1]
                an, fn = norms_a[0], norms_f[0]
                L = pack.layers[i]
                wqkv = torch.cat([f32c(attn.to_q.weight), f32c(attn.to_k.weight), f32c(attn.to_v.weight)], dim=0)
                L.attn_norm_g = own(f32c(an.g))
                L.w_qkv = own(ops.pack_weight(wqkv))
                L.w_out = own(ops.pack_weight(f32c(attn.to_out.weight)))
                L.attn_res_scale = own(f32c(ares.residual_scale)) if ares.residual_scale is not None else None
                L.ff_norm_g = own(f32c(fn.g))
                L.w_ff1 = own(ops.pack_weight(f32c(ff.ff[0][0].weight)))
                L.b_ff1 = own(f32c(ff.ff[0][0].bias))
                L.w_ff2 = own(ops.pack_weight(f32c(ff.ff[2].weight)))
                L.b_ff2 = own(f32c(ff.ff[2].bias))
                L.ff_res_scale = own(f32c(fres.residual_scale)) if fres.residual_scale is not None else None
            pack.final_norm_g = f32c(self.final_norm.g)
            if self.rotary_emb_dim:
                pack.inv_freq = self.rotary_pos_emb.inv_freq
            return pack

        # one cache slot per mask: a pack built before `causal` was flipped is not served afterwards
        return self._packs.get("enc_causal" if self.causal else "enc", self._sources(), build)

    # -- forward ----------------------------------------------------------------------------
    def forward_tokens(self, x2d: torch.Tensor, B: int, T: int, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B*T, dim], CONSUMED (the residual stream is updated in place) -> y [B*T, dim]."""
        return ops.encoder_fwd(x2d, self.packed(), B, T, out_dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        if D != self.dim:
            raise ValueError(f"HipEncoder: expected last dim {self.dim}, got {D}")
        x2d = x.detach().to(torch.float32).reshape(B * T, D).clone()
        return self.forward_tokens(x2d, B, T, torch.float32).view(B, T, D)

    # -- streaming: one position at a time (causal encoders only) ----------------------------
    def new_cache(self, batch_size: int, max_len: int, device: torch.device | str | None = None) -> EncoderCache:
        """An empty cache for `batch_size` sequences of up to `max_len` positions, on `device` (default: where the parameters are)."""
        self._require_causal("new_cache")
        if batch_size < 1 or max_len < 1:
            raise ValueError(f"HipEncoder.new_cache: batch_size={batch_size} and max_len={max_len} must be positive")
        if device is None:
            device = next(self.parameters()).device
        return EncoderCache(self.depth, batch_size, self.heads, max_len, self.dim_head, device)

    def _require_causal(self, what: str) -> None:
        if not self.causal:
            raise ValueError(f"HipEncoder.{what}: a bidirectional encoder (causal=False) has no incremental form: every output depends on "
                             "the whole window")

    def _check_stream(self, what: str, x: torch.Tensor, cache: EncoderCache, steps: int) -> None:
        self._require_causal(what)
        if not isinstance(cache, EncoderCache):
            raise TypeError(f"HipEncoder.{what}: cache must be an EncoderCache (HipEncoder.new_cache), got {type(cache)}")
        want = (self.depth, cache.batch_size, self.heads, cache.max_len, self.dim_head)
        if tuple(cache.k.shape) != want:
            raise ValueError(f"HipEncoder.{what}: the cache {tuple(cache.k.shape)} was not made for this encoder ({want})")
        if x.shape[0] != cache.batch_size:
            raise ValueError(f"HipEncoder.{what}: batch size {x.shape[0]} does not match the cache's {cache.batch_size}")
        if x.shape[-1] != self.dim:
            raise ValueError(f"HipEncoder.{what}: expected last dim {self.dim}, got {x.shape[-1]}")
        if x.device != cache.device:
            raise ValueError(f"HipEncoder.{what}: x is on {x.device}, the cache on {cache.device}")
        if cache.pos + steps > cache.max_len:
            raise ValueError(f"HipEncoder.{what}: {cache.pos} positions filled + {steps} would run past max_len={cache.max_len}")

    def prefill_tokens(self, x2d: torch.Tensor, B: int, T: int, cache: EncoderCache, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B*T, dim], CONSUMED -> y [B*T, dim]; fills the empty cache with positions 0 .. T-1."""
        y = ops.encoder_prefill(x2d, self.packed(), cache.k, cache.v, T, out_dtype)
        cache.pos = T
        return y

    def step_tokens(self, x2d: torch.Tensor, cache: EncoderCache, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B, dim], CONSUMED -> y [B, dim] at position cache.pos, which advances."""
        y = ops.encoder_step(x2d, self.packed(), cache.k, cache.v, cache.pos, out_dtype)
        cache.pos += 1
        return y

    def prefill(self, x: torch.Tensor, cache: EncoderCache) -> torch.Tensor:
        """x [B, T0, dim] -> y [B, T0, dim]: the causal forward over the first T0 positions, which leaves their keys and values in the
        (empty) cache so that `step` continues at position T0.  Inference only, like `forward` / `forward_tokens`: eval semantics, none of
        attn_dropout, ff_dropout, layer_dropout."""
        if x.ndim != 3:
            raise ValueError(f"HipEncoder.prefill: expected [B, T0, dim], got {tuple(x.shape)}")
        B, T0, D = x.shape
        self._check_stream("prefill", x, cache, T0)
        if cache.pos != 0:
            raise ValueError(f"HipEncoder.prefill: the cache already holds {cache.pos} positions; prefill starts from an empty cache (cache.reset())")
        if T0 < 1:
            raise ValueError("HipEncoder.prefill: T0 must be at least 1")
        x2d = x.detach().to(torch.float32).reshape(B * T0, D).clone()
        return self.prefill_tokens(x2d, B, T0, cache, torch.float32).view(B, T0, D)

    def step(self, x: torch.Tensor, cache: EncoderCache) -> torch.Tensor:
        """x [B, dim], the encoder input at position cache.pos -> y [B, dim], the output there: equal (to rounding) to row cache.pos of
        `forward` on the whole sequence so far, at the cost of one row per GEMM and a matrix-vector attention against the cache.  Advances
        cache.pos.  Inference only, like `forward` / `forward_tokens`: eval semantics, none of attn_dropout, ff_dropout, layer_dropout."""
        if x.ndim != 2:
            raise ValueError(f"HipEncoder.step: expected [B, dim], got {tuple(x.shape)}")
        self._check_stream("step", x, cache, 1)
        x2d = x.detach().to(torch.float32).clone().contiguous()
        return self.step_tokens(x2d, cache, torch.float32)

    def extend_tokens(self, x2d: torch.Tensor, B: int, k: int, cache: EncoderCache, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B*k, dim] (row b*k + t), CONSUMED -> y [B*k, dim] at positions cache.pos .. cache.pos+k-1; cache.pos advances by k."""
        y = ops.encoder_extend(x2d, self.packed(), cache.k, cache.v, cache.pos, k, out_dtype)
        cache.pos += k
        return y

    def extend(self, x: torch.Tensor, cache: EncoderCache) -> torch.Tensor:
        """x [B, k, dim], the encoder inputs at positions cache.pos .. cache.pos+k-1 -> y [B, k, dim], the outputs there: equal (to rounding)
        to those rows of `forward` on the whole sequence so far.  The block goes through every GEMM once (k rows per sequence) and through
        one attention launch per layer against the cache plus itself (tribe_encoder_extend_fwd), where k calls of `step` would stream the
        weights and pay the launches k times.  The cache may be empty (a prefill through this route) or hold any number of positions.
        Advances cache.pos by k.  Inference only, like `forward` / `forward_tokens`: eval semantics, none of attn_dropout, ff_dropout,
        layer_dropout."""
        if x.ndim != 3:
            raise ValueError(f"HipEncoder.extend: expected [B, k, dim], got {tuple(x.shape)}")
        B, k, D = x.shape
        self._check_stream("extend", x, cache, k)
        if k < 1:
            raise ValueError("HipEncoder.extend: k must be at least 1")
        x2d = x.detach().to(torch.float32).reshape(B * k, D).clone()
        return self.extend_tokens(x2d, B, k, cache, torch.float32).view(B, k, D)

    # -- slots: independent timelines in one cache, a position per sequence ------------------
    def new_slots(self, batch_size: int, max_len: int, device: torch.device | str | None = None) -> EncoderSlots:
        """`batch_size` empty slots of up to `max_len` positions each, on `device` (default: where the parameters are)."""
        self._require_causal("new_slots")
        if batch_size < 1 or max_len < 1:
            raise ValueError(f"HipEncoder.new_slots: batch_size={batch_size} and max_len={max_len} must be positive")
        if device is None:
            device = next(self.parameters()).device
        return EncoderSlots(self.depth, batch_size, self.heads, max_len, self.dim_head, device)

    def _check_slots(self, what: str, x: torch.Tensor, slots: EncoderSlots, steps: int, active) -> list[bool]:
        """Validates a slot call before anything is launched; returns one flag per slot."""
        self._require_causal(what)
        if not isinstance(slots, EncoderSlots):
            raise TypeError(f"HipEncoder.{what}: slots must be an EncoderSlots (HipEncoder.new_slots), got {type(slots)}")
        want = (self.depth, slots.batch_size, self.heads, slots.max_len, self.dim_head)
        if tuple(slots.k.shape) != want:
            raise ValueError(f"HipEncoder.{what}: the slots {tuple(slots.k.shape)} were not made for this encoder ({want})")
        if x.shape[0] != slots.batch_size:
            raise ValueError(f"HipEncoder.{what}: batch size {x.shape[0]} does not match the {slots.batch_size} slots")
        if x.shape[-1] != self.dim:
            raise ValueError(f"HipEncoder.{what}: expected last dim {self.dim}, got {x.shape[-1]}")
        if x.device != slots.device:
            raise ValueError(f"HipEncoder.{what}: x is on {x.device}, the slots on {slots.device}")
        return self._select_slots(f"HipEncoder.{what}", slots, steps, active)

    @staticmethod
    def _select_slots(what: str, slots: EncoderSlots, steps: int, active, filled: str = "positions filled") -> list[bool]:
        """One flag per slot for `active`, after checking that every active slot has room for `steps` more positions (the one place this
        is checked: HipEncoder.step_slots / extend_slots and SlotStream.push / push_block all come through here)."""
        if steps < 1:
            raise ValueError(f"{what}: k must be at least 1")
        flags = slots.select(what, active)
        for b, on in enumerate(flags):
            if on and slots.positions[b] + steps > slots.max_len:
                raise ValueError(f"{what}: slot {b}: {slots.positions[b]} {filled} + {steps} would run past max_len={slots.max_len}")
        return flags

    @staticmethod
    def _slot_mask(flags: list[bool], device: torch.device) -> torch.Tensor | None:
        """bool [B, 1] on the device (None: every slot is active), copied without waiting for the device."""
        if all(flags):
            return None
        return torch.tensor(flags, dtype=torch.bool).pin_memory().to(device, non_blocking=True).view(-1, 1)

    def step_slots_tokens(self, x2d: torch.Tensor, slots: EncoderSlots, flags: list[bool],
                          out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B, dim], CONSUMED (finite rows for inactive slots) -> y [B, dim]: active slot b at slots.positions[b], which advances.
        The rows of inactive slots are not meaningful."""
        pos = [p if on else -1 for p, on in zip(slots.positions, flags)]
        y = ops.encoder_step_slots(x2d, self.packed(), slots.k, slots.v, pos, out_dtype)
        slots.positions = [p + 1 if on else p for p, on in zip(slots.positions, flags)]
        return y

    def extend_slots_tokens(self, x2d: torch.Tensor, B: int, k: int, slots: EncoderSlots, flags: list[bool],
                            out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """x2d f32 [B*k, dim] (row b*k + t), CONSUMED -> y [B*k, dim]: active slot b at positions slots.positions[b] .. +k-1; it advances by k."""
        pos = [p if on else -1 for p, on in zip(slots.positions, flags)]
        y = ops.encoder_extend_slots(x2d, self.packed(), slots.k, slots.v, pos, k, out_dtype)
        slots.positions = [p + k if on else p for p, on in zip(slots.positions, flags)]
        return y

    def step_slots(self, x: torch.Tensor, slots: EncoderSlots, active: tp.Sequence[int] | tp.Sequence[bool] | None = None) -> torch.Tensor:
        """x [B, dim] -> y [B, dim]: `step` for independent timelines.  Active slot b (`active`: None = all, slot indices, or a bool sequence
        of length B) is computed at its own position slots.positions[b], which then advances by 1; the rows of inactive slots come back as
        zeros, and their positions and cache runs are untouched.  One call costs what one `step` at this batch size costs
        (tribe_encoder_step_slots_fwd), and does not synchronise the device with the host.  Inference only, like `step`: eval semantics,
        none of attn_dropout, ff_dropout, layer_dropout."""
        if x.ndim != 2:
            raise ValueError(f"HipEncoder.step_slots: expected [B, dim], got {tuple(x.shape)}")
        flags = self._check_slots("step_slots", x, slots, 1, active)
        mask = self._slot_mask(flags, x.device)
        x2d = x.detach().to(torch.float32).clone().contiguous()
        if mask is not None:
            x2d = torch.where(mask, x2d, 0.0)
        y = self.step_slots_tokens(x2d, slots, flags, torch.float32)
        return y if mask is None else torch.where(mask, y, 0.0)

    def extend_slots(self, x: torch.Tensor, slots: EncoderSlots, active: tp.Sequence[int] | tp.Sequence[bool] | None = None) -> torch.Tensor:
        """x [B, k, dim] -> y [B, k, dim]: `extend` for independent timelines -- the next k positions of every active slot, each from its own
        position (tribe_encoder_extend_slots_fwd); k is the same for all slots of a call.  Inactive slots as in `step_slots`.
        Inference only, like `step`."""
        if x.ndim != 3:
            raise ValueError(f"HipEncoder.extend_slots: expected [B, k, dim], got {tuple(x.shape)}")
        B, k, D = x.shape
        flags = self._check_slots("extend_slots", x, slots, k, active)
        mask = self._slot_mask(flags, x.device)
        x3 = x.detach().to(torch.float32).clone()
        if mask is not None:
            x3 = torch.where(mask.view(B, 1, 1), x3, 0.0)
        y = self.extend_slots_tokens(x3.reshape(B * k, D).contiguous(), B, k, slots, flags, torch.float32).view(B, k, D)
        return y if mask is None else torch.where(mask.view(B, 1, 1), y, 0.0)


class TransformerEncoderConfig(pydantic.BaseModel):
    model_config = pydantic.ConfigDict(extra="forbid")
    name: tp.Literal["TransformerEncoder"] = "TransformerEncoder"
    heads: int = 8
    depth: int = 12
    cross_attend: bool = False
    causal: bool = False
    attn_flash: bool = False
    attn_dropout: float = 0.1
    ff_mult: int = 4
    ff_dropout: float = 0.0
    use_scalenorm: bool = True
    use_rmsnorm: bool = False
    rel_pos_bias: bool = False
    alibi_pos_bias: bool = False
    rotary_pos_emb: bool = True
    rotary_xpos: bool = False
    residual_attn: bool = False
    scale_residual: bool = True
    layer_dropout: float = 0.0

    # Not in the reference config: which generation of x_transformers the restated encoder follows
    # (see oracle/xt_encoder.py).  Defaults = the 2.x behaviour.
    rotary_interleaved: bool = True
    legacy_scalenorm: bool = False

    def build(self, dim: int) -> nn.Module:
        if dim % self.heads != 0:
            raise ValueError(f"dim ({dim}) must be divisible by the number of heads ({self.heads})")
        if dim < 256:
            raise ValueError(f"dim ({dim}) is less than 256, which causes weird bug in x-transformers")
        unsupported = {
            "cross_attend": self.cross_attend, "use_rmsnorm": self.use_rmsnorm,
            "rel_pos_bias": self.rel_pos_bias, "alibi_pos_bias": self.alibi_pos_bias, "rotary_xpos": self.rotary_xpos,
            "residual_attn": self.residual_attn, "not use_scalenorm": not self.use_scalenorm,
        }
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"HipEncoder covers the TRIBE configuration only; unsupported options set: {bad}")
        if not 0.0 <= self.ff_dropout < 1.0:
            raise ValueError(f"ff_dropout must satisfy 0 <= p < 1, got {self.ff_dropout}")
        if not 0.0 <= self.layer_dropout <= 1.0:
            raise ValueError(f"layer_dropout must satisfy 0 <= p <= 1, got {self.layer_dropout}")
        if not 0.0 <= self.attn_dropout < 1.0:
            raise ValueError(f"attn_dropout must satisfy 0 <= p < 1, got {self.attn_dropout}")
        # attn_flash selects a kernel, not a result.  attn_dropout / ff_dropout / layer_dropout act on FmriEncoder's autograd training path
        # only (module docstring); the config's default attn_dropout is the reference's 0.1, FmriEncoderConfig's is 0.
        return HipEncoder(dim=dim, depth=self.depth, heads=self.heads, dim_head=dim // self.heads, ff_mult=self.ff_mult,
                          rotary_pos_emb=self.rotary_pos_emb, scale_residual=self.scale_residual,
                          rotary_interleaved=self.rotary_interleaved, legacy_scalenorm=self.legacy_scalenorm,
                          ff_dropout=self.ff_dropout, layer_dropout=self.layer_dropout, attn_dropout=self.attn_dropout,
                          causal=self.causal)
