"""FmriEncoder: trimodal fusion encoder + per-subject voxel head, on MI355X HIP kernels.

Drop-in for /root/reference/algonauts2025/model.py: same config fields and defaults
(`FmriEncoderConfig`, model.py:20-33), same constructor / `build` signature (:35-53), same
module API (`forward(batch, pool_outputs)`, `aggregate_features`, `transformer_forward`,
`compute_contrastive_loss`, ...) and the same parameter names, so `state_dict()` keys
(`projectors.<m>.{weight,bias}`, `predictor.{weights,bias}`, `time_pos_embed`,
`subject_embed.weight`, `encoder.*`, `contrastive_heads.<m>.*`) interchange with the reference.
With the extension `projector_hidden_sizes` every projector and contrastive head is the `Mlp` of `MlpConfig(hidden_sizes=...)` (keys
`projectors.<m>.<i>.{weight,bias}` in torchvision.ops.MLP's order): its hidden blocks run as HIP kernels in front of the same fused
output product; `None`, the default, is the reference's single Linear and launches exactly what it always did.

Data flow of `forward` (every step a HIP launch through libtribe_hip.so, nothing in torch):
  features [B,L,D,T] --tribe_pack_features--> bf16 [B*T, L*D]          (model.py:146-155)
    --tribe_projector_fwd x3 (MFMA GEMM; epilogue = bias + column slice of the fused stream
      + time_pos_embed (+ subject_embed))--> f32 x [B*T, 3072]          (model.py:157-172)
    --tribe_encoder_fwd (8 layers)--> bf16 y [B*T, 3072]                  (model.py:173)
    --tribe_voxel_head_fwd (grouped-by-subject MFMA GEMM)--> f32 [B,V,T]  (model.py:117-118)
    --tribe_adaptive_avg_pool_fwd--> f32 [B,V,T']                          (model.py:119-120)
fp32 master parameters live in torch; bf16 packed copies are cached per parameter version.
In `.eval()` / no-grad mode this fused path runs and records no autograd graph; in `.train()` mode with grad enabled
`forward` composes the same arithmetic from the autograd functions of modeling_utils/autograd.py (HIP forward AND backward).

Dropout (extensions `attn_dropout`, `ff_dropout`, `layer_dropout`, `projector_dropout`; all 0 by default) acts on that autograd training path
only: the fused path applies none, train mode under `no_grad` included (the reference's modules would drop there).  Each training pass with
an active `attn_dropout`, `ff_dropout` or `projector_dropout` draws one key (modeling_utils.models.common.draw_dropout_key: torch's default CPU generator) right
after its modality-dropout draw -- the prediction pass and the contrastive pass each draw their own -- and every mask of the pass is
tribe_dropout_apply's definition with that key and a site:
    encoder feed-forward of layer i          (1 << 56) | i
    attention probabilities of layer i       (4 << 56) | i                    (logical tensor [B * heads * T, T]; drawn inside the
                                                                               softmax-dropout row kernels, see autograd.Attention)
    projector of modality m, hidden block j  (2 << 56) | (m << 16) | j        (m: position in feature_dims;
    contrastive head of m, hidden block j    (3 << 56) | (m << 16) | j         output dropout: j = MLP_OUT_BLOCK = 0xFFFF)
`layer_dropout` follows x_transformers: per sub-layer (attention, then feed-forward, per depth) `random.random() < layer_dropout` skips
norm, block and residual scaling; the draws use Python's `random` and are made only when layer_dropout > 0.  `last_dropout_key` and
`last_layer_drops` keep the last pass's key and skip pattern.  With any of the four active the two passes never share latents.

`causal` (extension, off by default) builds the encoder as x_transformers' Decoder: TR t attends to the stimulus up to t only.  The fused
path gets it through the encoder's pack (tribe_encoder_fwd_ex), the training path hands it to autograd.RotaryAttention / Attention, which
then take the materialised route with the causal row kernels at every attn_dropout; the dropouts above compose with it unchanged.
A causal model can be followed step by step: `stream(batch_size, max_len)` returns an `EncoderStream` whose `push(one stimulus step)` runs
the projectors with row `pos` of time_pos_embed, HipEncoder.step on a KV cache and the voxel head at one time step (eval semantics only).
"""

from __future__ import annotations

import random
import typing as tp

import numpy as np
import pydantic
import torch
from torch import nn

from data_utils.dataloader import SegmentData
from modeling_utils._pack import PackCache, f32c
from modeling_utils.models.common import Mlp, MlpConfig, SubjectLayers, draw_dropout_key
from modeling_utils.models.transformer import TransformerEncoderConfig
from tribe_hip import ops


SITE_FF, SITE_PROJECTOR, SITE_HEAD, SITE_ATTN = 1, 2, 3, 4   # kinds of dropout site (module docstring); 0 = an Mlp used on its own


class FmriEncoderConfig(pydantic.BaseModel):
    model_config = pydantic.ConfigDict(extra="forbid")
    name: tp.Literal["FmriEncoder"] = "FmriEncoder"
    n_subjects: int | None = None
    feature_aggregation: tp.Literal["sum", "cat"] = "cat"
    layer_aggregation: tp.Literal["mean", "cat"] = "cat"
    subject_embedding: bool = False
    modality_dropout: float = 0.0

    contrastive_enabled: bool = False
    contrastive_modalities: list[str] = ["video"]
    contrastive_weight: float = 0.1
    contrastive_temperature: float = 0.07

    # Extensions (absent from the reference, whose model.py hard-codes them at :61, :106, :109-111);
    # the defaults reproduce the reference exactly, smaller values exist for tests.
    hidden: int = 3072
    depth: int = 8
    heads: int = 8
    max_timesteps: int = 1024
    rotary_interleaved: bool = True
    legacy_scalenorm: bool = False
    # training: let the contrastive pass reuse the prediction pass's latents whenever its own dropout draw, the inputs and the
    # parameters coincide (bit-identical loss; False = always re-run the encoder as model.py:228 does)
    share_contrastive_latents: bool = True
    # hidden sizes of every modality projector and contrastive head (MlpConfig.hidden_sizes): Linear -> LayerNorm -> GELU per size in
    # front of the output Linear.  None = the reference's single Linear (model.py:61, 64)
    projector_hidden_sizes: list[int] | None = None
    # dropout of the training path (module docstring): on the encoder's attention probabilities and on its feed-forward hidden
    # (0 <= p < 1 each), x_transformers' stochastic depth per sub-layer (0 <= p <= 1), and MlpConfig.dropout of the MLP projectors /
    # contrastive heads (0 <= p < 1; needs projector_hidden_sizes).  The reference hard-codes all four as 0 (model.py:62, 109-111)
    attn_dropout: float = 0.0
    ff_dropout: float = 0.0
    layer_dropout: float = 0.0
    projector_dropout: float = 0.0
    # causal encoder (TransformerEncoderConfig.causal: TR t sees the stimulus up to t only); the reference leaves the field at its default
    causal: bool = False

    @pydantic.model_validator(mode="after")
    def _check_dropout(self) -> "FmriEncoderConfig":
        if not 0.0 <= self.attn_dropout < 1.0:
            raise ValueError(f"attn_dropout must satisfy 0 <= p < 1, got {self.attn_dropout}")
        if not 0.0 <= self.ff_dropout < 1.0:
            raise ValueError(f"ff_dropout must satisfy 0 <= p < 1, got {self.ff_dropout}")
        if not 0.0 <= self.layer_dropout <= 1.0:
            raise ValueError(f"layer_dropout must satisfy 0 <= p <= 1, got {self.layer_dropout}")
        if not 0.0 <= self.projector_dropout < 1.0:
            raise ValueError(f"projector_dropout must satisfy 0 <= p < 1, got {self.projector_dropout}")
        if self.projector_dropout and not self.projector_hidden_sizes:
            raise ValueError("projector_dropout needs projector_hidden_sizes: the reference's single-Linear projector has no dropout")
        return self

    def build(self, feature_dims: dict[str, tuple[int, int] | None], n_outputs: int, n_output_timesteps: int) -> nn.Module:
        return FmriEncoder(feature_dims, n_outputs, n_output_timesteps, config=self)


class FmriEncoder(nn.Module):
    def __init__(self, feature_dims: dict[str, tuple[int, int] | None], n_outputs: int, n_output_timesteps: int,
                 config: FmriEncoderConfig):
        super().__init__()
        self.config = config
        self.feature_dims = feature_dims
        self.n_outputs = n_outputs
        self.n_output_timesteps = n_output_timesteps
        self.projectors = nn.ModuleDict()
        self.contrastive_heads = nn.ModuleDict()
        hidden = self.hidden = config.hidden
        for index, (modality, tup) in enumerate(feature_dims.items()):
            if tup is None:
                print(f"Warning: {modality} has no feature dimensions. Skipping projector.")
                continue
            num_layers, feature_dim = tup
            input_dim = feature_dim * num_layers if config.layer_aggregation == "cat" else feature_dim
            output_dim = hidden // len(feature_dims) if config.feature_aggregation == "cat" else hidden
            mlp = MlpConfig(norm_layer="layer", activation_layer="gelu", dropout=config.projector_dropout,
                            hidden_sizes=config.projector_hidden_sizes, dropout_backend="hip" if config.projector_dropout else "torch")
            self.projectors[modality] = mlp.build(input_dim, output_dim)
            if config.contrastive_enabled and modality in config.contrastive_modalities:
                self.contrastive_heads[modality] = mlp.build(input_dim, hidden)
            for kind, holder in ((SITE_PROJECTOR, self.projectors), (SITE_HEAD, self.contrastive_heads)):
                if modality in holder and isinstance(holder[modality], Mlp):
                    holder[modality].dropout_site = (kind << 56) | (index << 16)
        self.combiner = nn.Identity()
        self.predictor = SubjectLayers(in_channels=hidden, out_channels=n_outputs, n_subjects=config.n_subjects,
                                       average_subjects=False, bias=True)
        self.time_pos_embed = nn.Parameter(torch.randn(1, config.max_timesteps, hidden))
        if config.subject_embedding:
            self.subject_embed = nn.Embedding(config.n_subjects, hidden)
        self.encoder = TransformerEncoderConfig(attn_dropout=config.attn_dropout, ff_dropout=config.ff_dropout, layer_dropout=config.layer_dropout,
                                                depth=config.depth,
                                                heads=config.heads, rotary_interleaved=config.rotary_interleaved,
                                                legacy_scalenorm=config.legacy_scalenorm, causal=config.causal).build(dim=hidden)
        self._packs = PackCache()
        self.last_dropout_key: int | None = None          # key of the last training pass with an active HIP dropout
        self.last_layer_drops: list[bool] | None = None   # its skipped sub-layers (attention, feed-forward per depth); None: layer_dropout 0
        self._pass_serial = 0
        self._pass_key: int | None = None

    # ------------------------------------------------------------------------------------------
    def _batch_dict(self, batch: SegmentData | dict) -> dict[str, torch.Tensor]:
        return batch.data if hasattr(batch, "data") else batch

    def _pack(self, feat: tp.Any) -> torch.Tensor:
        """features -> bf16 [B*T, K_pad] projector operand (model.py:146-155).  Batches from the GPU segment loader
        (data_utils/gpu_loader.py: `PackedFeature`) already are in that layout and skip the pass."""
        mean = self.config.layer_aggregation == "mean"
        if hasattr(feat, "packed"):
            if not mean or feat.L == 1:
                return feat.packed
            feat = feat.unpack()
        if feat.ndim not in (3, 4):
            raise AssertionError(f"expected [B, L, D, T] or [B, D, T] features, got {tuple(feat.shape)}")
        return ops.pack_features(feat.contiguous(), layer_mean=mean)

    def _packed_linear(self, key: str, lin: nn.Linear) -> tuple[torch.Tensor, torch.Tensor]:
        return self._packs.get(key, [lin.weight, lin.bias], lambda: (ops.pack_weight(f32c(lin.weight)), f32c(lin.bias)))

    @staticmethod
    def _output_linear(proj: nn.Module, packed: torch.Tensor, drop_key: int | None = None) -> tuple[torch.Tensor, nn.Linear]:
        """(bf16 operand, Linear) of a projector's or contrastive head's last product: the packed features and the module itself for
        the reference's single Linear; with projector_hidden_sizes the hidden blocks (Linear -> LayerNorm -> GELU, HIP) run first and
        hand over their bf16 [B*T, H_pad] output.  Differentiable where grad is enabled.  drop_key: the pass key of an active
        projector_dropout (training path only)."""
        if isinstance(proj, Mlp):
            return proj.hidden_operand(packed, drop_key=drop_key), proj.blocks()[1]
        return packed, proj

    def _draw_pass_key(self) -> int | None:
        """The pass key of the HIP dropouts, drawn only when one is active (so at all-zero settings the RNG stream is untouched)."""
        enc = self.encoder   # (the encoder module holds its own rates)
        if enc.ff_dropout > 0 or enc.attn_dropout > 0 or self.config.projector_dropout > 0:
            self.last_dropout_key = draw_dropout_key()
            return self.last_dropout_key
        return None

    def _draw_modality_dropout(self) -> list[str]:
        # model.py:133-141 -- same RNG consumption order as the reference
        drop = []
        for modality in self.feature_dims.keys():
            if torch.rand(1).item() < self.config.modality_dropout and self.training:
                drop.append(modality)
        if len(drop) == len(self.feature_dims):
            drop = list(np.random.choice(drop, len(drop) - 1, replace=False))
        return drop

    def _fused_embed(self, data: dict[str, torch.Tensor], add_embeddings: bool, pos0: int = 0, draw: bool = True, time_pos: bool = True
                     ) -> tuple[torch.Tensor, int, int]:
        """aggregate_features (+ transformer_forward's embedding adds when `add_embeddings`): f32 [B*T, hidden].
        pos0: the position of the first time step (a stream's steps: rows pos0 .. pos0 + T - 1 of time_pos_embed); draw=False: no
        modality-dropout draw (streaming is eval-only and leaves the RNG alone); time_pos=False: the subject embedding only -- the caller
        adds the positional rows itself (SlotStream: one row index per sample)."""
        for modality in data.keys():
            if modality in self.feature_dims:
                break
        ref = data[modality]
        B, T = ref.shape[0], ref.shape[-1]
        device = ref.device
        cat = self.config.feature_aggregation == "cat"
        n_mod = len(self.feature_dims)
        if not cat and any(m not in self.projectors for m in self.feature_dims):
            # reference behaviour: a 3072//n zero block cannot be summed with hidden-wide projections (model.py:143-144,163-164)
            raise RuntimeError(f"The size of tensor a ({self.hidden}) must match the size of tensor b ({self.hidden // n_mod}) "
                               "at non-singleton dimension 2")
        if add_embeddings and time_pos and pos0 + T > self.time_pos_embed.shape[1]:
            raise RuntimeError(f"sequence length {pos0 + T} exceeds the positional table ({self.time_pos_embed.shape[1]})")
        dropped = self._draw_modality_dropout() if draw else []
        pos = f32c(self.time_pos_embed)[0][pos0:] if add_embeddings and time_pos else None
        semb, sid = None, None
        if add_embeddings and hasattr(self, "subject_embed"):
            semb = f32c(self.subject_embed.weight)
            # the projector epilogue gathers subject_embed rows by this index with no bounds check on the device:
            # validate 0 <= id < n_subjects here (nn.Embedding raises IndexError in the reference, model.py:171-172)
            sid = self.predictor.check_subjects(data["subject_id"])
            if self.predictor.average_subjects:
                sid = data["subject_id"].flatten().to(torch.int64).contiguous()
        width = (self.hidden // n_mod) * n_mod if cat else self.hidden
        x = torch.empty(B * T, width, dtype=torch.float32, device=device)
        slot = self.hidden // n_mod
        first = True
        for i, modality in enumerate(self.feature_dims.keys()):
            col0 = i * slot if cat else 0
            n_out = slot if cat else self.hidden
            emb = (pos, semb, sid) if (cat or first) else (None, None, None)  # 'sum': embeddings are added once
            if modality not in self.projectors or modality in dropped:
                if cat or first:
                    ops.projector_zero_fwd(B * T, T, n_out, x, col0, *emb)
                # 'sum' with a dropped non-first modality contributes nothing
            else:
                feat = data[modality]
                if feat.ndim not in (3, 4):
                    raise AssertionError(f"expected [B, L, D, T] or [B, D, T] features, got {tuple(feat.shape)}")
                with torch.no_grad():
                    packed, lin = self._output_linear(self.projectors[modality], self._pack(feat))
                w, b = self._packed_linear(f"proj.{modality}", lin)
                ops.projector_fwd(packed, T, w, b, n_out, x, col0, accumulate=(not cat and not first), pos_embed=emb[0],
                                  subj_embed=emb[1], subject_id=emb[2])
            first = False
        return x, B, T

    # -- reference API ---------------------------------------------------------------------------
    def aggregate_features(self, batch: SegmentData | dict) -> torch.Tensor:
        """model.py:125-165 -> f32 [B, T, hidden]."""
        x, B, T = self._fused_embed(self._batch_dict(batch), add_embeddings=False)
        return x.view(B, T, -1)

    def transformer_forward(self, x: torch.Tensor, subject_id: torch.Tensor | None = None) -> torch.Tensor:
        """model.py:167-174 on an explicit [B, T, hidden] tensor (the fused `forward` never takes this detour)."""
        x = x + self.time_pos_embed[:, : x.size(1)].to(x.device)
        if hasattr(self, "subject_embed"):
            x = x + self.subject_embed(subject_id)
        return self.encoder(x)

    def _latents(self, data: dict[str, torch.Tensor], out_dtype: torch.dtype) -> tuple[torch.Tensor, int, int]:
        x, B, T = self._fused_embed(data, add_embeddings=True)
        return self.encoder.forward_tokens(x, B, T, out_dtype), B, T

    # -- training path: same arithmetic, every op an autograd function whose forward AND backward are HIP kernels ----
    def _wants_grad(self) -> bool:
        # Lightning runs training_step in train mode with grad enabled; evaluation (.eval()) keeps the fused fast path
        return self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _latents_key(self, data: dict[str, torch.Tensor], dropped: list[str]) -> tuple:
        """Everything the latents of a training pass depend on: the inputs (storage, version, shape), the modality-dropout draw and the
        version of every parameter -- two passes with equal keys compute bit-identical latents (the kernels are deterministic)."""
        inputs = tuple((k, v.data_ptr(), v._version, tuple(v.shape)) for k, v in data.items()
                       if (k in self.feature_dims or k == "subject_id") and isinstance(v, torch.Tensor))
        return inputs, tuple(dropped), tuple(p._version for p in self.parameters())

    def _latents_autograd(self, data: dict[str, torch.Tensor], share: str = "") -> tuple[torch.Tensor, int, int]:
        """aggregate_features + transformer_forward up to (not including) the final ScaleNorm: f32 [B*T, hidden].

        `share`: the reference's training step runs the encoder TWICE -- once for the prediction (model.py:113-123) and once more
        inside compute_contrastive_loss -> get_brain_latents (model.py:177-182, 228), each with its own modality-dropout draw.
        Whenever the two draws coincide (always at modality_dropout == 0; 19.5 % of the steps at the default 0.3 with three
        modalities) the second pass recomputes the first bit for bit.  The prediction pass ("produce") therefore leaves its latents
        behind and the contrastive pass ("consume") -- after drawing ITS dropout set from the same RNG stream the reference
        consumes -- takes them when inputs, draw and parameter versions all match, and recomputes otherwise.  The loss is
        bit-identical either way; autograd sums the two branches' gradients at the shared node."""
        dropped = self._draw_modality_dropout()
        self._pass_key = self._draw_pass_key()
        key = self._latents_key(data, dropped) if share else None
        if key is not None and (self._pass_key is not None or self.encoder.layer_dropout > 0):
            self._pass_serial += 1
            key = key + (self._pass_serial,)   # a stochastic pass: no two have equal latents
        if share == "consume":
            kept, self._shared_latents = getattr(self, "_shared_latents", None), None
            if kept is not None and kept[0] == key and self.config.share_contrastive_latents:
                self.shared_latent_hits = getattr(self, "shared_latent_hits", 0) + 1
                return kept[1]
        out = self._latents_autograd_compute(data, dropped)
        self._shared_latents = (key, out) if share == "produce" else None
        return out

    def _latents_autograd_compute(self, data: dict[str, torch.Tensor], dropped: list[str]) -> tuple[torch.Tensor, int, int]:
        from modeling_utils import autograd as ag

        cfg = self.config
        cat = cfg.feature_aggregation == "cat"
        for modality in data.keys():
            if modality in self.feature_dims:
                break
        ref = data[modality]
        B, T = ref.shape[0], ref.shape[-1]
        n_mod = len(self.feature_dims)
        slot = self.hidden // n_mod if cat else self.hidden
        if not cat and any(m not in self.projectors for m in self.feature_dims):
            # reference behaviour: a hidden // n zero block cannot be summed with hidden-wide projections (model.py:143-144,163-164)
            raise RuntimeError(f"The size of tensor a ({self.hidden}) must match the size of tensor b ({self.hidden // n_mod}) "
                               "at non-singleton dimension 2")
        slices = []
        pkey = self._pass_key if cfg.projector_dropout > 0 else None
        for m in self.feature_dims.keys():
            if m not in self.projectors or m in dropped:  # model.py:143-144,158-159: zero block, no gradient
                slices.append(torch.zeros(B * T, slot, dtype=torch.float32, device=ref.device))
                continue
            packed, lin = self._output_linear(self.projectors[m], self._pack(data[m]), pkey)
            if lin is self.projectors[m]:
                slices.append(ag.ProjectorFuse.apply(packed, lin.weight, lin.bias))
            else:   # behind hidden blocks the operand needs its gradient
                slices.append(self.projectors[m].output(packed, pkey))
        if cat:
            x = torch.cat(slices, dim=1).view(B, T, n_mod * slot)   # model.py:161-162
        else:
            x = slices[0]
            for extra in slices[1:]:                                # model.py:163-164: sum(tensors)
                x = x + extra
            x = x.view(B, T, slot)
        x = x + self.time_pos_embed[:, :T]                      # model.py:169-170 (autograd sums the rows over the batch)
        subject_id = data["subject_id"]
        if hasattr(self, "subject_embed"):
            x = x + self.subject_embed(subject_id)              # model.py:171-172
        x = x.reshape(B * T, -1).contiguous()
        enc = self.encoder
        cos, sin, neg_sin = enc.rotary_tables(T, x.device)     # neg_sin: the backward's rotation by -theta
        gs, eps = enc.final_norm.gain_scale, enc.final_norm.eps
        scale = enc.dim_head**-0.5
        # x_transformers' stochastic depth: one random.random() per sub-layer, in layer order, only when layer_dropout > 0
        drops = [random.random() < enc.layer_dropout for _ in range(2 * enc.depth)] if enc.layer_dropout > 0 else None
        self.last_layer_drops = drops
        fkey = self._pass_key if enc.ff_dropout > 0 else None
        akey = self._pass_key if enc.attn_dropout > 0 else None
        for i in range(enc.depth):
            norms_a, attn, res_a = enc.layers[2 * i]
            norms_f, ff, res_f = enc.layers[2 * i + 1]
            if not (drops and drops[2 * i]):        # a skipped sub-layer leaves x as it is: no norm, no block, no residual scaling
                # the block input forks into norm(x) and the scaled residual; ScaleNormFork's backward sums the two gradients in its own kernel
                xn, xr = ag.ScaleNormFork.apply(x, norms_a[0].g, gs, eps, res_a.residual_scale)
                qkv = ag.QKVLinear.apply(xn, attn.to_q.weight, attn.to_k.weight, attn.to_v.weight)
                adrop = () if akey is None else (enc.attn_dropout, akey, (SITE_ATTN << 56) | i)
                if enc.causal:   # the trailing argument of both functions: the mask takes the materialised route at every p
                    adrop = (adrop or (0.0, 0, 0)) + (True,)
                if enc.rotary_emb_dim:
                    ao, _ = ag.RotaryAttention.apply(qkv, cos, sin, neg_sin, B, T, enc.heads, enc.dim_head, scale, enc.rotary_emb_dim,
                                                     enc.rotary_interleaved, *adrop)
                else:
                    ao = ag.Attention.apply(qkv, B, T, enc.heads, enc.dim_head, scale, *adrop)
                x = ag.Linear.apply(ao, attn.to_out.weight, None, xr, res_a.residual_scale, True, True)
            if not (drops and drops[2 * i + 1]):
                xn, xr = ag.ScaleNormFork.apply(x, norms_f[0].g, gs, eps, res_f.residual_scale)
                args = (xn, ff.ff[0][0].weight, ff.ff[0][0].bias, ff.ff[2].weight, ff.ff[2].bias, xr, res_f.residual_scale, True)
                if fkey is not None:
                    args += (ff.ff[1].p, fkey, (SITE_FF << 56) | i)
                x = ag.FeedForward.apply(*args)
        return x, B, T

    def _forward_autograd(self, data: dict[str, torch.Tensor], pool_outputs: bool) -> torch.Tensor:
        from modeling_utils import autograd as ag

        x, B, T = self._latents_autograd(data, share="produce" if self.config.contrastive_enabled else "")
        enc = self.encoder
        y = ag.ScaleNorm.apply(x, enc.final_norm.g, enc.final_norm.gain_scale, enc.final_norm.eps)
        out = ag.VoxelHead.apply(y.view(B, T, -1), self.predictor.weights, self.predictor.bias,
                                 self.predictor.check_subjects(data["subject_id"]))
        if pool_outputs and T != self.n_output_timesteps:
            out = ag.AdaptivePool.apply(out, self.n_output_timesteps)
        return out

    def forward(self, batch: SegmentData | dict, pool_outputs: bool = True) -> torch.Tensor:
        data = self._batch_dict(batch)
        if self._wants_grad():
            return self._forward_autograd(data, pool_outputs)
        with torch.no_grad():
            return self._forward_inference(data, pool_outputs)

    def _forward_inference(self, data: dict[str, torch.Tensor], pool_outputs: bool = True) -> torch.Tensor:
        y, B, T = self._latents(data, torch.bfloat16)  # [B*T, hidden] bf16, final-normed
        out = self.predictor.forward_tokens(y.view(B, T, -1), data["subject_id"])  # [B, V, T] f32
        if pool_outputs and T != self.n_output_timesteps:  # AdaptiveAvgPool1d(T)(x[..., T]) is the identity
            out = ops.adaptive_avg_pool(out, self.n_output_timesteps)
        return out

    # --- streaming (causal encoders): one stimulus step at a time ------------------------------------
    def stream(self, batch_size: int, max_len: int | None = None, independent: bool = False) -> "EncoderStream | SlotStream":
        """A stream of `batch_size` timelines of up to `max_len` stimulus steps (None: config.max_timesteps) through this model:
        EncoderStream.push(one step) -> the prediction at that step.  Needs `causal=True`.  independent=True: a SlotStream, whose
        timelines start, advance and end independently of each other (one position per slot)."""
        max_len = self.config.max_timesteps if max_len is None else max_len
        if max_len > self.time_pos_embed.shape[1]:
            raise ValueError(f"FmriEncoder.stream: max_len={max_len} exceeds the positional table ({self.time_pos_embed.shape[1]} steps)")
        if independent:
            return SlotStream(self, batch_size, max_len)
        return EncoderStream(self, batch_size, max_len)

    # --- contrastive alignment helpers (model.py:177-241) -----------------------------------------
    @torch.no_grad()
    def get_brain_latents(self, batch: SegmentData | dict) -> torch.Tensor:
        y, B, T = self._latents(self._batch_dict(batch), torch.float32)
        return y.view(B, T, -1)

    @torch.no_grad()
    def get_modality_latents(self, batch: SegmentData | dict, modality: str) -> torch.Tensor:
        assert modality in self.contrastive_heads, f"No contrastive head found for modality '{modality}'"
        data = self._batch_dict(batch)
        feat = data.get(modality, None)
        if feat is None:
            raise KeyError(f"Modality '{modality}' not found in batch.data")
        B, T = feat.shape[0], feat.shape[-1]
        packed, lin = self._output_linear(self.contrastive_heads[modality], self._pack(feat))
        w, b = self._packed_linear(f"chead.{modality}", lin)
        out = torch.empty(B * T, self.hidden, dtype=torch.float32, device=feat.device)
        ops.projector_fwd(packed, T, w, b, self.hidden, out, 0, False, None, None, None)
        return out.view(B, T, -1)

    @staticmethod
    def _info_nce(q: torch.Tensor, k: torch.Tensor, tau: float = 0.07) -> torch.Tensor:
        """model.py:208-221: symmetric InfoNCE over flattened [B, T, H] sequences (HIP: row normalisation, logits MFMA
        GEMM, log-sum-exp kernels; differentiable through modeling_utils.autograd.InfoNCE)."""
        from modeling_utils import autograd as ag

        bt, h = q.shape[0] * q.shape[1], q.shape[2]
        return ag.InfoNCE.apply(q.reshape(bt, h).float().contiguous(), k.reshape(bt, h).float().contiguous(), tau)

    def _contrastive_autograd(self, data: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        """model.py:223-241 on the training path: a SECOND pass through aggregate_features + encoder (fresh
        modality-dropout draws, as the reference's get_brain_latents does, model.py:177-182,228), the contrastive heads
        and the symmetric InfoNCE -- all differentiable HIP functions."""
        from modeling_utils import autograd as ag

        x, B, T = self._latents_autograd(data, share="consume")
        hkey = self._pass_key if self.config.projector_dropout > 0 else None   # the contrastive pass's own key
        enc = self.encoder
        brain = ag.ScaleNorm.apply(x, enc.final_norm.g, enc.final_norm.gain_scale, enc.final_norm.eps, True)  # f32 [B*T, H]
        losses: dict[str, torch.Tensor] = {}
        for modality in self.config.contrastive_modalities:
            if modality not in self.contrastive_heads or modality not in data:
                continue
            feat = data[modality]
            packed, head = self._output_linear(self.contrastive_heads[modality], self._pack(feat), hkey)
            if head is self.contrastive_heads[modality]:
                lat = ag.ProjectorFuse.apply(packed, head.weight, head.bias)        # f32 [B * T_mod, hidden]
            else:
                lat = self.contrastive_heads[modality].output(packed, hkey)
            T_mod = feat.shape[-1]
            if T_mod != T:   # model.py:234-238: adaptive average pool of the modality latents to the brain's time axis
                lat = lat.view(B, T_mod, -1).transpose(1, 2).contiguous()           # [B, hidden, T_mod]
                lat = ag.AdaptivePool.apply(lat, T).transpose(1, 2).reshape(B * T, -1).contiguous()
            losses[modality] = ag.InfoNCE.apply(brain, lat, self.config.contrastive_temperature)
        return losses

    def compute_contrastive_loss(self, batch: SegmentData | dict) -> dict[str, torch.Tensor]:
        if not self.config.contrastive_enabled:
            return {}
        data = self._batch_dict(batch)
        if self._wants_grad():
            return self._contrastive_autograd(data)
        brain = self.get_brain_latents(batch)
        losses: dict[str, torch.Tensor] = {}
        for modality in self.config.contrastive_modalities:
            if modality not in self.contrastive_heads or modality not in data:
                continue
            lat = self.get_modality_latents(batch, modality)
            if lat.size(1) != brain.size(1):
                lat = ops.adaptive_avg_pool(lat.transpose(1, 2).contiguous(), brain.size(1)).transpose(1, 2)
            losses[modality] = self._info_nce(brain, lat, tau=self.config.contrastive_temperature)
        return losses


class EncoderStream:
    """A causal FmriEncoder followed step by step (FmriEncoder.stream): the encoder's keys and values of the steps seen so far live in an
    EncoderCache, so a new 0.5 s stimulus step costs one row per GEMM and a matrix-vector attention instead of a forward over the window.

    Outputs are on the un-pooled stimulus grid (`forward(batch, pool_outputs=False)`'s columns): adaptive pooling to TRs needs the whole
    window and stays with the caller.  Inference only: eval semantics whatever `model.training` says -- no modality dropout, none of the
    encoder's or projectors' dropouts, no autograd graph.  The voxel head runs its usual form (rows = voxels of the sample's subject,
    N = T = 1 column)."""

    def __init__(self, model: FmriEncoder, batch_size: int, max_len: int):
        self.model = model
        self.cache = model.encoder.new_cache(batch_size, max_len, model.time_pos_embed.device)

    @property
    def pos(self) -> int:
        return self.cache.pos

    def reset(self) -> None:
        self.cache.reset()

    def _steps(self, what: str, data: dict[str, torch.Tensor], one: bool) -> int:
        """Validates a push / prefill batch before anything is launched; returns its number of time steps."""
        T = None
        for modality in self.model.feature_dims:
            feat = data.get(modality) if modality in self.model.projectors else None
            if feat is None:
                continue
            if feat.ndim not in (3, 4):
                raise ValueError(f"EncoderStream.{what}: {modality}: expected [B, L, D, T] or [B, D, T] features, got {tuple(feat.shape)}")
            if feat.shape[0] != self.cache.batch_size:
                raise ValueError(f"EncoderStream.{what}: {modality}: batch size {feat.shape[0]} does not match the stream's {self.cache.batch_size}")
            if feat.device != self.cache.device:
                raise ValueError(f"EncoderStream.{what}: {modality} is on {feat.device}, the stream on {self.cache.device}")
            if T is not None and feat.shape[-1] != T:
                raise ValueError(f"EncoderStream.{what}: modalities disagree on the number of time steps ({T} vs {feat.shape[-1]})")
            T = feat.shape[-1]
        if T is None:
            raise ValueError(f"EncoderStream.{what}: the batch holds none of the modalities {list(self.model.projectors)}")
        if one and T != 1:
            raise ValueError(f"EncoderStream.{what}: expected one time step per call ([B, L, D, 1] or [B, D, 1]), got {T}")
        if self.cache.pos + T > self.cache.max_len:
            raise ValueError(f"EncoderStream.{what}: {self.cache.pos} steps seen + {T} would run past max_len={self.cache.max_len}")
        return T

    @torch.no_grad()
    def push(self, data: SegmentData | dict) -> torch.Tensor:
        """One stimulus step of every timeline: each modality [B, L, D, 1] or [B, D, 1], plus `subject_id` -> f32 [B, n_outputs], the
        prediction at this step given the steps pushed so far."""
        model = self.model
        data = model._batch_dict(data)
        self._steps("push", data, one=True)
        x, B, _ = model._fused_embed(data, add_embeddings=True, pos0=self.cache.pos, draw=False)
        model.encoder._check_stream("step", x, self.cache, 1)
        y = model.encoder.step_tokens(x, self.cache, torch.bfloat16)
        return model.predictor.forward_tokens(y.view(B, 1, -1), data["subject_id"])[:, :, 0]

    @torch.no_grad()
    def push_block(self, data: SegmentData | dict) -> torch.Tensor:
        """The next k stimulus steps of every timeline at once, onto a stream that holds any number of steps: each modality [B, L, D, k] or
        [B, D, k], plus `subject_id` -> f32 [B, n_outputs, k], the predictions at steps pos .. pos+k-1.  What k calls of `push` give (to
        rounding), with every GEMM and one attention launch per layer run once for the block (HipEncoder.extend)."""
        model = self.model
        data = model._batch_dict(data)
        k = self._steps("push_block", data, one=False)
        x, B, _ = model._fused_embed(data, add_embeddings=True, pos0=self.cache.pos, draw=False)   # positional rows pos .. pos+k-1
        model.encoder._check_stream("extend", x.view(B, k, -1), self.cache, k)
        y = model.encoder.extend_tokens(x, B, k, self.cache, torch.bfloat16)
        return model.predictor.forward_tokens(y.view(B, k, -1), data["subject_id"])

    @torch.no_grad()
    def prefill(self, data: SegmentData | dict) -> torch.Tensor:
        """The first T0 steps at once, into an empty stream: each modality [B, L, D, T0] or [B, D, T0] -> f32 [B, n_outputs, T0]; `push`
        continues at step T0."""
        model = self.model
        data = model._batch_dict(data)
        if self.cache.pos != 0:
            raise ValueError(f"EncoderStream.prefill: the stream already holds {self.cache.pos} steps; prefill starts from an empty one (reset())")
        T = self._steps("prefill", data, one=False)
        x, B, _ = model._fused_embed(data, add_embeddings=True, draw=False)
        model.encoder._check_stream("prefill", x.view(B, T, -1), self.cache, T)
        y = model.encoder.prefill_tokens(x, B, T, self.cache, torch.bfloat16)
        return model.predictor.forward_tokens(y.view(B, T, -1), data["subject_id"])


class SlotStream:
    """Independent timelines through one causal FmriEncoder (FmriEncoder.stream(..., independent=True)): every one of the B slots has its own
    position, a call advances any subset of them, and a finished slot is reset and refilled while the others carry on -- at the cost of one
    step at batch size B per call (HipEncoder.step_slots / extend_slots on an EncoderSlots), where B separate streams pay every launch B
    times.  Each slot's positional row is its own: time_pos_embed[0, positions[b] + t].

    Outputs as EncoderStream's (the un-pooled stimulus grid; inference only); the rows of inactive slots are zeros.  `subject_id` and
    every modality are given for all B slots in every call; what an inactive slot holds is not read into any result."""

    def __init__(self, model: FmriEncoder, batch_size: int, max_len: int):
        self.model = model
        self.slots = model.encoder.new_slots(batch_size, max_len, model.time_pos_embed.device)

    @property
    def positions(self) -> list[int]:
        return list(self.slots.positions)

    def reset(self, slots: tp.Sequence[int] | None = None) -> None:
        self.slots.reset(slots)

    def _steps(self, what: str, data: dict[str, torch.Tensor], one: bool, active) -> tuple[int, list[bool]]:
        """Validates a push batch before anything is launched; returns its number of time steps and one flag per slot."""
        B, T = self.slots.batch_size, None
        for modality in self.model.feature_dims:
            feat = data.get(modality) if modality in self.model.projectors else None
            if feat is None:
                continue
            if feat.ndim not in (3, 4):
                raise ValueError(f"SlotStream.{what}: {modality}: expected [B, L, D, T] or [B, D, T] features, got {tuple(feat.shape)}")
            if feat.shape[0] != B:
                raise ValueError(f"SlotStream.{what}: {modality}: batch size {feat.shape[0]} does not match the stream's {B} slots")
            if feat.device != self.slots.device:
                raise ValueError(f"SlotStream.{what}: {modality} is on {feat.device}, the stream on {self.slots.device}")
            if T is not None and feat.shape[-1] != T:
                raise ValueError(f"SlotStream.{what}: modalities disagree on the number of time steps ({T} vs {feat.shape[-1]})")
            T = feat.shape[-1]
        if T is None:
            raise ValueError(f"SlotStream.{what}: the batch holds none of the modalities {list(self.model.projectors)}")
        if one and T != 1:
            raise ValueError(f"SlotStream.{what}: expected one time step per call ([B, L, D, 1] or [B, D, 1]), got {T}")
        return T, self.model.encoder._select_slots(f"SlotStream.{what}", self.slots, T, active, filled="steps seen")

    def _embed(self, data: dict[str, torch.Tensor], k: int, flags: list[bool]) -> tuple[torch.Tensor, torch.Tensor | None]:
        """f32 [B*k, hidden] encoder input: projectors + subject embedding as in EncoderStream, plus row positions[b] + t of time_pos_embed
        for sample b (gathered: one index_select and an add); the rows of inactive slots are zeros.  Also the bool [B, 1] slot mask (None:
        all active).  Index and mask reach the device through pinned memory on the current stream: no synchronisation."""
        model, device = self.model, self.slots.device
        x, B, _ = model._fused_embed(data, add_embeddings=True, draw=False, time_pos=False)
        rows = [(p if on else 0) + t for p, on in zip(self.slots.positions, flags) for t in range(k)]
        index = torch.tensor(rows, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        x += f32c(model.time_pos_embed)[0].index_select(0, index)[:, : x.shape[1]]
        mask = model.encoder._slot_mask(flags, device)
        if mask is not None:
            x = torch.where(mask.repeat_interleave(k, 0), x, 0.0)
        return x, mask

    @torch.no_grad()
    def push(self, data: SegmentData | dict, active: tp.Sequence[int] | tp.Sequence[bool] | None = None) -> torch.Tensor:
        """One stimulus step of every active slot (`active`: None = all, slot indices, or a bool sequence of length B): each modality
        [B, L, D, 1] or [B, D, 1], plus `subject_id` -> f32 [B, n_outputs], the prediction of slot b at its own step positions[b] given the
        steps pushed into that slot since its last reset.  Rows of inactive slots are zeros."""
        model = self.model
        data = model._batch_dict(data)
        _, flags = self._steps("push", data, True, active)
        x, mask = self._embed(data, 1, flags)   # [B, hidden] on the slots' device by construction (_steps)
        y = model.encoder.step_slots_tokens(x, self.slots, flags, torch.bfloat16)
        out = model.predictor.forward_tokens(y.view(len(flags), 1, -1), data["subject_id"])[:, :, 0]
        return out if mask is None else torch.where(mask, out, 0.0)

    @torch.no_grad()
    def push_block(self, data: SegmentData | dict, active: tp.Sequence[int] | tp.Sequence[bool] | None = None) -> torch.Tensor:
        """The next k stimulus steps of every active slot at once: each modality [B, L, D, k] or [B, D, k], plus `subject_id` -> f32
        [B, n_outputs, k], the predictions of slot b at its steps positions[b] .. positions[b]+k-1.  k is the same for all slots of a
        call.  Rows of inactive slots are zeros."""
        model = self.model
        data = model._batch_dict(data)
        k, flags = self._steps("push_block", data, False, active)
        B = len(flags)
        x, mask = self._embed(data, k, flags)
        y = model.encoder.extend_slots_tokens(x, B, k, self.slots, flags, torch.bfloat16)
        out = model.predictor.forward_tokens(y.view(B, k, -1), data["subject_id"])
        return out if mask is None else torch.where(mask.view(B, 1, 1), out, 0.0)
