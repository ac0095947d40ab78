"""Wav2Vec-BERT 2.0 audio feature extractor on MI355X HIP kernels.

Mirror of the reference plugin `Wav2VecBert` (/root/reference/data_utils/data_utils/features/audio.py:27-263): a 30-60 s
waveform chunk is resampled to 16 kHz, z-scored and turned into 160-dim filterbank features by the HF SeamlessM4T
feature extractor (audio.py:222-234; on the host by default, or on the GPU by `HipFbank` = `tribe_fbank_fwd` with
`frontend="hip"`; resampling is scipy's on the host by default, or the reference's julius filter on the GPU by
`tribe_resample_frac_fwd` with `resampler="hip"`; soundfile IO stays on the host);
`Wav2Vec2BertModel(features, output_hidden_states=True)` (audio.py:253-263) yields 25 hidden states `[T@50Hz, 1024]`,
which are resampled to 2 Hz by nearest-neighbour `F.interpolate` (audio.py:163-171) -> `[25, 1024, 2*duration]`.

Here the conformer forward and the resampling run in one C call (`tribe_w2vbert_fwd`): LayerNorm kernels, bf16 MFMA GEMMs
with fused swish / GLU / half-step-residual epilogues, flash attention with the "relative_key" position bias, a fused
causal-depthwise-conv + LayerNorm + swish kernel, and a row gather for the nearest-neighbour resampling.
"""

from __future__ import annotations

import ctypes as C
import typing as tp

import numpy as np
import pydantic
import torch

from tribe_hip import ops
from tribe_hip._lib import ConformerFp8Layer, ConformerLayer, W2vBertDesc
from tribe_hip.ops import (fbank_frame_count, julius_resample_kernels, kaldi_mel_filters, povey_window,  # noqa: F401  (host helpers
                           resample_output_length)                                                       # of the front end)

from .extractor_host import ExtractorHost
from .plugin import HbmFeaturePlugin

# facebook/w2v-bert-2.0 hyper-parameters (public model card; configuration input, not verifiable offline)
W2V_BERT_2 = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                  feature_projection_input_dim=160, hidden_act="swish", position_embeddings_type="relative_key",
                  left_max_position_embeddings=64, right_max_position_embeddings=8, conv_depthwise_kernel_size=31,
                  layer_norm_eps=1e-5)


def nearest_index(t_in: int, t_out: int) -> torch.Tensor:
    """Source index of F.interpolate(mode='nearest') along the last axis: floor(i * t_in / t_out) (audio.py:163-171)."""
    scale = torch.tensor(t_in / t_out, dtype=torch.float32)  # ATen computes the scale in float
    return torch.clamp((torch.arange(t_out, dtype=torch.float32) * scale).floor().to(torch.int64), max=t_in - 1)


class HipWav2Vec2Bert(ExtractorHost):
    """Packed bf16 weights of Wav2Vec2BertModel + the forward-with-resampling launcher.  enable_fp8(calibration_features
    [B, T, feat_dim]) switches the four feed-forward Linears of every layer (70 % of a Conformer layer's GEMM flops) to e4m3; its
    amax table columns are ffn1 in / out, ffn2 in / out."""

    FORWARD, FP8_LAYER, FP8_FIELDS = "tribe_w2vbert_fwd", ConformerFp8Layer, ("w_ffn1_in", "w_ffn1_out", "w_ffn2_in", "w_ffn2_out")
    FP8_SOURCE = "ffn_packs"
    FP8_WIDTHS_ERROR = "fp8 path: hidden_size and intermediate_size must be multiples of 128"

    def __init__(self, config: tp.Any, state_dict: dict[str, torch.Tensor], device: str | torch.device = "cuda"):
        super().__init__(config, state_dict, device)
        g, f32, own = self.cfg, self.f32, self.own
        self.dim, self.depth, self.heads, self.inter = g("hidden_size"), g("num_hidden_layers"), g("num_attention_heads"), g("intermediate_size")
        self.feat_dim, self.kernel = g("feature_projection_input_dim"), g("conv_depthwise_kernel_size")
        self.left, self.right = g("left_max_position_embeddings"), g("right_max_position_embeddings")
        self.eps = float(g("layer_norm_eps"))
        if g("position_embeddings_type") != "relative_key" or g("hidden_act") != "swish":
            raise NotImplementedError("only the w2v-bert-2.0 configuration (relative_key positions, swish) is built")
        self.dim_head = self.dim // self.heads
        self.feat_pad = ops.round_up(self.feat_dim, 64)
        self.fp8_widths = (self.dim, self.inter)
        self.fp_ln = (f32("feature_projection.layer_norm.weight"), f32("feature_projection.layer_norm.bias"))
        self.w_fp = ops.pack_weight(f32("feature_projection.projection.weight"), cols_pad=self.feat_pad)
        self.b_fp = f32("feature_projection.projection.bias")
        self.layers = (ConformerLayer * max(self.depth, 1))()
        self.ffn_packs: list[list[torch.Tensor]] = []     # per layer: bf16 ffn1 in / out, ffn2 in / out (what enable_fp8 quantises)
        H = self.dim
        for i in range(self.depth):
            p = f"encoder.layers.{i}."
            L = self.layers[i]
            self.ffn_packs.append([])
            for tag in ("ffn1", "ffn2"):
                setattr(L, f"{tag}_ln_w", own(f32(p + f"{tag}_layer_norm.weight")))
                setattr(L, f"{tag}_ln_b", own(f32(p + f"{tag}_layer_norm.bias")))
                w_in, w_out = ops.pack_weight(f32(p + f"{tag}.intermediate_dense.weight")), ops.pack_weight(f32(p + f"{tag}.output_dense.weight"))
                self.ffn_packs[-1] += [w_in, w_out]
                setattr(L, f"w_{tag}_in", own(w_in))
                setattr(L, f"b_{tag}_in", own(f32(p + f"{tag}.intermediate_dense.bias")))
                setattr(L, f"w_{tag}_out", own(w_out))
                setattr(L, f"b_{tag}_out_half", own(0.5 * f32(p + f"{tag}.output_dense.bias")))  # x + 0.5 * ffn(x)
            L.attn_ln_w, L.attn_ln_b = own(f32(p + "self_attn_layer_norm.weight")), own(f32(p + "self_attn_layer_norm.bias"))
            a = p + "self_attn."
            L.w_qkv = own(ops.pack_weight(torch.cat([f32(a + "linear_q.weight"), f32(a + "linear_k.weight"), f32(a + "linear_v.weight")])))
            L.b_qkv = own(torch.cat([f32(a + "linear_q.bias"), f32(a + "linear_k.bias"), f32(a + "linear_v.bias")]))
            L.dist_emb = own(ops.pack_weight(f32(a + "distance_embedding.weight")))  # [left+right+1, 64] bf16
            L.w_attn_out, L.b_attn_out = own(ops.pack_weight(f32(a + "linear_out.weight"))), own(f32(a + "linear_out.bias"))
            c = p + "conv_module."
            L.conv_ln_w, L.conv_ln_b = own(f32(c + "layer_norm.weight")), own(f32(c + "layer_norm.bias"))
            pw1 = f32(c + "pointwise_conv1.weight").squeeze(-1)  # [2H, H]: GLU halves a = rows [:H], b = rows [H:]
            L.w_pw1 = own(ops.pack_weight(torch.stack([pw1[:H], pw1[H:]], dim=1).reshape(2 * H, H).contiguous()))  # a0, b0, a1, b1, ...
            L.w_dw_kc = own(f32(c + "depthwise_conv.weight").squeeze(1).t().contiguous())  # [K, H] tap-major
            L.dw_ln_w, L.dw_ln_b = own(f32(c + "depthwise_layer_norm.weight")), own(f32(c + "depthwise_layer_norm.bias"))
            L.w_pw2 = own(ops.pack_weight(f32(c + "pointwise_conv2.weight").squeeze(-1)))
            L.final_ln_w, L.final_ln_b = own(f32(p + "final_layer_norm.weight")), own(f32(p + "final_layer_norm.bias"))
        del self._sd

    def _calibrate(self, calibration_features: torch.Tensor, amax: torch.Tensor) -> None:
        self.hidden_states_resampled(calibration_features, 1, _amax=amax)

    def hidden_states_resampled(self, input_features: torch.Tensor, n_out: int, fp8: bool | None = None,
                                _amax: torch.Tensor | None = None) -> torch.Tensor:
        """input_features f32 [B, T, feat_dim] (unpadded chunks) -> f32 [B, depth + 1, dim, n_out]: every hidden state
        transposed to channels-first and nearest-resampled to n_out time points (audio.py:253-263, 163-171).
        fp8: None = use the e4m3 feed-forward GEMMs when enable_fp8() has run."""
        feats = input_features.to(device=self.device, dtype=torch.float32).contiguous()
        B, T, Fd = feats.shape
        if Fd != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim features, got {Fd}")
        idx = nearest_index(T, n_out).to(self.device)
        d = W2vBertDesc()
        d.B, d.T, d.feat_dim, d.feat_pad = B, T, self.feat_dim, self.feat_pad
        d.dim, d.depth, d.heads, d.dim_head, d.inter, d.conv_kernel = self.dim, self.depth, self.heads, self.dim_head, self.inter, self.kernel
        d.rel_left, d.rel_right, d.ln_eps = self.left, self.right, self.eps
        d.fp_ln_w, d.fp_ln_b = self.fp_ln[0].data_ptr(), self.fp_ln[1].data_ptr()
        d.w_fp, d.b_fp = self.w_fp.data_ptr(), self.b_fp.data_ptr()
        d.layers_host = C.cast(self.layers, C.POINTER(ConformerLayer))
        d.features, d.out_index, d.n_out = feats.data_ptr(), idx.data_ptr(), n_out
        states = torch.empty(self.depth + 1, B, n_out, self.dim, dtype=torch.float32, device=self.device)
        return self._launch(d, states, fp8, _amax, "hidden_states_resampled").permute(1, 0, 3, 2).contiguous()  # [B, n_states, dim, n_out]


class HipFbank:
    """The filterbank front end of w2v-bert-2.0 on the GPU (`ops.w2vbert_fbank`): SeamlessM4TFeatureExtractor at its defaults
    (80 mel bins, stride 2, 16 kHz), usable wherever the plugin takes a `feature_extractor`.  Called like the HF class on ONE
    waveform [n] or [n, channels] (numpy, host or device tensor; a host waveform is uploaded once) or on a list of them; returns
    `{"input_features": f32 [B, T_max, 160] on the GPU, "lengths": each chunk's T}`.  `zscore=True` runs the reference's
    `_preprocess_wav` (channel mean, z-score over the chunk) on the GPU first."""

    def __init__(self, feature_size: int = 80, sampling_rate: int = 16_000, num_mel_bins: int = 80, padding_value: float = 0.0,
                 stride: int = 2, device: str | torch.device = "cuda"):
        if (feature_size, sampling_rate, num_mel_bins, padding_value, stride) != (80, 16_000, 80, 0.0, 2):
            raise NotImplementedError("only the w2v-bert-2.0 front end (80 mel bins, stride 2, 16 kHz, zero padding) is built")
        self.feature_size, self.sampling_rate, self.num_mel_bins, self.padding_value, self.stride = 80, 16_000, 80, 0.0, 2
        self.device = torch.device(device)

    def __call__(self, raw_speech: tp.Any, sampling_rate: int | None = None, zscore: bool = False, **kwargs: tp.Any) -> dict[str, tp.Any]:
        if sampling_rate is not None and sampling_rate != self.sampling_rate:
            raise ValueError(f"HipFbank works at {self.sampling_rate} Hz, got a waveform sampled at {sampling_rate} Hz")
        chunks = list(raw_speech) if isinstance(raw_speech, (list, tuple)) else [raw_speech]
        dev = [torch.as_tensor(c, dtype=torch.float32).to(self.device).contiguous() for c in chunks]
        for c in dev:
            fbank_frame_count(int(c.shape[0]) if c.ndim else 0)          # ValueError below one frame, before anything is launched
        features, lengths = ops.w2vbert_fbank(dev, zscore=zscore)
        return {"input_features": features, "lengths": lengths}


class Wav2VecBert(HbmFeaturePlugin):
    """The reference's audio feature (audio.py:27-263) on the HIP conformer forward: fields `name`, `layers`,
    `layer_aggregation`, `device`, `infra`; `prepare`, `__call__ -> Tensor[L, D, T]`, `_get_data -> [25, 1024, T_event@2Hz]`
    per Sound event (item uid `filepath_offset_duration`, audio.py:145-149).  Waveform IO (`event.read()`) stays on the host as in
    the reference (third-party there too).  `resampler` selects who brings the waveform to 16 kHz: "scipy" (default) is
    `scipy.signal.resample_poly` on the host, as this build always did; "hip" uploads the native-rate waveform once and runs the
    reference's own filter, `julius.resample.ResampleFrac` per channel (audio.py:129-138), on the GPU (`ops.resample_frac`).  The
    two filters differ, so unlike `frontend` this field changes the result: it stays in the class uid and marks the item uid
    (`..._julius`).  julius is not installed here; its filter is restated from its published source, not executed.
    `frontend` selects who turns the 16 kHz waveform into
    `input_features`: "hf" (default) is the reference's route -- `_preprocess_wav` in torch and the HF filterbank extractor on
    the host, then one upload of the features; "hip" uploads the waveform once and runs the channel mean, the z-score and the
    whole filterbank (`HipFbank`) on the GPU, so the features never exist on the host.  Everything from `input_features` on
    -- 24 conformer layers, all 25 hidden states, the nearest-neighbour resampling to 2 Hz -- is one C call either way."""

    name: tp.Literal["Wav2VecBert"] = "Wav2VecBert"
    pretrained: str = "facebook/w2v-bert-2.0"             # audio.py:47,222; resolved from the local HF cache only
    frontend: tp.Literal["hf", "hip"] = "hf"              # a route, not a result: kept out of the class uid like `device`
    resampler: tp.Literal["scipy", "hip"] = "scipy"       # a result: julius' filter ("hip") is not scipy's, see `_item_uid`
    _EVENT_TYPE: tp.ClassVar[str] = "Sound"
    _KIND: tp.ClassVar[str] = "sampled"
    _model: tp.Any = pydantic.PrivateAttr(default=None)
    _feature_extractor: tp.Any = pydantic.PrivateAttr(default=None)

    def attach(self, model: HipWav2Vec2Bert, feature_extractor: tp.Any = None) -> "Wav2VecBert":
        """Provide weights (+ optionally the filterbank front end) explicitly (offline use)."""
        self._model = model
        if feature_extractor is not None:
            self._feature_extractor = feature_extractor
        return self

    @property
    def model(self) -> HipWav2Vec2Bert:
        if self._model is None:
            self._model = self._get_sound_model()
        return self._model

    def _get_sound_model(self) -> HipWav2Vec2Bert:
        from transformers import Wav2Vec2BertModel

        hf = Wav2Vec2BertModel.from_pretrained(self.pretrained, local_files_only=True)
        return HipWav2Vec2Bert(hf.config, hf.state_dict())

    @property
    def feature_extractor(self) -> tp.Any:
        if self._feature_extractor is None:
            self._feature_extractor = self._get_feature_extractor()
        return self._feature_extractor

    @classmethod
    def _exclude_from_cls_uid(cls) -> list[str]:
        return super()._exclude_from_cls_uid() + ["frontend"]

    def _get_feature_extractor(self) -> tp.Any:
        if self.frontend == "hip":
            return HipFbank()
        from transformers import AutoFeatureExtractor, SeamlessM4TFeatureExtractor

        try:
            return AutoFeatureExtractor.from_pretrained(self.pretrained, local_files_only=True)
        except Exception:
            # the checkpoint's preprocessor_config is not cached: the class the model card names, at its defaults
            # (80 mel bins, stride 2 -> 160-dim frames at 50 Hz, 16 kHz); parity with the hub file is unpinned offline
            return SeamlessM4TFeatureExtractor()

    @property
    def _input_frequency(self) -> float:
        return getattr(self.feature_extractor, "sampling_rate", 16_000)

    def _item_uid(self, event: tp.Any) -> str:
        uid = f"{event.filepath}_{event.offset:.2f}_{event.duration:.2f}"
        return uid + "_julius" if self.resampler == "hip" else uid     # the cache is keyed by item uid alone: keep the two filters apart

    def _preprocess_wav(self, wav: torch.Tensor) -> torch.Tensor:
        wav = torch.mean(wav, dim=1)                                   # audio.py:123-127: mono, z-scored
        return (wav - wav.mean()) / (1e-8 + wav.std())

    def _resample_wav(self, wav: torch.Tensor, old_frequency: float, new_frequency: float) -> torch.Tensor:
        """audio.py:129-138 uses julius.ResampleFrac (absent here): same role, scipy's polyphase resampler -- a different
        anti-aliasing filter, so resampled waveforms are parity-unpinned; at equal rates the waveform passes through."""
        old, new = int(old_frequency), int(new_frequency)
        if old == new:
            return wav
        from scipy.signal import resample_poly

        return torch.from_numpy(resample_poly(wav.numpy(), new, old, axis=0).astype("float32"))

    def _get_features(self, wav: torch.Tensor) -> torch.Tensor:
        out = self.feature_extractor(wav.numpy(), return_tensors="pt", sampling_rate=self.feature_extractor.sampling_rate, do_normalize=True)
        try:
            return out["input_features"]
        except KeyError:
            return out["input_values"]

    def _process_wav(self, wav: torch.Tensor, timepoints: int) -> torch.Tensor:
        """audio.py:253-263 + 163-171 in one launch sequence: f32 [n_states, dim, timepoints] on the GPU."""
        return self.model.hidden_states_resampled(self._get_features(wav), timepoints)[0]

    def _process_wav_hip(self, wav: torch.Tensor, timepoints: int) -> torch.Tensor:
        """`_preprocess_wav` + `_get_features` + `_process_wav` without the host: wav f32 [n, channels] is uploaded once."""
        fe = self.feature_extractor
        if not isinstance(fe, HipFbank):
            raise TypeError(f'frontend="hip" needs a HipFbank feature extractor, got {type(fe).__name__}')
        feats = fe(wav.to(self.model.device), sampling_rate=fe.sampling_rate, zscore=True)["input_features"]
        return self.model.hidden_states_resampled(feats, timepoints)[0]

    def _compute(self, events: list[tp.Any]) -> tp.Iterator[np.ndarray]:
        from ..base import Frequency

        for event in events:
            got = event.read()
            if hasattr(got, "audio"):                                   # a Video event: its sound track (audio.py:155-158)
                audio = got.audio
                wav, sfreq = torch.tensor(audio.to_soundarray(), dtype=torch.float32), audio.fps
            else:
                wav, sfreq = torch.as_tensor(got, dtype=torch.float32), event.frequency
            if wav.ndim == 1:
                wav = wav[:, None]
            timepoints = Frequency(2.0).to_ind(event.duration)
            if self.resampler == "hip":                                 # one upload at the native rate; 16 kHz exists on the GPU only
                wav = ops.resample_frac(wav.contiguous().to(self.model.device), int(sfreq), int(self._input_frequency))[0]
                if self.frontend != "hip":
                    wav = wav.cpu()                                     # the HF extractor works on the host
            else:
                wav = self._resample_wav(wav, sfreq, self._input_frequency)
            if self.frontend == "hip":
                yield self._process_wav_hip(wav, timepoints).cpu().numpy()
            else:
                yield self._process_wav(self._preprocess_wav(wav), timepoints).cpu().numpy()
