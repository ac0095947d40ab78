"""What the three frozen extractor hosts (HipLlamaModel, HipVJEPA2Encoder, HipWav2Vec2Bert) share: reading a config and a state
dict, owning the device tensors a layer table points to, the e4m3 calibration and the tail of every forward (fp8 choice, workspace,
launch on the current stream).  A subclass supplies its weight-name table, its descriptor and the class attributes below."""

from __future__ import annotations

import ctypes as C
import math
import typing as tp

import torch

from tribe_hip import ops
from tribe_hip._lib import check, lib


class ExtractorHost:
    FORWARD: str                       # C entry point; its workspace planner is FORWARD with "_fwd" -> "_workspace_bytes"
    FP8_LAYER: type[C.Structure]       # struct of one layer's e4m3 weights: FP8_FIELDS, then w_scale[4] and in_scale[4]
    FP8_FIELDS: tuple[str, str, str, str]
    FP8_SOURCE = "packs"               # attribute holding, per layer, the four bf16 packs enable_fp8 quantises, in FP8_FIELDS order
    FP8_WIDTHS_ERROR: str              # raised by enable_fp8 unless every entry of self.fp8_widths is a multiple of 128
    MISSING_WEIGHTS_ARE_NONE = False   # f32() of a name the state dict lacks: None (optional biases) instead of a KeyError

    def __init__(self, config: tp.Any, state_dict: dict[str, torch.Tensor], device: str | torch.device):
        """The subclass constructor runs this first and ends with `del self._sd`: f32() is for construction only."""
        self.cfg = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
        self.device = torch.device(device)
        self._sd = state_dict
        self.keep: list[torch.Tensor] = []   # owns every tensor a layer table refers to
        self.fp8_layers = None               # FP8_LAYER array once enable_fp8() has run
        self.fp8_widths: tuple[int, ...] = ()

    def f32(self, name: str) -> torch.Tensor | None:
        if self.MISSING_WEIGHTS_ARE_NONE and name not in self._sd:
            return None
        return self._sd[name].detach().to(device=self.device, dtype=torch.float32).contiguous()

    def own(self, t: torch.Tensor | None) -> int | None:
        if t is None:
            return None
        self.keep.append(t)
        return t.data_ptr()

    def _calibrate(self, calibration: torch.Tensor, amax: torch.Tensor) -> None:
        """One bf16 forward over `calibration` with `_amax=amax`."""
        raise NotImplementedError

    def enable_fp8(self, calibration: torch.Tensor, margin: float = 1.0) -> torch.Tensor:
        """Switch the four GEMMs per layer that FP8_FIELDS names to e4m3 (BASELINE config 5): per-tensor weight scales amax / 448 and
        static per-tensor input scales from one bf16 calibration pass over `calibration` -- the model's usual input: token ids [B, T],
        a clip [B, frames, C, H, W], features [B, T, feat_dim] -- (amax * margin / 448).  Returns the calibration amax table
        f32 [depth, 4], columns in FP8_FIELDS order."""
        if any(v % 128 for v in self.fp8_widths):
            raise ValueError(self.FP8_WIDTHS_ERROR)
        self.fp8_layers = None
        amax = torch.zeros(max(self.depth, 1), 4, dtype=torch.float32, device=self.device)
        self._calibrate(calibration, amax)
        table = amax.cpu()                                    # one-time sync: the scales become launch constants
        seen = table[: self.depth]
        if not bool((torch.isfinite(seen) & (seen > 0)).all()):   # tribe_absmax_fwd reports a NaN / inf anywhere in a tensor as NaN / inf
            raise ValueError(f"fp8 calibration saw an all-zero or non-finite (NaN / inf) GEMM input: amax per layer {seen.tolist()}")
        layers = (self.FP8_LAYER * max(self.depth, 1))()
        self.fp8_packs = []
        for i in range(self.depth):
            q = []
            for j, (field, w) in enumerate(zip(self.FP8_FIELDS, getattr(self, self.FP8_SOURCE)[i])):
                w_amax = float(ops.absmax(w))
                if not (math.isfinite(w_amax) and w_amax > 0):
                    raise ValueError(f"fp8: layer {i} weight {field} has amax {w_amax}: an all-zero or non-finite tensor has no e4m3 scale")
                w_scale = w_amax / ops.FP8_MAX
                q.append(ops.quantize_fp8(w, w_scale, K_pad=w.shape[1]))
                setattr(layers[i], field, q[-1].data_ptr())
                layers[i].w_scale[j] = w_scale
                layers[i].in_scale[j] = float(table[i, j]) * margin / ops.FP8_MAX
            self.fp8_packs.append(q)
        self.fp8_layers = layers
        return table

    def _launch(self, d: C.Structure, states: torch.Tensor, fp8: bool | None, amax: torch.Tensor | None, caller: str,
                forward: str | None = None, extra: tuple[tp.Any, ...] = ()) -> torch.Tensor:
        """The tail of every forward: d is the filled descriptor but for fp8_host / amax_out; fp8 None = the e4m3 GEMMs when enable_fp8()
        has run; amax = the calibration table to fill (a bf16 pass).  Returns `states`, written by FORWARD on the current stream.
        `forward` names another entry point that takes the same descriptor, with `extra` arguments between it and `states`."""
        forward = forward or self.FORWARD
        if (self.fp8_layers is not None if fp8 is None else fp8) and amax is None:
            if self.fp8_layers is None:
                raise ValueError(f"{caller}(fp8=True) before enable_fp8()")
            d.fp8_host = C.cast(self.fp8_layers, C.POINTER(self.FP8_LAYER))
        if amax is not None:
            d.amax_out = amax.data_ptr()
        nbytes = getattr(lib(), forward.replace("_fwd", "_workspace_bytes"))(C.byref(d))
        ws = ops.workspace(nbytes, self.device, "extractor")
        check(getattr(lib(), forward)(C.byref(d), *extra, states.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), forward)
        return states
