"""V-JEPA2 (ViT-g) video feature extractor on MI355X HIP kernels.

Mirror of the reference plugin `VJEPA2` / `VideoModel` (/root/reference/data_utils/data_utils/features/video.py:56-274):
for every 0.5 s step a clip of 64 frames covering the previous 4 s (video.py:203-224) goes through the HF video
processor and `VJEPA2Model(..., output_hidden_states=True)` (video.py:247-268); the 41 hidden states are stacked and
averaged over the 8192 tokens (video.py:228) -> `[41, 1408]` per step.  Here the encoder forward and the token mean run
in one C call (`tribe_vjepa2_fwd`); the predictor head, whose output the reference discards, is not run.
Frame decoding stays on the host (SURVEY: moviepy decode is out of scope).  The processor (resize / crop / rescale /
normalise) runs on the host by default, and the boundary is its `pixel_values_videos` f32 [B, frames, 3, H, W]; with
`VJEPA2(frontend="hip")` the decoded uint8 frames are uploaded instead and `HipVideoProcessor` (`tribe_video_preprocess_fwd`,
csrc/vidproc.hip) writes `pixel_values_videos` straight into HBM.
"""

from __future__ import annotations

import ctypes as C
import typing as tp

import numpy as np
import pydantic
import torch

from tribe_hip import ops
from tribe_hip._lib import VitFp8Layer, VitLayer, Vjepa2Desc
from tribe_hip.ops import aa_resize_taps, video_resized_size  # noqa: F401  (host helpers of the front end)

from .extractor_host import ExtractorHost
from .plugin import HbmFeaturePlugin

# facebook/vjepa2-vitg-fpc64-256 hyper-parameters (public model card; configuration input, not verifiable offline)
VJEPA2_VITG_FPC64_256 = dict(patch_size=16, crop_size=256, frames_per_clip=64, tubelet_size=2, hidden_size=1408, in_chans=3,
                             num_attention_heads=22, num_hidden_layers=40, mlp_ratio=48 / 11, layer_norm_eps=1e-6, qkv_bias=True)


def rope3d_tables(grid_depth: int, grid_size: int, dim_head: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-element cos / sin tables [tokens, dim_head] of VJEPA2RopeAttention (modeling_vjepa2.py:180-294): the head is
    split into three segments of 2*((dim_head//3)//2) dims rotated by the frame / height / width index of the token;
    inside a segment of D dims element j uses frequency 10000^(-(j mod D/2)/(D/2)) (the library TILES its frequencies,
    `repeat(1,1,1,2)`, while pairing (2i, 2i+1)); remaining dims are passed through (cos 1, sin 0)."""
    seg = 2 * ((dim_head // 3) // 2)
    ids = torch.arange(grid_depth * grid_size * grid_size)
    tpf = grid_size * grid_size
    frame = ids // tpf
    height = (ids - tpf * frame) // grid_size
    width = (ids - tpf * frame) - grid_size * height
    omega = 1.0 / 10000 ** (torch.arange(seg // 2, dtype=torch.float32) / (seg / 2.0))
    cos = torch.ones(ids.numel(), dim_head)
    sin = torch.zeros(ids.numel(), dim_head)
    for k, pos in enumerate((frame, height, width)):
        freq = pos.float()[:, None] * omega[None, :]  # [tokens, seg/2]
        cos[:, k * seg:(k + 1) * seg] = freq.cos().repeat(1, 2)
        sin[:, k * seg:(k + 1) * seg] = freq.sin().repeat(1, 2)
    return cos.contiguous(), sin.contiguous()


class HipVJEPA2Encoder(ExtractorHost):
    """Packed bf16 weights of the V-JEPA2 encoder + the forward-with-token-mean launcher.  enable_fp8(calibration_clip
    [B, frames, C, H, W]) switches the four Linear GEMMs of every layer to e4m3 (amax table columns: qkv, proj, fc1, fc2 in)."""

    FORWARD, FP8_LAYER, FP8_FIELDS = "tribe_vjepa2_fwd", VitFp8Layer, ("w_qkv", "w_proj", "w_fc1", "w_fc2")
    FP8_WIDTHS_ERROR = "fp8 path: hidden_size and the MLP width must be multiples of 128"
    MISSING_WEIGHTS_ARE_NONE = True    # qkv_bias=False checkpoints

    def __init__(self, config: tp.Any, state_dict: dict[str, torch.Tensor], device: str | torch.device = "cuda"):
        super().__init__(config, {k.removeprefix("encoder."): v for k, v in state_dict.items() if not k.startswith("predictor.")}, device)
        g, f32, own = self.cfg, self.f32, self.own
        self.patch, self.crop, self.frames, self.tubelet = g("patch_size"), g("crop_size"), g("frames_per_clip"), g("tubelet_size")
        self.dim, self.chans, self.heads, self.depth = g("hidden_size"), g("in_chans"), g("num_attention_heads"), g("num_hidden_layers")
        self.mlp = int(self.dim * g("mlp_ratio"))
        self.eps = float(g("layer_norm_eps"))
        self.dim_head = self.dim // self.heads
        self.fp8_widths = (self.dim, self.mlp)
        wp = f32("embeddings.patch_embeddings.proj.weight")  # [dim, C, tub, p, p]
        self.w_patch = ops.pack_weight(wp.reshape(self.dim, -1).contiguous())
        self.b_patch = f32("embeddings.patch_embeddings.proj.bias")
        self.layers = (VitLayer * max(self.depth, 1))()
        self.packs: list[tuple[torch.Tensor, ...]] = []      # bf16 (qkv, proj, fc1, fc2) per layer, the source of the fp8 packs
        for i in range(self.depth):
            p = f"layer.{i}."
            L = self.layers[i]
            wqkv = torch.cat([f32(p + "attention.query.weight"), f32(p + "attention.key.weight"), f32(p + "attention.value.weight")])
            bq = f32(p + "attention.query.bias")
            L.norm1_w, L.norm1_b = own(f32(p + "norm1.weight")), own(f32(p + "norm1.bias"))
            packs = (ops.pack_weight(wqkv), ops.pack_weight(f32(p + "attention.proj.weight")), ops.pack_weight(f32(p + "mlp.fc1.weight")),
                     ops.pack_weight(f32(p + "mlp.fc2.weight")))
            self.packs.append(packs)
            L.w_qkv, L.w_proj, L.w_fc1, L.w_fc2 = (own(t) for t in packs)
            L.b_qkv = own(torch.cat([bq, f32(p + "attention.key.bias"), f32(p + "attention.value.bias")])) if bq is not None else None
            L.b_proj = own(f32(p + "attention.proj.bias"))
            L.norm2_w, L.norm2_b = own(f32(p + "norm2.weight")), own(f32(p + "norm2.bias"))
            L.b_fc1, L.b_fc2 = own(f32(p + "mlp.fc1.bias")), own(f32(p + "mlp.fc2.bias"))
        self._tabs: dict[tuple[int, int], tuple[torch.Tensor, torch.Tensor]] = {}
        del self._sd

    def _calibrate(self, calibration_clip: torch.Tensor, amax: torch.Tensor) -> None:
        self.hidden_state_means(calibration_clip, _amax=amax)

    def hidden_state_means(self, pixel_values_videos: torch.Tensor, fp8: bool | None = None, _amax: torch.Tensor | None = None) -> torch.Tensor:
        """pixel_values_videos f32 [B, frames, C, H, W] -> f32 [B, depth + 1, dim] (video.py:262-268 + :228).
        fp8: None = use the e4m3 GEMMs when enable_fp8() has run."""
        pix = pixel_values_videos.to(device=self.device, dtype=torch.float32).contiguous()
        B, F, Cc, H, W = pix.shape
        if Cc != self.chans or F % self.tubelet or H % self.patch or W % self.patch:
            raise ValueError(f"unexpected clip shape {tuple(pix.shape)}")
        key = (F // self.tubelet, H // self.patch)
        if H != W:
            raise ValueError("square frames expected (crop_size x crop_size)")
        if key not in self._tabs:
            cos, sin = rope3d_tables(key[0], key[1], self.dim_head)
            self._tabs[key] = (cos.to(self.device), sin.to(self.device))
        cos, sin = self._tabs[key]
        d = Vjepa2Desc()
        d.B, d.frames, d.chans, d.height, d.width, d.tubelet, d.patch = B, F, Cc, H, W, self.tubelet, self.patch
        d.dim, d.depth, d.heads, d.dim_head, d.mlp, d.ln_eps = self.dim, self.depth, self.heads, self.dim_head, self.mlp, self.eps
        d.w_patch, d.b_patch, d.K_pad = self.w_patch.data_ptr(), ops._p(self.b_patch), self.w_patch.shape[1]
        d.layers_host = C.cast(self.layers, C.POINTER(VitLayer))
        d.cos_tab, d.sin_tab, d.pixels = cos.data_ptr(), sin.data_ptr(), pix.data_ptr()
        states = torch.empty(self.depth + 1, B, self.dim, dtype=torch.float32, device=self.device)
        return self._launch(d, states, fp8, _amax, "hidden_state_means").transpose(0, 1).contiguous()


def default_video_processor(frames: np.ndarray, crop_size: int = 256) -> torch.Tensor:
    """What the HF `VJEPA2VideoProcessor` does at its defaults (video_processing_vjepa2.py: resize shortest edge to
    int(crop * 256 / 224) bilinear, centre crop, rescale 1/255, ImageNet normalise) for uint8 frames [F, H, W, 3] ->
    f32 [1, F, 3, crop, crop].  The HF class needs torchvision (absent); its interpolation kernel's antialiasing is not
    reproduced bit for bit, so pixel parity is unpinned -- pass `processor=` to `VJEPA2.attach` to use another front end."""
    x = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 3, 1, 2).float()
    H, W = x.shape[-2:]
    short = int(crop_size * 256 / 224)
    scale = short / min(H, W)
    nh, nw = max(short, int(round(H * scale))), max(short, int(round(W * scale)))
    x = torch.nn.functional.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)
    top, left = (nh - crop_size) // 2, (nw - crop_size) // 2
    x = x[:, :, top:top + crop_size, left:left + crop_size] / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return ((x - mean) / std)[None]


class HipVideoProcessor:
    """`default_video_processor` on the GPU (`ops.video_preprocess`), usable wherever `VJEPA2.attach(processor=...)` takes a
    processor.  Called on uint8 frames [F, H, W, 3] (numpy, host or device tensor; host frames are uploaded once, as uint8):
    returns f32 [1, F, 3, crop, crop] on the GPU.  `batched(frames, index)` takes the DISTINCT frames of several clips and an
    integer index [clips, F] into them and returns [clips, F, 3, crop, crop] from one launch."""

    def __init__(self, crop_size: int = 256, device: str | torch.device = "cuda"):
        self.crop_size, self.device = int(crop_size), torch.device(device)

    def _upload(self, frames: tp.Any) -> torch.Tensor:
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        if t.dtype != torch.uint8:
            raise ValueError(f"HipVideoProcessor: frames must be uint8, got {t.dtype}")
        return t.to(self.device).contiguous()

    def __call__(self, frames: tp.Any) -> torch.Tensor:
        dev = self._upload(frames)
        return ops.video_preprocess(dev, np.arange(dev.shape[0]), self.crop_size)[None]

    def batched(self, frames: tp.Any, index: tp.Any) -> torch.Tensor:
        index = np.asarray(index)
        if index.ndim != 2:
            raise ValueError(f"HipVideoProcessor.batched: index must be [clips, frames], got {index.shape}")
        return ops.video_preprocess(self._upload(frames), index, self.crop_size).reshape(*index.shape, 3, self.crop_size, self.crop_size)


class VJEPA2(HbmFeaturePlugin):
    """The reference's video feature (video.py:56-236) on the HIP ViT-g forward: fields `name`, `layers`, `layer_aggregation`,
    `device`, `infra`; `prepare`, `__call__ -> Tensor[L, D, T]`, `_get_data -> [41, 1408, T_event@2Hz]` per Video event (item
    uid `filepath_offset_duration`, video.py:191-195).  Per 0.5 s step the 64 frames of the previous 4 s are decoded on the
    host (`event.read().get_frame(t)`, moviepy in the reference), processed, and the encoder forward + token mean of all
    41 states is one C call; `clips_per_launch` steps go through the encoder together.  `frontend` selects who turns the decoded
    frames into `pixel_values_videos`: "host" (default) runs the processor per clip on the host and uploads its f32 result;
    "hip" decodes every DISTINCT frame time of a launch group once (consecutive steps of an event whose duration is a multiple
    of 0.5 s share most of their frames), uploads those frames as uint8 and runs `HipVideoProcessor` in one launch per group."""

    name: tp.Literal["VJEPA2"] = "VJEPA2"
    pretrained: str = "facebook/vjepa2-vitg-fpc64-256"    # video.py:247-254; resolved from the local HF cache only
    frontend: tp.Literal["host", "hip"] = "host"          # a route, not a result: kept out of the class uid like `device`
    clips_per_launch: int = 4   # 37.6 ms per clip at 4, 41.3 at 2, 44.9 at 1 (profiles/r02_p_config3_e2e.txt, r02_m_extractor_bench.txt)
    _EVENT_TYPE: tp.ClassVar[str] = "Video"
    _KIND: tp.ClassVar[str] = "sampled"
    _PASS_EVENT_DURATION: tp.ClassVar[bool] = True
    _model: tp.Any = pydantic.PrivateAttr(default=None)
    _processor: tp.Any = pydantic.PrivateAttr(default=None)

    def attach(self, model: HipVJEPA2Encoder, processor: tp.Callable[[np.ndarray], torch.Tensor] | None = None) -> "VJEPA2":
        if processor is not None and self.frontend == "hip":
            raise ValueError('VJEPA2: frontend="hip" runs its own processor on the GPU; attach no `processor`, or use frontend="host"')
        self._model, self._processor = model, processor
        return self

    @classmethod
    def _exclude_from_cls_uid(cls) -> list[str]:
        return super()._exclude_from_cls_uid() + ["frontend"]

    @property
    def model(self) -> HipVJEPA2Encoder:
        if self._model is None:
            from transformers import AutoModel

            hf = AutoModel.from_pretrained(self.pretrained, local_files_only=True)
            self._model = HipVJEPA2Encoder(hf.config, hf.state_dict())
        return self._model

    def _item_uid(self, event: tp.Any) -> str:
        return f"{event.filepath}_{event.offset:.2f}_{event.duration:.2f}"

    def _compute(self, events: list[tp.Any]) -> tp.Iterator[np.ndarray]:
        from ..base import Frequency

        model = self.model
        if self.frontend == "hip":
            yield from self._compute_hip(events)
            return
        process = self._processor or (lambda fr: default_video_processor(fr, model.crop))
        n_frames = model.frames
        subtimes = [k / n_frames * 4.0 for k in reversed(range(n_frames))]                  # video.py:203-205
        for event in events:
            video = event.read()
            expect = Frequency(2.0).to_ind(event.duration)
            times = np.linspace(0, video.duration, expect + 1)[1:]                          # video.py:218
            out = np.zeros((len(times), model.depth + 1, model.dim))                        # f64, as np.zeros in video.py:230
            for k0 in range(0, len(times), self.clips_per_launch):
                clips = []
                for t in times[k0:k0 + self.clips_per_launch]:
                    frames = np.array([np.asarray(video.get_frame(max(0, t - t2))).astype("uint8") for t2 in subtimes])
                    clips.append(process(frames))
                means = model.hidden_state_means(torch.cat(clips, dim=0))                   # [clips, 41, dim]
                out[k0:k0 + len(clips)] = means.cpu().numpy()
            if hasattr(video, "close"):
                video.close()
            yield out.transpose(1, 2, 0)                                                    # [n_states, dim, T_event] (video.py:234)

    def _compute_hip(self, events: list[tp.Any]) -> tp.Iterator[np.ndarray]:
        """`_compute` with the processor on the GPU: per launch group the frame times of all clips are collected, each distinct
        time (equal as Python floats, nothing looser) is decoded once, and the distinct frames go up as one uint8 tensor."""
        from ..base import Frequency

        model = self.model
        if self._processor is not None:
            raise ValueError('VJEPA2: frontend="hip" runs its own processor on the GPU; attach no `processor`, or use frontend="host"')
        process = HipVideoProcessor(model.crop, model.device)
        n_frames = model.frames
        subtimes = [k / n_frames * 4.0 for k in reversed(range(n_frames))]                  # video.py:203-205
        for event in events:
            video = event.read()
            expect = Frequency(2.0).to_ind(event.duration)
            times = np.linspace(0, video.duration, expect + 1)[1:]                          # video.py:218
            out = np.zeros((len(times), model.depth + 1, model.dim))
            for k0 in range(0, len(times), self.clips_per_launch):
                slot_of: dict[float, int] = {}                                              # distinct frame time -> row of `frames`
                index = [[slot_of.setdefault(float(max(0, t - t2)), len(slot_of)) for t2 in subtimes] for t in times[k0:k0 + self.clips_per_launch]]
                frames = np.array([np.asarray(video.get_frame(tt)).astype("uint8") for tt in slot_of])
                means = model.hidden_state_means(process.batched(frames, index))            # [clips, 41, dim]
                out[k0:k0 + len(index)] = means.cpu().numpy()
            if hasattr(video, "close"):
                video.close()
            yield out.transpose(1, 2, 0)
