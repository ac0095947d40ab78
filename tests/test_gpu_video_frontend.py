"""GPU: the HIP video front end (csrc/vidproc.hip, ops.video_preprocess, features.video.HipVideoProcessor) against
`default_video_processor` run on the CPU in the same test and against numpy restatements of it
(tests/test_video_frontend_host.py: `restate`, every array float64 or every array float32).

Value tolerance, per shape, on fixed-seed frames with structure (ramps, saturated 0 and 255 patches, noise):
  1. max |kernel - float64 restatement| <= 4 x max |float32 restatement - float64 restatement| on the same frames, computed in
     the test, no element excluded (4 x: what tests/test_gpu_fbank.py grants a different summation order -- the kernel runs
     k-ordered fma chains from tables rounded to float32 once, numpy blocked sums with float32-built weights);
  2. max |kernel - default_video_processor| <= that bar + max |float64 restatement - default_video_processor| (the triangle
     inequality; torch builds its filter from a float32 scale, which is inexact at most shapes).

Figures (output values are O(1), in [-2.12, 2.64]):

    frames            crop   float32 - float64   kernel - float64 (MI355X)   float64 - torch   kernel - torch (MI355X)
    37 x 53           32     8.35e-07            7.19e-07                    1.14e-05          1.16e-05
    20 x 28           32     7.23e-07            7.23e-07                    6.12e-06          6.12e-06
    160 x 90          32     6.89e-07            8.67e-07                    8.20e-07          1.19e-06
    36 x 64           32     3.65e-07            3.65e-07                    3.65e-07          0
    73 x 41           64     8.14e-07            8.14e-07                    8.87e-06          8.70e-06
    400 x 300         32     1.15e-06            1.01e-06                    7.76e-06          8.26e-06
    720 x 1280        256    1.48e-06            9.48e-07                    8.70e-05          8.69e-05

(the bar of check 1 is four times the first column.  At the identity resize, 36 x 64, the kernel is torch's arithmetic bit for bit.)
End to end through the plugin on a 5 s fake clip (tiny random ViT), relative L2 against the float32 `transformers` model on the CPU:
2.02e-3 with `frontend="host"`, 2.02e-3 with `"hip"`, 5.7e-5 between the two; `get_frame` calls 80 and 23.
"""

import numpy as np
import pytest
import torch

from tests.test_video_frontend_host import MEAN, STD, make_frames, restate

pytestmark = pytest.mark.gpu

BAR_FACTOR = 4.0
SHAPES = [(37, 53, 32), (20, 28, 32), (160, 90, 32), (36, 64, 32), (73, 41, 64), (400, 300, 32), (720, 1280, 256)]
_REFS: dict[tuple[int, int, int], tuple[np.ndarray, ...]] = {}


def _refs(H: int, W: int, crop: int) -> tuple[np.ndarray, ...]:
    """(frames, float64 restatement, bar of check 1, default_video_processor on the CPU): computed once per shape, never modified."""
    from data_utils.features.video import default_video_processor

    key = (H, W, crop)
    if key not in _REFS:
        frames = make_frames(2, H, W)
        r64 = restate(frames, crop, np.float64)
        bar = BAR_FACTOR * float(np.abs(restate(frames, crop, np.float32) - r64).max())
        _REFS[key] = (frames, r64, bar, default_video_processor(frames, crop).numpy())
    return _REFS[key]


def _hip(frames: np.ndarray, index, crop: int) -> torch.Tensor:
    from tribe_hip import ops

    out = ops.video_preprocess(torch.from_numpy(frames).cuda(), index, crop)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    return out


@pytest.mark.parametrize("H,W,crop", SHAPES)
def test_video_preprocess_matches_the_restatement_and_the_host_processor(H, W, crop):
    frames, r64, bar, want = _refs(H, W, crop)
    got = _hip(frames, [0, 1], crop).cpu().numpy()[None]
    assert got.shape == want.shape == r64.shape == (1, 2, 3, crop, crop) and np.isfinite(got).all()
    e_r, e_t, t_r = float(np.abs(got - r64).max()), float(np.abs(got - want).max()), float(np.abs(r64 - want).max())
    print(f"{H} x {W} -> {crop}: float32 - float64 {bar / BAR_FACTOR:.3e} (bar {bar:.3e})   kernel - float64 {e_r:.3e}   "
          f"float64 - torch {t_r:.3e}   kernel - torch {e_t:.3e}   values in [{got.min():.2f}, {got.max():.2f}]")
    assert 0 < bar < 1e-4
    assert e_r <= bar, f"max |kernel - f64| {e_r:.3e} above {BAR_FACTOR} x {bar / BAR_FACTOR:.3e}"
    assert e_t <= bar + t_r, f"max |kernel - torch| {e_t:.3e} above {bar:.3e} + {t_r:.3e}"


def test_a_slot_does_not_depend_on_its_batch():
    H, W, crop = 73, 41, 64
    frames = make_frames(5, H, W, seed=3)
    index = np.array([[3, 0, 0, 4], [1, 4, 2, 3]])                                # 2 clips x 4 slots: repeats and a permutation
    dev = torch.from_numpy(frames).cuda()
    from tribe_hip import ops

    got = ops.video_preprocess(dev, index, crop)
    assert got.shape == (8, 3, crop, crop)
    for slot, f in enumerate(index.reshape(-1)):
        alone = ops.video_preprocess(dev[f:f + 1].contiguous(), [0], crop)
        assert torch.equal(alone[0], got[slot]), f"slot {slot} (frame {f}) depends on its batch"
    assert torch.equal(ops.video_preprocess(dev, index, crop), got)               # the same bits on every call
    assert torch.equal(got[1], got[2]) and not torch.equal(got[0], got[1])

    from data_utils.features.video import HipVideoProcessor

    proc = HipVideoProcessor(crop_size=crop)
    assert torch.equal(proc.batched(frames, index), got.reshape(2, 4, 3, crop, crop))
    one = proc(frames)                                                            # numpy in, uploaded once as uint8
    assert one.shape == (1, 5, 3, crop, crop) and torch.equal(one[0, 3], got[0])
    assert torch.equal(proc(torch.from_numpy(frames)), one) and torch.equal(proc(dev), one)


@pytest.mark.parametrize("H,W,crop", [(37, 53, 32), (720, 1280, 256)])
def test_constant_frames_give_each_channels_constant(H, W, crop):
    _, _, bar, _ = _refs(H, W, crop)
    frames = np.zeros((2, H, W, 3), np.uint8)
    frames[1] = 255
    got = _hip(frames, [0, 1], crop).cpu().numpy().astype(np.float64)
    for f, level in enumerate((0.0, 1.0)):
        for c in range(3):
            want = (level - MEAN[c]) / STD[c]
            err = float(np.abs(got[f, c] - want).max())
            assert err <= bar, f"level {level}, channel {c}: {err:.3e} above {bar:.3e}"


def test_video_preprocess_refusals():
    from tribe_hip import TribeHipError, ops

    u8 = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    with pytest.raises(TribeHipError):
        ops.video_preprocess(u8, [0, 1], 32)                                      # a host tensor
    with pytest.raises(ValueError):
        ops.video_preprocess(u8.cuda().float(), [0, 1], 32)
    with pytest.raises(ValueError):
        ops.video_preprocess(torch.zeros(2, 40, 48, 4, dtype=torch.uint8).cuda()[..., :3], [0, 1], 32)    # a non-contiguous view
    with pytest.raises(ValueError):
        ops.video_preprocess(torch.zeros(2, 40, 48, 4, dtype=torch.uint8).cuda(), [0, 1], 32)             # last dimension 4
    with pytest.raises(ValueError):
        ops.video_preprocess(u8.cuda(), [0, 2], 32)                               # an index equal to n_src
    with pytest.raises(ValueError):
        ops.video_preprocess(u8.cuda(), [-1], 32)
    with pytest.raises(ValueError):
        ops.video_preprocess(u8.cuda(), [], 32)


# ---- end to end: the plugin with either front end ------------------------------------------------------------------------
def test_plugin_front_ends_agree_end_to_end_and_hip_decodes_each_distinct_frame_once():
    import types

    from tests.test_gpu_extractors import _tiny_vjepa2

    from data_utils.features.video import VJEPA2, HipVJEPA2Encoder, default_video_processor

    cfg, hf = _tiny_vjepa2()
    duration, steps, per_launch = 5.0, 10, 4                                     # a multiple of 0.5 s: consecutive clips share frames

    class _Clip:
        def __init__(self):
            self.duration, self.calls = duration, 0

        def get_frame(self, t):
            self.calls += 1
            return ((np.arange(80 * 96 * 3).reshape(80, 96, 3) * 7 + int(t * 1000)) % 251).astype(np.uint8)

    subtimes = [k / cfg.frames_per_clip * 4.0 for k in reversed(range(cfg.frames_per_clip))]
    times = np.linspace(0, duration, steps + 1)[1:]
    outs, calls = {}, {}
    for frontend in ("host", "hip"):
        clip = _Clip()
        event = types.SimpleNamespace(filepath="clip.mkv", offset=0.0, duration=duration, read=lambda clip=clip: clip)
        plug = VJEPA2(frontend=frontend, clips_per_launch=per_launch).attach(HipVJEPA2Encoder(cfg, hf.state_dict()))
        (arr,) = list(plug._get_data([event]))
        outs[frontend], calls[frontend] = torch.from_numpy(arr), clip.calls
    assert outs["hip"].shape == outs["host"].shape == (cfg.num_hidden_layers + 1, cfg.hidden_size, steps)

    groups = [times[k0:k0 + per_launch] for k0 in range(0, steps, per_launch)]    # launch groups of 4, 4 and 2 steps
    distinct = sum(len({float(max(0, t - t2)) for t in group for t2 in subtimes}) for group in groups)
    assert calls["host"] == steps * cfg.frames_per_clip
    assert calls["hip"] == distinct < calls["host"], (calls, distinct)

    probe, want = _Clip(), []
    for t in times:
        frames = np.array([probe.get_frame(max(0, t - t2)) for t2 in subtimes])
        with torch.no_grad():
            states = hf(pixel_values_videos=default_video_processor(frames, cfg.crop_size), output_hidden_states=True, skip_predictor=True).hidden_states
        want.append(torch.stack([s[0].mean(0) for s in states]))
    want = torch.stack(want, dim=-1).double()                                    # [n_states, dim, steps]

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    e_host, e_hip, e_pair = rel(outs["host"], want), rel(outs["hip"], want), rel(outs["hip"], outs["host"])
    print(f"vs float32 transformers: frontend=host {e_host:.3e}, frontend=hip {e_hip:.3e}; hip vs host {e_pair:.3e}; "
          f"get_frame calls host {calls['host']}, hip {calls['hip']}")
    assert e_host < 3e-2 and e_hip < 3e-2 and e_pair < 3e-2
