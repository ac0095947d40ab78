"""GPU: the HIP audio front end (csrc/fbank.hip, ops.w2vbert_fbank, features.audio.HipFbank) against transformers'
SeamlessM4TFeatureExtractor run on the CPU in the same test.

Value tolerance.  The extractor stores the spectrum as complex64 before squaring and normalises in float32, so even an
all-float64 restatement of its arithmetic (frames, DC removal, pre-emphasis, Povey window, DFT as a matrix product, mel,
log, per-bin z-score, pad, stack: `restate` below) differs from it.  Measured on the CPU, |restatement - extractor| over all
elements, max / 99.9th percentile:

    waveform                      float64 restatement       float32 restatement       (the kernels, MI355X: max)
    noise_7s                      8.31e-06 / 7.85e-06       5.72e-05 / 4.91e-05       4.20e-05
    speech_like_10s               6.30e-06 / 5.85e-06       1.65e-04 / 4.67e-05       5.77e-05
    gated_noise_floor_10s         5.15e-07 / 4.61e-07       3.02e-05 / 2.98e-06       1.98e-05
    odd_frames_3s                 6.30e-06 / 5.88e-06       5.79e-05 / 1.80e-05       3.03e-05
    two_channel (after stage 1)   6.74e-06 / 6.29e-06       4.08e-05 / 3.46e-05       2.62e-05

(the features are z-scored, O(1); the float64 column is mostly the extractor's own float32 normalisation.)

The bar for the kernels is max |d| <= 4 x the float32 restatement's max |d| ON THE SAME WAVEFORM, computed in the test from
the restatement itself, with no element excluded (4 x: the summation order of a 400-term DFT and of the 80 x 257 mel product
differs between numpy's blocked sums and a k-ordered fma chain, and `log` near the mel floor amplifies absolute error).
The float32 restatement stays far below 1e-2 on every value waveform, so the DFT is accumulated in float32.

A waveform with digital silence sits on the max(., mel_floor) clamp, where one ulp flips a frame between log(floor) and
something larger and moves the whole bin's mean and variance: it is kept out of the value test and checked for shape,
finiteness and agreement on the bins none of whose frames lies within a factor of 2 of the floor (floor / 2 <= energy <=
2 floor) in the float64 restatement's mel energies; at least half of the 80 bins must remain (76 do).  A frame of exact
zeros is 0 in every arithmetic, clamps identically everywhere and excludes nothing."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SR = 16_000
MEL_FLOOR = 1.192092955078125e-07
BAR_FACTOR = 4.0


# ---- waveforms (fixed seeds) -------------------------------------------------------------------------------------------
def wav_noise(seconds: float = 7.0, seed: int = 0, n: int | None = None) -> np.ndarray:
    n = int(seconds * SR) if n is None else n
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def wav_speech_like(seconds: float = 10.0, seed: int = 1, n: int | None = None) -> np.ndarray:
    """Chirped harmonics (f0 110 -> 220 Hz, 20 partials falling as 1 / h) with a 4 Hz amplitude modulation, plus 1 % noise."""
    n = int(seconds * SR) if n is None else n
    t = np.arange(n) / SR
    phase = 2 * np.pi * (110.0 * t + 0.5 * (110.0 / (n / SR)) * t * t)
    tone = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 21))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)
    x = 0.2 * env * tone
    x = x + 0.01 * np.abs(x).max() * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def wav_gated(seed: int = 2) -> np.ndarray:
    """Noise switched on and off at 0.5 Hz (1 s on, 1 s off) over a 1e-4 noise floor, 10 s + 37 samples."""
    n = 10 * SR + 37
    rng = np.random.default_rng(seed)
    gate = ((np.arange(n) // SR) % 2 == 0).astype(np.float64)
    return (0.2 * gate * rng.standard_normal(n) + 1e-4 * rng.standard_normal(n)).astype(np.float32)


def wav_odd_frames(seed: int = 3) -> np.ndarray:
    n = 3 * SR + 160                      # F = 299
    assert (1 + (n - 400) // 160) % 2 == 1
    return wav_speech_like(n=n, seed=seed)


def wav_two_channel(seed: int = 4) -> np.ndarray:
    n = 5 * SR + 11
    left, right = wav_speech_like(n=n, seed=seed), wav_noise(n=n, seed=seed + 1)
    return np.stack([left + 0.02, 0.5 * right - 0.01], axis=1).astype(np.float32)      # [n, 2], a DC offset per channel


def wav_with_silence(seed: int = 5) -> np.ndarray:
    """Speech-like, with half a second of exact zeros and 0.75 s of a 150 Hz tone at 1e-6 whose spectral skirt crosses the
    mel floor in a few bins."""
    x = wav_speech_like(seconds=6.0, seed=seed)
    x[SR: SR + SR // 2] = 0.0
    t = np.arange(3 * SR // 4) / SR
    x[4 * SR: 4 * SR + 3 * SR // 4] = (1e-6 * np.sin(2 * np.pi * 150.0 * t)).astype(np.float32)
    return x


VALUE_WAVEFORMS = {"noise_7s": wav_noise, "speech_like_10s": wav_speech_like, "gated_noise_floor_10s": wav_gated, "odd_frames_3s": wav_odd_frames}


# ---- the oracle and its restatements -----------------------------------------------------------------------------------
def hf_features(wav: np.ndarray) -> np.ndarray:
    from transformers import SeamlessM4TFeatureExtractor

    fe = SeamlessM4TFeatureExtractor()
    out = fe(wav, return_tensors="pt", sampling_rate=SR)
    return out["input_features"][0].numpy()


def preprocess_wav(wav: np.ndarray) -> np.ndarray:
    """Stage 1 as the reference writes it (torch, float32, on the host)."""
    w = torch.mean(torch.from_numpy(wav), dim=1)
    return ((w - w.mean()) / (1e-8 + w.std())).numpy()


def restate(wav: np.ndarray, dtype, return_mel: bool = False) -> np.ndarray:
    """Stages 2-6 in numpy, every array of `dtype`, the DFT as a matrix product."""
    from data_utils.features.audio import fbank_frame_count, kaldi_mel_filters, povey_window

    dt = np.dtype(dtype)
    x = wav.astype(dt) * dt.type(32768.0)
    F = fbank_frame_count(x.size)
    frames = x[np.arange(F)[:, None] * 160 + np.arange(400)[None, :]].copy()
    frames -= frames.mean(axis=1, keepdims=True, dtype=dt)
    frames[:, 1:] -= dt.type(0.97) * frames[:, :-1]
    frames[:, 0] *= dt.type(1 - 0.97)
    frames *= povey_window().astype(dt)
    ang = 2 * np.pi * ((np.arange(400)[:, None] * np.arange(257)[None, :]) % 512) / 512
    re, im = frames @ np.cos(ang).astype(dt), frames @ (-np.sin(ang)).astype(dt)
    energy = (re * re + im * im) @ kaldi_mel_filters().astype(dt)
    if return_mel:
        return energy                                                          # [F, 80], before the floor
    lm = np.log(np.maximum(dt.type(MEL_FLOOR), energy))
    lm = (lm - lm.mean(axis=0, keepdims=True, dtype=dt)) / np.sqrt(lm.var(axis=0, ddof=1, keepdims=True, dtype=dt) + dt.type(1e-7))
    if F % 2:
        lm = np.concatenate([lm, np.zeros((1, 80), dt)])
    return lm.reshape(-1, 160)


def _hip(wav: np.ndarray, zscore: bool = False) -> tuple[np.ndarray, int]:
    from tribe_hip import ops

    feats, lengths = ops.w2vbert_fbank(torch.from_numpy(wav).cuda(), zscore=zscore)
    torch.cuda.synchronize()
    assert feats.shape[0] == 1 and feats.dtype == torch.float32 and feats.is_cuda
    return feats[0].cpu().numpy(), lengths[0]


def _check_values(name: str, wav_for_oracle: np.ndarray, got: np.ndarray) -> None:
    want = hf_features(wav_for_oracle)
    assert got.shape == want.shape, (got.shape, want.shape)
    ref32 = float(np.abs(restate(wav_for_oracle, np.float32) - want).max())
    err = np.abs(got - want)
    print(f"{name}: hip max |d| {err.max():.3e}  p99.9 {np.quantile(err, 0.999):.3e}   float32 restatement max |d| {ref32:.3e}   "
          f"bar {BAR_FACTOR * ref32:.3e}")
    assert np.isfinite(got).all()
    assert ref32 < 1e-2
    assert float(err.max()) <= BAR_FACTOR * ref32, f"{name}: max |d| {err.max():.3e} above {BAR_FACTOR} x {ref32:.3e}"


@pytest.mark.parametrize("name", sorted(VALUE_WAVEFORMS))
def test_fbank_matches_the_hf_extractor(name):
    wav = VALUE_WAVEFORMS[name]()
    got, T = _hip(wav)
    F = 1 + (wav.size - 400) // 160
    assert T == (F + 1) // 2 == got.shape[0] and got.shape[1] == 160
    if F % 2:
        assert name == "odd_frames_3s" and (got[-1, 80:] == 0).all() and np.abs(got[-1, :80]).max() > 0
    _check_values(name, wav, got)


def test_fbank_two_channels_through_the_zscore_stage():
    wav = wav_two_channel()
    got, T = _hip(wav, zscore=True)
    assert T == got.shape[0]
    _check_values("two_channel_zscore", preprocess_wav(wav), got)


def test_fbank_batch_equals_single_chunks_bit_for_bit():
    from tribe_hip import ops

    chunks = [wav_speech_like(seconds=4.0, seed=11), wav_odd_frames(seed=12), wav_noise(seconds=2.5, seed=13)]
    dev = [torch.from_numpy(c).cuda() for c in chunks]
    feats, lengths = ops.w2vbert_fbank(dev, zscore=True)
    assert feats.shape == (3, max(lengths), 160)
    assert lengths == [(1 + (c.size - 400) // 160 + 1) // 2 for c in chunks] and len(set(lengths)) == 3
    for i, d in enumerate(dev):
        single, (T,) = ops.w2vbert_fbank(d, zscore=True)
        assert T == lengths[i] and torch.equal(single[0], feats[i, :T]), f"chunk {i} depends on its batch"
        assert (feats[i, T:] == 0).all()
    assert (feats[1, lengths[1] - 1, 80:] == 0).all()                    # the zero frame appended to the odd chunk
    again, _ = ops.w2vbert_fbank(dev, zscore=True)
    assert torch.equal(again, feats)                                      # ordered reductions: the same bits on every call
    _check_values("batch_chunk_0_zscore", preprocess_wav(chunks[0][:, None]), feats[0, : lengths[0]].cpu().numpy())


def test_fbank_digital_silence_off_the_floor():
    wav = wav_with_silence()
    got, T = _hip(wav)
    want = hf_features(wav)
    assert got.shape == want.shape and np.isfinite(got).all()
    energy = restate(wav, np.float64, return_mel=True)                     # [F, 80] mel energies before the floor
    assert (energy == 0).all(axis=1).any(), "the waveform was meant to hold frames of digital silence"
    # a frame of exact zeros is 0 in every arithmetic and clamps the same way everywhere; the frames that can flip are those whose
    # energy lies within a factor of 2 of the floor, and a bin that has one is left out
    near = (energy >= MEL_FLOOR / 2) & (energy <= 2 * MEL_FLOOR)
    keep = ~near.any(axis=0)
    print(f"digital silence: {int(keep.sum())} of 80 bins checked, {int((energy < MEL_FLOOR).any(axis=1).sum())} frames on the floor")
    assert keep.sum() >= 40
    cols = np.concatenate([keep, keep])
    ref32 = float(np.abs(restate(wav, np.float32) - want)[:, cols].max())
    err = float(np.abs(got - want)[:, cols].max())
    print(f"digital silence: hip max |d| {err:.3e} on the checked bins, float32 restatement {ref32:.3e}, bar {BAR_FACTOR * ref32:.3e}")
    assert ref32 < 1e-2 and err <= BAR_FACTOR * ref32


def test_fbank_refuses_host_tensors_and_short_chunks():
    from tribe_hip import TribeHipError, ops

    with pytest.raises(TribeHipError):
        ops.w2vbert_fbank(torch.zeros(16_000))
    with pytest.raises(ValueError):
        ops.w2vbert_fbank(torch.zeros(399, device="cuda"))
    with pytest.raises(ValueError):
        ops.w2vbert_fbank([torch.zeros(800, device="cuda"), torch.zeros(800, 2, device="cuda")])


# ---- end to end: the plugin with either front end ------------------------------------------------------------------------
def _tiny_w2vbert(hidden=128, heads=2, layers=2, inter=256):
    from transformers import Wav2Vec2BertConfig, Wav2Vec2BertModel

    cfg = Wav2Vec2BertConfig(vocab_size=None, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                             intermediate_size=inter, feature_projection_input_dim=160, hidden_act="swish",
                             position_embeddings_type="relative_key", left_max_position_embeddings=64,
                             right_max_position_embeddings=8, conv_depthwise_kernel_size=31, add_adapter=False,
                             use_intermediate_ffn_before_adapter=False, layerdrop=0.0, apply_spec_augment=False)
    torch.manual_seed(0)
    m = Wav2Vec2BertModel(cfg).eval()
    with torch.no_grad():  # zero-initialised in HF; make the relative-position path carry signal
        for layer in m.encoder.layers:
            layer.self_attn.distance_embedding.weight.normal_(0, 0.5)
    return cfg, m


def test_plugin_front_ends_agree_end_to_end():
    import types

    from data_utils.features.audio import HipFbank, HipWav2Vec2Bert, Wav2VecBert
    from transformers import SeamlessM4TFeatureExtractor

    cfg, hf = _tiny_w2vbert()
    left = wav_speech_like(seconds=6.0, seed=21)
    wav = np.stack([left, 0.6 * wav_noise(seconds=6.0, seed=22) + 0.3 * left], axis=1)                  # [n, 2]
    snd = types.SimpleNamespace(filepath="clip.wav", offset=0.0, duration=6.0, frequency=float(SR), read=lambda: torch.from_numpy(wav))
    outs = {}
    for frontend, fe in (("hf", SeamlessM4TFeatureExtractor()), ("hip", HipFbank())):
        plug = Wav2VecBert(frontend=frontend).attach(HipWav2Vec2Bert(cfg, hf.state_dict()), feature_extractor=fe)
        (arr,) = list(plug._get_data([snd]))
        outs[frontend] = torch.from_numpy(arr)
    assert outs["hip"].shape == outs["hf"].shape == (cfg.num_hidden_layers + 1, cfg.hidden_size, 12)

    feats = torch.from_numpy(hf_features(preprocess_wav(wav)))[None]
    with torch.no_grad():
        states = torch.stack(hf(feats, output_hidden_states=True).hidden_states)[:, 0]           # [n_states, T, hidden] f32
    want = torch.nn.functional.interpolate(states.transpose(1, 2), size=12, mode="nearest")

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    e_hf, e_hip, e_pair = rel(outs["hf"], want), rel(outs["hip"], want), rel(outs["hip"], outs["hf"])
    print(f"vs float32 transformers: frontend=hf {e_hf:.3e}, frontend=hip {e_hip:.3e}; hip vs hf {e_pair:.3e}")
    assert e_pair < 3e-2 and e_hf < 3e-2 and e_hip < 3e-2
