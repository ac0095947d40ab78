"""CPU (no GPU): the host side of the HIP audio front end -- its constant tables and frame arithmetic against transformers'
SeamlessM4TFeatureExtractor, the plugin's `frontend` field, and the argument checks of the C entry points (made before
any launch)."""

import ctypes

import numpy as np
import pytest


def _hf():
    from transformers import SeamlessM4TFeatureExtractor

    return SeamlessM4TFeatureExtractor()


def test_tables_equal_the_hf_extractor():
    from data_utils.features.audio import kaldi_mel_filters, povey_window

    fe = _hf()
    window, mel = povey_window(), kaldi_mel_filters()
    assert window.dtype == np.float64 and window.shape == (400,) and mel.dtype == np.float64 and mel.shape == (257, 80)
    assert np.abs(window - fe.window).max() <= 1e-12
    assert np.abs(mel - fe.mel_filters).max() <= 1e-12


@pytest.mark.parametrize("n", [400, 559, 560, 16000, 16037, 160 * 7 + 400, 160 * 8 + 400])
def test_frame_count_and_stacked_length_agree_with_the_hf_shape(n):
    from data_utils.features.audio import fbank_frame_count

    wav = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    with np.errstate(all="ignore"):                                   # n = 400: one frame, ddof = 1 -> NaN features, shape still defined
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = _hf()(wav, return_tensors="np", sampling_rate=16000)["input_features"]
    F = fbank_frame_count(n)
    assert F == 1 + (n - 400) // 160
    assert want.shape == (1, (F + 1) // 2, 160)


def test_shorter_than_one_frame_is_an_error():
    from data_utils.features.audio import HipFbank, fbank_frame_count

    with pytest.raises(ValueError):
        fbank_frame_count(399)
    assert HipFbank().sampling_rate == 16000
    with pytest.raises(NotImplementedError):
        HipFbank(stride=1)
    with pytest.raises(NotImplementedError):
        HipFbank(feature_size=128, num_mel_bins=128)
    with pytest.raises(ValueError):
        HipFbank()(np.zeros(16000, np.float32), sampling_rate=8000)


def test_frontend_field_of_the_audio_plugin():
    import pydantic

    from data_utils.features.audio import HipFbank, Wav2VecBert

    assert Wav2VecBert().frontend == "hf"
    hip = Wav2VecBert(frontend="hip")
    assert hip.frontend == "hip" and isinstance(hip.feature_extractor, HipFbank) and hip._input_frequency == 16000
    with pytest.raises(pydantic.ValidationError):
        Wav2VecBert(frontend="x")
    assert "frontend" in Wav2VecBert._exclude_from_cls_uid() and "device" in Wav2VecBert._exclude_from_cls_uid()


def test_fbank_argument_errors_do_not_need_a_gpu():
    from tribe_hip import _lib

    handle = _lib.lib()
    table = np.zeros(400, np.float32)                                  # any non-null address: nothing is dereferenced before the checks pass
    addr = table.ctypes.data

    def call(n, B=1, channels=1, wavs=(addr,), window=addr, mel=addr, out=addr, ws=addr, ws_bytes=1 << 30, T_max=1 << 20):
        n_arr = (ctypes.c_int64 * len(n))(*n)
        ptrs = (ctypes.c_void_p * len(wavs))(*wavs) if wavs is not None else None
        return handle.tribe_fbank_fwd(ptrs, n_arr, B, channels, 1, window, mel, out, T_max, None, ws, ws_bytes, None)

    assert call([399]) < 0 and b"399 samples" in handle.tribe_last_error()
    with pytest.raises(ValueError):
        _lib.check(call([399]), "tribe_fbank_fwd")
    assert call([16000], channels=0) < 0 and b"channels" in handle.tribe_last_error()
    assert call([16000], wavs=None) < 0 and b"null" in handle.tribe_last_error()
    assert call([16000], wavs=(None,)) < 0 and b"null" in handle.tribe_last_error()
    assert call([16000], window=None) < 0 and call([16000], mel=None) < 0 and call([16000], out=None) < 0 and call([16000], ws=None) < 0
    assert call([16000], B=0) < 0 and call([16000] * 33, B=33, wavs=(addr,) * 33) < 0
    assert call([16000], T_max=10) < 0 and b"T_max" in handle.tribe_last_error()
    assert call([16000], ws_bytes=16) < 0 and b"workspace" in handle.tribe_last_error()

    one = (ctypes.c_int64 * 1)(16000)
    short = (ctypes.c_int64 * 2)(16000, 12)
    assert handle.tribe_fbank_workspace_bytes(one, 1) >= 98 * 80 * 4
    assert handle.tribe_fbank_workspace_bytes(short, 2) == 0 and handle.tribe_fbank_workspace_bytes(None, 1) == 0
