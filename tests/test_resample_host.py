"""CPU (no GPU): the host side of the HIP resampler -- julius' `ResampleFrac` filter bank (zeros = 24, rolloff = 0.945) as
`julius_resample_kernels` builds it, its output length, the 64 MiB cap, the plugin's `resampler` field and item uid, and the
argument checks of `tribe_resample_frac_fwd` (made before any launch).  julius is not installed: `_recipe` below is a second
transcription of its published torch recipe, so the tables are pinned against the recipe, not against the package."""

import ctypes
import math
import types

import numpy as np
import pytest
import torch

RATIOS = {(48000, 16000): (3, 1, 77, 157), (44100, 16000): (441, 160, 70, 581), (22050, 16000): (441, 320, 35, 511),
          (8000, 16000): (1, 2, 26, 53), (11025, 16000): (441, 640, 26, 493)}


def _recipe(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945) -> torch.Tensor:
    g = math.gcd(old_sr, new_sr)
    old_sr, new_sr = old_sr // g, new_sr // g
    sr = min(new_sr, old_sr) * rolloff
    width = math.ceil(zeros * old_sr / sr)
    idx = torch.arange(-width, width + old_sr).float()
    kernels = []
    for i in range(new_sr):
        t = (-i / new_sr + idx / old_sr) * sr
        t.clamp_(-zeros, zeros)
        t *= math.pi
        window = torch.cos(t / zeros / 2) ** 2
        kernel = torch.where(t == 0, torch.tensor(1.0, dtype=t.dtype), torch.sin(t) / t) * window
        kernel /= kernel.sum()
        kernels.append(kernel)
    return torch.stack(kernels)


@pytest.mark.parametrize("rates", sorted(RATIOS))
def test_table_shape_and_values(rates):
    from data_utils.features.audio import julius_resample_kernels

    old, new, width, table = julius_resample_kernels(*rates)
    assert (old, new, width, table.shape[1]) == RATIOS[rates]
    assert table.dtype == torch.float32 and table.shape == (new, 2 * width + old) and table.is_contiguous()
    assert float((table.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    want = _recipe(*rates)
    assert table.shape == want.shape and np.array_equal(table.numpy().view(np.uint32), want.numpy().view(np.uint32))
    assert julius_resample_kernels(*rates)[3] is table                  # cached


def test_equal_rates_need_no_table():
    from data_utils.features.audio import julius_resample_kernels, resample_output_length

    old, new, width, table = julius_resample_kernels(16000, 16000)
    assert (old, new, width) == (1, 1, 0) and table.numel() == 0
    assert resample_output_length(12345, 16000, 16000) == 12345


def test_output_length_is_the_float32_floor():
    from data_utils.features.audio import resample_output_length

    assert 160 * 299993 // 441 == 108840 and resample_output_length(299993, 44100, 16000) == 108841      # the float32 bump
    assert 27000002 // 3 == 9000000 and resample_output_length(27000002, 48000, 16000) == 9000001
    assert resample_output_length(299993, 441, 160) == 108841                                              # reduced rates: the same
    assert resample_output_length(441 * 100, 44100, 16000) == 160 * 100                                    # a multiple of old
    assert resample_output_length(3 * 1000, 48000, 16000) == 1000
    assert resample_output_length(1, 48000, 16000) == 0 and resample_output_length(1, 8000, 16000) == 2
    assert resample_output_length(1, 44100, 16000) == 0 and resample_output_length(5, 48000, 16000) == 1
    for rates, (old, new, _, _) in RATIOS.items():                      # never more than the strided convolution produces
        for n in (1, 2, old - 1, old, old + 1, 7 * old + 3, 299993, 2_646_000, 27000002, (1 << 31) + 5):
            if n >= 1:
                assert 0 <= resample_output_length(n, *rates) <= (n // old + 1) * new


def test_a_table_above_64_mib_is_refused():
    from data_utils.features.audio import julius_resample_kernels

    with pytest.raises(ValueError, match="64 MiB"):
        julius_resample_kernels(44100, 16001)
    with pytest.raises(ValueError):
        julius_resample_kernels(0, 16000)


def test_resampler_field_and_item_uid_of_the_audio_plugin():
    import pydantic

    from data_utils.features.audio import Wav2VecBert

    event = types.SimpleNamespace(filepath="clip.wav", offset=1.5, duration=6.0)
    default, hip = Wav2VecBert(), Wav2VecBert(resampler="hip")
    assert default.resampler == "scipy" and hip.resampler == "hip"
    assert default._item_uid(event) == "clip.wav_1.50_6.00" == Wav2VecBert(frontend="hip")._item_uid(event)
    assert hip._item_uid(event) != default._item_uid(event) and hip._item_uid(event).startswith(default._item_uid(event))
    assert Wav2VecBert(frontend="hip", resampler="hip")._item_uid(event) == hip._item_uid(event)
    assert "resampler" not in Wav2VecBert._exclude_from_cls_uid()       # a result, not a route
    with pytest.raises(pydantic.ValidationError):
        Wav2VecBert(resampler="julius")


def test_resample_argument_errors_do_not_need_a_gpu():
    from tribe_hip import _lib

    handle = _lib.lib()
    dummy = np.zeros(16, np.float32)                                    # any non-null address: nothing is dereferenced before the checks pass
    addr = dummy.ctypes.data
    SAME = object()

    def call(n=(1000,), n_out=(333,), B=None, channels=2, old=3, new=1, width=77, wavs=SAME, outs=SAME, table=addr, n_null=False, n_out_null=False):
        B = len(n) if B is None else B
        n_arr = None if n_null else (ctypes.c_int64 * len(n))(*n)
        m_arr = None if n_out_null else (ctypes.c_int64 * len(n_out))(*n_out)
        wavs = (addr,) * len(n) if wavs is SAME else wavs
        outs = (addr,) * len(n) if outs is SAME else outs
        w_arr = None if wavs is None else (ctypes.c_void_p * len(wavs))(*wavs)
        o_arr = None if outs is None else (ctypes.c_void_p * len(outs))(*outs)
        return handle.tribe_resample_frac_fwd(w_arr, n_arr, B, channels, old, new, width, table, o_arr, m_arr, None)

    def refused(word: bytes, **kw) -> bool:
        return call(**kw) < 0 and word in handle.tribe_last_error()

    assert refused(b"chunks", n=(), n_out=(), B=0)
    assert refused(b"chunks", n=(1000,) * 33, n_out=(333,) * 33)
    assert refused(b"channels", channels=0)
    assert refused(b"samples", n=(0,))
    assert refused(b"n_out", n_out=(0,))
    assert refused(b"n_out", n_out=(335,))                               # (1000 / 3 + 1) * 1 = 334 is the last that exists
    assert refused(b"n_out", n=(1000, 7), n_out=(333, 4))                # (7 / 3 + 1) * 1 = 3
    assert refused(b"equal", old=1, new=1)
    assert refused(b"equal", old=160, new=160)
    assert refused(b">= 1", old=0) and refused(b">= 1", new=0) and refused(b">= 1", old=-3)
    assert refused(b"coprime", old=6, new=2) and refused(b"coprime", old=44100, new=16000, width=70)
    assert refused(b"width", width=0)
    assert refused(b"null", wavs=None) and refused(b"null", outs=None) and refused(b"null", table=None)
    assert refused(b"null", n_null=True) and refused(b"null", n_out_null=True)
    assert refused(b"null", wavs=(None,)) and refused(b"null", outs=(None,))
    assert refused(b"64 MiB", old=44100, new=16001, width=70)           # 16001 x 44240 float32 = 2.8 GB
    assert refused(b"64 MiB", old=3, new=1, width=1 << 23)
    with pytest.raises(ValueError, match="64 MiB"):
        _lib.check(call(old=44100, new=16001, width=70), "tribe_resample_frac_fwd")
