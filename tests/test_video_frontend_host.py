"""CPU (no GPU): the host side of the HIP video front end -- the tap tables of the antialiased resize, a numpy restatement of
`default_video_processor` built from the same formula, the plugin's `frontend` field, and the argument checks that are made
before any launch.  `make_frames`, `dense_weights` and `restate` are shared with tests/test_gpu_video_frontend.py."""

import numpy as np
import pytest
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_frames(n: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """uint8 [n, H, W, 3] with structure: a diagonal ramp per channel, a saturated 0 patch and a saturated 255 patch, and
    noise of +-24 levels -- the processed values span most of [-2.1, 2.6]."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        for c in range(3):
            ramp = 255.0 * ((x * (c + 1) + y * (3 - c) + 7 * f) % (W + H)) / (W + H - 1)
            v = ramp + rng.integers(-24, 25, (H, W))
            v[: max(1, H // 4), : max(1, W // 3)] = 0
            v[H - max(1, H // 3):, W - max(1, W // 4):] = 255
            out[f, :, :, c] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def dense_weights(n_in: int, n_out: int, dt) -> np.ndarray:
    """[n_out, n_in] matrix of the antialiased triangle filter (the formula of the issue, not the code under test): windows and
    centres from the exact ratio in float64, the weights and their normalisation in `dt`."""
    scale = n_in / n_out
    support = scale if scale >= 1 else 1.0
    M = np.zeros((n_out, n_in), dt)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(lo, hi) - c + 0.5) / support)).astype(dt)
        M[i, lo:hi] = w / w.sum(dtype=dt)
    return M


def resized_size(H: int, W: int, crop: int) -> tuple[int, int]:
    short = int(crop * 256 / 224)
    s = short / min(H, W)
    return max(short, int(round(H * s))), max(short, int(round(W * s)))


def restate(frames: np.ndarray, crop: int, dt) -> np.ndarray:
    """`default_video_processor` in numpy, every array of `dt`: W pass, H pass, crop, / 255, normalise -> [1, F, 3, crop, crop]."""
    dt = np.dtype(dt).type
    _, H, W, _ = frames.shape
    nh, nw = resized_size(H, W, crop)
    x = frames.astype(dt).transpose(0, 3, 1, 2)
    x = np.einsum("pw,fchw->fchp", dense_weights(W, nw, dt), x, optimize=True)
    x = np.einsum("oh,fchp->fcop", dense_weights(H, nh, dt), x, optimize=True)
    top, left = (nh - crop) // 2, (nw - crop) // 2
    x = x[:, :, top:top + crop, left:left + crop] / dt(255.0)
    mean, std = np.array(MEAN, dt).reshape(1, 3, 1, 1), np.array(STD, dt).reshape(1, 3, 1, 1)
    return ((x - mean) / std)[None]


def _scatter(first: np.ndarray, weights: np.ndarray, n_in: int) -> np.ndarray:
    M = np.zeros((len(first), n_in), np.float32)
    for r, f in enumerate(first):
        M[r, f:f + weights.shape[1]] += weights[r]
    return M


AXES = [(720, 292), (1280, 519), (1080, 292), (1920, 519), (37, 36), (53, 52), (20, 36), (28, 50), (160, 64), (90, 36), (400, 48),
        (300, 36), (73, 130), (41, 73), (5, 3), (3, 1), (1, 4)]


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_tap_tables(n_in, n_out):
    from data_utils.features.video import aa_resize_taps

    first, w = aa_resize_taps(n_in, n_out, 0, n_out)
    taps = w.shape[1]
    assert first.dtype == np.int32 and w.dtype == np.float32 and first.shape == (n_out,) and w.shape == (n_out, taps)
    assert (first >= 0).all() and (first + taps <= n_in).all()                        # every row, the last positions included
    assert (np.diff(first) >= 0).all() and (w >= 0).all()
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= taps * 2.0 ** -24
    # the table is the dense matrix of the formula, rounded once
    assert np.array_equal(_scatter(first, w, n_in), dense_weights(n_in, n_out, np.float64).astype(np.float32))
    # a table for (start, count) equals those rows of the full table (as matrices: a narrower table may pad differently)
    for start, count in ((0, 1), (n_out // 3, max(1, n_out // 2)), (n_out - 1, 1)):
        f2, w2 = aa_resize_taps(n_in, n_out, start, count)
        assert (f2 >= 0).all() and (f2 + w2.shape[1] <= n_in).all() and w2.shape[1] <= taps
        assert np.array_equal(_scatter(f2, w2, n_in), _scatter(first, w, n_in)[start:start + count])
    # flipping the axis flips the table (the filter is symmetric; up to float64 rounding of the mirrored centres)
    flipped = _scatter(first, w, n_in)[::-1, ::-1]
    assert np.abs(flipped - _scatter(first, w, n_in)).max() <= 2.0 ** -22


def test_tap_table_details():
    from data_utils.features.video import aa_resize_taps

    first, w = aa_resize_taps(64, 64, 0, 64)                                          # identity: one tap of exactly 1.0
    assert w.shape == (64, 1) and (w == 1.0).all() and np.array_equal(first, np.arange(64))
    first, w = aa_resize_taps(36, 36, 2, 32)
    assert w.shape == (32, 1) and (w == 1.0).all() and np.array_equal(first, np.arange(2, 34))
    assert aa_resize_taps(20, 36)[1].shape[1] == 2                                    # upscaling: 2 taps
    assert aa_resize_taps(720, 292, 18, 256)[1].shape[1] == 5 and aa_resize_taps(1080, 292, 18, 256)[1].shape[1] == 8
    assert aa_resize_taps(400, 48, 8, 32)[1].shape[1] == 17
    first, w = aa_resize_taps(20, 36)                                                  # right edge: first moves down, zeros in front
    assert first[-1] == 18 and w[-1, 0] == 0.0 and w[-1, 1] == 1.0
    for bad in ((0, 4, 0, 4), (4, 0, 0, 1), (4, 4, -1, 2), (4, 4, 3, 2), (4, 4, 0, 0)):
        with pytest.raises(ValueError):
            aa_resize_taps(*bad)


@pytest.mark.parametrize("H,W,crop", [(90, 160, 32), (160, 90, 32), (36, 36, 32)])
def test_float64_restatement_matches_default_video_processor(H, W, crop):
    """At these shapes n_in / n_out is exact in float32, so torch's own float32 scale is the formula's.  What remains is torch's
    float32 arithmetic: weights, two filter passes on values up to 255 (half an ulp there is 7.6e-6, which is 1.3e-7 after
    / 255 / 0.224) and three normalisation roundings at magnitudes up to 2.64 (half an ulp 1.2e-7).
    Measured on these frames, max |float64 restatement - torch|: 90 x 160 7.6e-7, 160 x 90 8.2e-7, 36 x 36 3.7e-7 (random frames
    in the session that specified this change: 6.4e-7).  The bar is 2e-6, between two and three times the largest figure seen: a wrong tap, a
    window off by one or a missing normalisation moves values by 1e-3 or more."""
    from data_utils.features.video import default_video_processor

    frames = make_frames(2, H, W)
    want = default_video_processor(frames, crop).numpy()
    got = restate(frames, crop, np.float64)
    assert got.shape == want.shape == (1, 2, 3, crop, crop)
    assert want.min() < -1.9 and want.max() > 2.4
    err = float(np.abs(got - want).max())
    print(f"{H} x {W} -> {crop}: max |float64 restatement - default_video_processor| = {err:.3e}")
    assert err <= 2e-6


def test_frontend_field_of_the_video_plugin():
    import pydantic

    from data_utils.features.video import VJEPA2, HipVideoProcessor

    assert VJEPA2().frontend == "host"
    assert VJEPA2(frontend="hip").frontend == "hip"
    with pytest.raises(pydantic.ValidationError):
        VJEPA2(frontend="gpu")
    assert "frontend" in VJEPA2._exclude_from_cls_uid() and "device" in VJEPA2._exclude_from_cls_uid()
    with pytest.raises(ValueError):
        VJEPA2(frontend="hip").attach(object(), processor=lambda fr: fr)
    VJEPA2(frontend="hip").attach(object())
    VJEPA2().attach(object(), processor=lambda fr: fr)
    proc = HipVideoProcessor(crop_size=64)
    assert proc.crop_size == 64
    with pytest.raises(ValueError):
        proc(np.zeros((2, 8, 8, 3), np.float32))


def test_video_preprocess_argument_errors_do_not_need_a_gpu():
    from tribe_hip import TribeHipError, _lib, ops

    with pytest.raises(TribeHipError):
        ops.video_preprocess(torch.zeros(2, 40, 40, 3, dtype=torch.uint8), [0, 1], 32)        # a host tensor

    handle = _lib.lib()
    first = np.arange(2, 34, dtype=np.int32)                                       # 36 -> 36, crop 32: identity, one tap
    ones = np.ones((32, 1), np.float32)
    src = np.array([0, 1, 1], np.int32)
    mean, std = np.array(MEAN, np.float32), np.array(STD, np.float32)
    addr = ones.ctypes.data                                                          # any non-null address: nothing is dereferenced or launched before the checks pass

    def call(frames=addr, n_src=2, H=36, W=36, src=src, resized=(36, 36), crop=32, first_h=first, first_w=first, w_h=ones, w_w=ones,
             taps_h=1, taps_w=1, std=std, out=addr, ws=addr, ws_bytes=1 << 20):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return handle.tribe_video_preprocess_fwd(frames, n_src, H, W, p(src), len(src) if src is not None else 1, resized[0], resized[1], crop,
                                                 p(first_h), p(w_h), taps_h, p(first_w), p(w_w), taps_w, p(mean), p(std), out, ws, ws_bytes, None)

    assert call(src=np.array([0, 2], np.int32)) < 0 and b"src[1] = 2" in handle.tribe_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(src=np.array([-1], np.int32)), "tribe_video_preprocess_fwd")
    assert call(H=33) < 0 and b"H tap window" in handle.tribe_last_error()                       # first_h + taps passes the frame
    assert call(W=33) < 0 and b"W tap window" in handle.tribe_last_error()
    assert call(first_h=first - 3) < 0 and call(first_w=first[::-1].copy()) < 0                    # negative / moving backwards
    assert call(resized=(36, 31)) < 0 and b"crop" in handle.tribe_last_error()
    assert call(frames=None) < 0 and b"null" in handle.tribe_last_error()
    assert call(src=None) < 0 and call(first_h=None) < 0 and call(w_w=None) < 0 and call(out=None) < 0 and call(ws=None) < 0
    assert call(n_src=0) < 0 and call(crop=0) < 0 and call(taps_h=0) < 0 and call(taps_h=65) < 0
    assert call(std=np.array([0.2, 0.0, 0.2], np.float32)) < 0
    assert call(ws_bytes=16) < 0 and b"workspace" in handle.tribe_last_error()

    wsb = handle.tribe_video_preprocess_workspace_bytes
    assert wsb(3, 32, 1, 1) >= (32 + 32 + 3 + 32 + 32) * 4
    assert wsb(0, 32, 1, 1) == 0 and wsb(3, 0, 1, 1) == 0 and wsb(3, 32, 0, 1) == 0 and wsb(3, 32, 65, 1) == 0
