"""Audio front end of one 149 s window (chunks of 60 s + 60 s + 29 s at 16 kHz, two channels, as scripts/e2e_bench.py cuts it):
the host route of the reference (`_preprocess_wav` in torch + the HF SeamlessM4TFeatureExtractor + the upload of the
features; wall clock, ends in a device synchronise) against the HIP route (`ops.w2vbert_fbank` on waveforms already in
HBM; HIP events around all three chunks in one call), plus the upload of the waveforms the HIP route needs instead.
Both routes are warmed up, then alternated `--repeat` times; medians and the spread are printed, and the two results
are compared.  Needs a GPU: there is no CPU timing of the HIP route.

    python scripts/fbank_bench.py [--repeat 7] [--iters 20]
"""

from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "algonauts-2025_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=7, help="alternations of the two routes")
ap.add_argument("--iters", type=int, default=20, help="HIP calls inside one event pair")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("fbank_bench: no GPU visible; the HIP route is not timed on a CPU")

from transformers import SeamlessM4TFeatureExtractor  # noqa: E402

from data_utils.features.audio import Wav2VecBert  # noqa: E402
from tribe_hip import ops  # noqa: E402

SR, dev = 16_000, torch.device("cuda")
rng = np.random.default_rng(0)
seconds = (60, 60, 29)
wavs = [torch.from_numpy((0.1 * rng.standard_normal((s * SR, 2))).astype(np.float32)) for s in seconds]     # [n, 2] as event.read() delivers
plugin, fe = Wav2VecBert(), SeamlessM4TFeatureExtractor()


def host_route() -> tuple[list[torch.Tensor], float]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = []
    for w in wavs:
        mono = plugin._preprocess_wav(w)
        feats = fe(mono.numpy(), return_tensors="pt", sampling_rate=SR)["input_features"]
        out.append(feats.to(dev))
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def upload() -> tuple[list[torch.Tensor], float]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [w.to(dev) for w in wavs]
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def hip_route(dev_wavs: list[torch.Tensor]) -> tuple[torch.Tensor, list[int], float]:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.iters):
        feats, lengths = ops.w2vbert_fbank(dev_wavs, zscore=True)
    stop.record()
    stop.synchronize()
    return feats, lengths, start.elapsed_time(stop) * 1e-3 / args.iters


dev_wavs, _ = upload()
host_route()
hip_route(dev_wavs)                                                    # warm-up of both routes at the timed shapes
t_host, t_up, t_hip = [], [], []
for _ in range(args.repeat):
    want, t = host_route()
    t_host.append(t)
    dev_wavs, t = upload()
    t_up.append(t)
    feats, lengths, t = hip_route(dev_wavs)
    t_hip.append(t)

err = max(float((feats[i, : lengths[i]] - want[i][0]).abs().max()) for i in range(len(wavs)))
frames = sum(ops.fbank_frame_count(int(w.shape[0])) for w in wavs)
flops = frames * (2.0 * 400 * 512 + 2.0 * 258 * 96)                    # the MFMA work as launched: DFT 400 x 512 and mel 258 x 96 per frame


def ms(xs: list[float]) -> str:
    return f"{statistics.median(xs) * 1e3:9.3f} ms (min {min(xs) * 1e3:.3f}, max {max(xs) * 1e3:.3f})"


print(f"audio front end, one 149 s window: chunks of {seconds} s, 2 channels, {frames} frames -> rows {lengths}; {args.repeat} alternations")
print(f"  host route (_preprocess_wav + HF extractor + upload of features), wall clock : {ms(t_host)}")
print(f"  HIP route  (tribe_fbank_fwd, 3 chunks in one call), HIP events, {args.iters:3d} calls/pair : {ms(t_hip)}")
print(f"  upload of the three waveforms the HIP route needs instead, wall clock        : {ms(t_up)}")
print(f"  matrix-pipe work of the HIP route {flops * 1e-9:.2f} GFLOP -> {flops / statistics.median(t_hip) * 1e-12:.2f} TFLOP/s over the whole call (f32 MFMA peak 157)")
print(f"  max |hip - host| over the three chunks: {err:.3e}")
