"""Resampling of one 60 s stereo chunk to 16 kHz, from 44.1 kHz and from 48 kHz, as `Wav2VecBert._compute` meets it: the waveform
[n, 2] float32 sits on the host (what `event.read()` delivers) and the 16 kHz waveform is wanted in HBM.

  HIP route     upload of the native-rate waveform, then `ops.resample_frac` (julius' filter, csrc/resample.hip); the two are
                timed separately with HIP events (`--iters` kernel calls inside one event pair)
  host, scipy   today's default `Wav2VecBert._resample_wav` (`scipy.signal.resample_poly`, one thread) + the upload of its 16 kHz
                result; wall clock, ends in a device synchronise
  host, julius  julius' ResampleFrac restated with torch (`F.pad(replicate)` + strided `conv1d` with the same float32 table) at
                16 threads + the upload of its result; wall clock, ends in a device synchronise

All routes are warmed up at the timed shapes, then alternated `--repeat` times; medians and the spread are printed.  The HIP result
is compared with the torch restatement (same filter) and with scipy (a different filter: the distance is the filters', for scale).
Needs a GPU: there is no CPU timing of the HIP route.

    python scripts/resample_bench.py [--repeat 7] [--iters 20]
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
ap.add_argument("--repeat", type=int, default=7, help="alternations of the routes")
ap.add_argument("--iters", type=int, default=20, help="HIP kernel calls inside one event pair")
ap.add_argument("--seconds", type=int, default=60)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("resample_bench: no GPU visible; the HIP route is not timed on a CPU")

from data_utils.features.audio import Wav2VecBert, julius_resample_kernels, resample_output_length  # noqa: E402
from tribe_hip import ops  # noqa: E402

NEW_SR, THREADS, dev = 16_000, 16, torch.device("cuda")
torch.set_num_threads(THREADS)
plugin = Wav2VecBert()


def ms(xs: list[float]) -> str:
    return f"{statistics.median(xs) * 1e3:9.3f} ms (min {min(xs) * 1e3:.3f}, max {max(xs) * 1e3:.3f})"


def events() -> tuple[torch.cuda.Event, torch.cuda.Event]:
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def bench(old_sr: int) -> None:
    rng = np.random.default_rng(old_sr)
    n = args.seconds * old_sr
    wav = torch.from_numpy((0.1 * rng.standard_normal((n, 2))).astype(np.float32))
    old, new, width, table = julius_resample_kernels(old_sr, NEW_SR)
    m = resample_output_length(n, old_sr, NEW_SR)

    def hip_upload() -> tuple[torch.Tensor, float]:
        start, stop = events()
        torch.cuda.synchronize()
        start.record()
        d = wav.to(dev)
        stop.record()
        stop.synchronize()
        return d, start.elapsed_time(stop) * 1e-3

    def hip_kernel(d: torch.Tensor) -> tuple[torch.Tensor, float]:
        start, stop = events()
        start.record()
        for _ in range(args.iters):
            (out,) = ops.resample_frac(d, old_sr, NEW_SR)
        stop.record()
        stop.synchronize()
        return out, start.elapsed_time(stop) * 1e-3 / args.iters

    def host_scipy() -> tuple[torch.Tensor, float]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = plugin._resample_wav(wav, old_sr, NEW_SR).to(dev)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def host_julius() -> tuple[torch.Tensor, float]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = torch.nn.functional.pad(wav.t()[:, None, :], (width, width + old), mode="replicate")      # [2, 1, n + 2 W + old]
        y = torch.nn.functional.conv1d(x, table[:, None, :], stride=old)                              # [2, new, n // old + 1]
        out = y.transpose(1, 2).reshape(2, -1)[:, :m].t().contiguous().to(dev)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    d, _ = hip_upload()
    hip_kernel(d)
    host_scipy()
    host_julius()                                                          # warm-up of every route at the timed shape
    t_up, t_k, t_sp, t_ju = [], [], [], []
    for _ in range(args.repeat):
        d, t = hip_upload()
        t_up.append(t)
        got, t = hip_kernel(d)
        t_k.append(t)
        sp, t = host_scipy()
        t_sp.append(t)
        ju, t = host_julius()
        t_ju.append(t)
    hip_total = statistics.median(t_up) + statistics.median(t_k)
    k = min(sp.shape[0], m)
    flops = 2.0 * m * 2 * table.shape[1]
    print(f"{old_sr} -> {NEW_SR} Hz ({old} / {new}, {table.shape[1]} taps), {args.seconds} s x 2 channels: {n} -> {m} samples, "
          f"{n * 8 / 2**20:.1f} MiB up at the native rate against {m * 8 / 2**20:.1f} MiB at 16 kHz; {args.repeat} alternations")
    print(f"  HIP route, upload of the native-rate waveform, HIP events                    : {ms(t_up)}")
    print(f"  HIP route, tribe_resample_frac_fwd, HIP events, {args.iters:3d} calls/pair              : {ms(t_k)}"
          f"   ({flops / statistics.median(t_k) * 1e-12:.2f} TFLOP/s f32 on the vector ALU)")
    print(f"  HIP route, upload + kernel (sum of the medians)                              : {hip_total * 1e3:9.3f} ms")
    print(f"  host, scipy resample_poly (1 thread) + upload of the 16 kHz result, wall     : {ms(t_sp)}   = {statistics.median(t_sp) / hip_total:.1f} x the HIP route")
    print(f"  host, julius restated in torch (pad + conv1d, {THREADS} threads) + upload, wall     : {ms(t_ju)}   = {statistics.median(t_ju) / hip_total:.1f} x the HIP route")
    print(f"  max |hip - torch restatement| {float((got - ju).abs().max()):.3e} (same filter);  max |hip - scipy| {float((got[:k] - sp[:k]).abs().max()):.3e} "
          f"(different filters; scipy returns {sp.shape[0]} samples)")


for rate in (44_100, 48_000):
    bench(rate)
