"""Video front end of one V-JEPA2 clip (64 decoded uint8 frames -> pixel_values_videos f32 [1, 64, 3, 256, 256]) at two frame sizes,
720 x 1280 and 480 x 854: the host route the plugin uses by default (`default_video_processor` in torch on the CPU + the upload of
its float32 result; wall clock, ends in a device synchronise) against the HIP route (`ops.video_preprocess` on uint8 frames already
in HBM; HIP events around several calls), plus the upload of the uint8 frames the HIP route needs instead (wall clock, ends in a
synchronise; a clip without shared frames -- the plugin uploads each distinct frame of a launch group once).  Both routes are
warmed up, then alternated `--repeat` times; medians and the spread are printed, and the two results are compared.
Needs a GPU: there is no CPU timing of the HIP route.

    python scripts/video_frontend_bench.py [--repeat 7] [--iters 20] [--threads 16]
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
ap.add_argument("--threads", type=int, default=16, help="torch CPU threads of the host route")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--crop", type=int, default=256)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("video_frontend_bench: no GPU visible; the HIP route is not timed on a CPU")

from data_utils.features.video import default_video_processor  # noqa: E402
from tribe_hip import ops  # noqa: E402

torch.set_num_threads(args.threads)
dev = torch.device("cuda")
index = np.arange(args.frames)


def ms(xs: list[float]) -> str:
    return f"{statistics.median(xs) * 1e3:9.3f} ms (min {min(xs) * 1e3:.3f}, max {max(xs) * 1e3:.3f})"


def bench(H: int, W: int) -> None:
    frames = np.random.default_rng(H).integers(0, 256, (args.frames, H, W, 3), dtype=np.uint8)

    def host_route() -> tuple[torch.Tensor, float]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pix = default_video_processor(frames, args.crop).to(dev)
        torch.cuda.synchronize()
        return pix, time.perf_counter() - t0

    def upload() -> tuple[torch.Tensor, float]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize()
        return up, time.perf_counter() - t0

    def hip_route(dev_frames: torch.Tensor) -> tuple[torch.Tensor, float]:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            pix = ops.video_preprocess(dev_frames, index, args.crop)
        stop.record()
        stop.synchronize()
        return pix, start.elapsed_time(stop) * 1e-3 / args.iters

    dev_frames, _ = upload()
    host_route()
    hip_route(dev_frames)                                               # warm-up of both routes at the timed shape
    t_host, t_up, t_hip = [], [], []
    for _ in range(args.repeat):
        want, t = host_route()
        t_host.append(t)
        dev_frames, t = upload()
        t_up.append(t)
        got, t = hip_route(dev_frames)
        t_hip.append(t)
    err = float((got[None] - want).abs().max())
    nh, nw = ops.video_resized_size(H, W, args.crop)
    (first_h, w_h), (first_w, w_w) = (ops.aa_resize_taps(n, m, (m - args.crop) // 2, args.crop) for n, m in ((H, nh), (W, nw)))
    taps = (w_h.shape[1], w_w.shape[1])
    # what the crop window needs of a frame: the rows and the 3-byte pixels its tap windows reach
    read_bytes = args.frames * int(first_h[-1] + taps[0] - first_h[0]) * int(first_w[-1] + taps[1] - first_w[0]) * 3
    in_bytes, out_bytes = frames.nbytes, args.frames * 3 * args.crop * args.crop * 4
    print(f"video front end, one clip: {args.frames} frames of {H} x {W} -> resize {nh} x {nw} ({taps[0]} x {taps[1]} taps) -> crop {args.crop}; "
          f"{args.repeat} alternations, {args.threads} CPU threads")
    print(f"  host route (default_video_processor + upload of {out_bytes / 1e6:.1f} MB float32), wall clock : {ms(t_host)}")
    print(f"  HIP route  (tribe_video_preprocess_fwd, one launch), HIP events, {args.iters:3d} calls/pair : {ms(t_hip)}")
    print(f"  upload of the {in_bytes / 1e6:.1f} MB of uint8 frames the HIP route needs instead, wall clock : {ms(t_up)}")
    print(f"  HIP kernel: the crop window needs {read_bytes / 1e6:.1f} MB of the frames, {out_bytes / 1e6:.1f} MB written -> "
          f"{(read_bytes + out_bytes) / statistics.median(t_hip) * 1e-12:.2f} TB/s over the whole call (HBM peak 8)")
    print(f"  max |hip - host| over the clip: {err:.3e}")


for H, W in ((720, 1280), (480, 854)):
    bench(H, W)
