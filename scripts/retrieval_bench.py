"""Retrieval metric timings on one GPU: µs per within-batch `TopkAcc.update_bvt` (B = 16, V = 1000, T' = 100, the retrieval branch
of `_run_step`) and ms for one 8192 x 8192 gallery `Rank.update` (V = 1000).  HIP events around many back-to-back calls.

    python scripts/retrieval_bench.py [--iters 200]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]

import torch  # noqa: E402

from modeling_utils.metrics.metrics import Rank, TopkAcc  # noqa: E402


def _time_ms(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(16, 1000, 100, device="cuda", generator=g)
    target = 0.2 * pred + torch.randn(16, 1000, 100, device="cuda", generator=g)
    top1 = TopkAcc(topk=1)

    def batch_update():
        top1.update_bvt(pred, target)
        if top1._count > 1 << 16:
            top1.reset()

    us_batch = 1e3 * _time_ms(batch_update, args.iters)
    x = torch.randn(8192, 1000, device="cuda", generator=g)
    y = 0.03 * x + torch.randn(8192, 1000, device="cuda", generator=g)
    rank = Rank()

    def gallery_update():
        rank.update(x, y)
        rank.reset()

    ms_gallery = _time_ms(gallery_update, max(3, args.iters // 50))
    flops = 2.0 * 8192 * 8192 * 1000 * (1 + 1 / 128)   # + the true-score tile of each workgroup
    print(json.dumps({"update_bvt_B16_V1000_T100_us": round(us_batch, 2), "gallery_8192x8192_V1000_ms": round(ms_gallery, 3),
                      "gallery_tflops": round(flops / ms_gallery / 1e9, 1)}))


if __name__ == "__main__":
    main()
