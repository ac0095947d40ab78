"""Regression-metric statistics kernel against the Pearson statistics kernel and a torch-composed route, at the validation shape.

GPU box:  python scripts/regression_metrics_bench.py [out.txt]      (default: profiles/regression_metrics_bench.txt)

Inputs: predictions and targets f32 [64, 1000, 100] (51.2 MB per call, 8 bytes read per element).  Six input pairs (307 MB, more
than the 256 MiB Infinity Cache) are used in rotation, so a call does not re-read what the call before it left on the die.  Per
route: HIP-event time of 300 calls after 30 warm-up calls, repeated 5 times with the routes alternating; the file records the median,
the spread (max - min of the 5 repeats) and the algorithmic bytes over the median time as a fraction of the 8 TB/s HBM3E peak.

Routes:
  regression rows     tribe_regression_stats_update on [B, V, T] contiguous (bvt_stats_rows_kernel<RegressionAcc>)
  pearson rows        tribe_pearson_stats_update on the same tensors (bvt_stats_rows_kernel<PearsonAcc>): same bytes, two fewer f64 operations per
                      element
  regression strided  the '(b t) v' matrix viewed as [B, V, T] (bvt_stats_strided_kernel<RegressionAcc>)
  pearson strided     the same view (bvt_stats_strided_kernel<PearsonAcc>)
  torch composed      d = t.double() - p.double(); the five sums over (b, t) with torch reductions
"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from tribe_hip import ops  # noqa: E402

B, V, T, HBM_PEAK = 64, 1000, 100, 8.0e12
N_PAIRS, WARMUP, CALLS, REPEATS = 6, 30, 300, 5
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "regression_metrics_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
pairs = []
for _ in range(N_PAIRS):
    pred = torch.randn(B, V, T, generator=g, device=dev)
    pairs.append((pred, 0.5 * pred + torch.randn(B, V, T, generator=g, device=dev)))
views = [(p.permute(0, 2, 1).reshape(B * T, V).contiguous().view(B, T, V).transpose(1, 2),
          t.permute(0, 2, 1).reshape(B * T, V).contiguous().view(B, T, V).transpose(1, 2)) for p, t in pairs]
nbytes = 8 * B * V * T
stats = torch.zeros(1, V, 6, dtype=torch.float64, device=dev)


def torch_composed(p, t):
    t64 = t.double()
    d = t64 - p.double()
    return torch.stack([d.sum((0, 2)), (d * d).sum((0, 2)), d.abs().sum((0, 2)), t64.sum((0, 2)), (t64 * t64).sum((0, 2))], -1)


routes = {
    "regression rows": (lambda p, t: ops.regression_stats_update(stats, p, t), pairs),
    "pearson rows": (lambda p, t: ops.pearson_stats_update(stats, p, t), pairs),
    "regression strided": (lambda p, t: ops.regression_stats_update(stats, p, t), views),
    "pearson strided": (lambda p, t: ops.pearson_stats_update(stats, p, t), views),
    "torch composed": (torch_composed, pairs),
}


def timed(fn, inputs, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(*inputs[i % len(inputs)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e-3


for fn, inputs in routes.values():
    timed(fn, inputs, WARMUP)
times = {name: [] for name in routes}
for _ in range(REPEATS):
    for name, (fn, inputs) in routes.items():
        times[name].append(timed(fn, inputs, CALLS))

# the statistics the two kernels leave must agree with the composed route before a time means anything
stats.zero_()
ops.regression_stats_update(stats, *pairs[0])
want = torch_composed(*pairs[0])
mags = want.abs()
mags[:, 0], mags[:, 3] = want[:, 2], pairs[0][1].double().abs().sum((0, 2))   # sum d and sum t against the sums of their magnitudes
rel = float(((stats[0, :, :5] - want).abs() / mags).max())
assert rel < 1e-12, f"statistics differ from the composed route by {rel:.3e} of the summed magnitudes"

lines = [f"regression metrics statistics, pred / true f32 [{B}, {V}, {T}], {nbytes / 1e6:.1f} MB read per call, {N_PAIRS} input pairs in rotation",
         f"{CALLS} calls per timing after {WARMUP} warm-up calls, {REPEATS} repeats, routes alternating; device events",
         f"{'route':22s} {'median us':>10s} {'spread us':>10s} {'TB/s':>6s} {'of 8 TB/s':>10s}"]
for name, ts in times.items():
    med = statistics.median(ts)
    lines.append(f"{name:22s} {med * 1e6:10.1f} {(max(ts) - min(ts)) * 1e6:10.1f} {nbytes / med / 1e12:6.2f} {nbytes / med / HBM_PEAK:10.1%}")
lines.append(f"largest difference of the five sums, kernel vs composed route, relative to the summed magnitudes: {rel:.2e}")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
