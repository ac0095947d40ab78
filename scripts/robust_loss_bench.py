"""The element-wise loss family (L1 / SmoothL1 / Huber / MSE: csrc/robust_loss.hip) against the path it replaces and against the
HBM roofline.

GPU box:  python scripts/robust_loss_bench.py [out.json]

Per kind, at [16, 1000, 100] (the reference's batch; 6.4 MB per tensor, launch-bound) and at [64, 1000, 1024] (the bench batch; 262 MB
per tensor, HBM-bound), forward + backward to a [B, V, T'] leaf of
  * the new path: the HIP loss's forward_bvt on the pair in place (partial sums, final sum, backward: three launches), and
  * the parent's path: the stock torch.nn loss on the two permuted, reshaped '(b t) d' copies, autograd back to the leaf.
At [64, 1000, 1024] the forward and the backward entry points are also timed alone, next to tribe_mse_fwd / tribe_mse_bwd (the family's
(MSE, mean) instance under its own names).  That pair is measured twice per round: the gap between its two figures is the spread
below which a difference means nothing on a shared machine.

Every variant of one shape is timed in turn within a round (alternated), ROUNDS rounds; the table shows the median over rounds of
the per-call HIP-event time.  ALGORITHMIC bytes: each input element read once (forward 8 n, backward 8 n) and each gradient element
written once (4 n); GB/s and the fraction of the 8 TB/s HBM3E peak follow from them (~6.3 TB/s is what a streaming kernel reaches in
practice).  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel durations."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

from modeling_utils.losses import hip_loss_for  # noqa: E402
from tribe_hip import ops  # noqa: E402
from tribe_hip._lib import check, lib  # noqa: E402

HBM_PEAK, ROUNDS = 8.0e12, 5
SHAPES = {(16, 1000, 100): 1000, (64, 1000, 1024): 30}      # shape -> launches per timed window
KINDS = {
    "L1Loss": (nn.L1Loss(), "l1", 0.0, "mean"),
    "SmoothL1Loss(beta=1)": (nn.SmoothL1Loss(), "smooth_l1", 1.0, "mean"),
    "HuberLoss(delta=1)": (nn.HuberLoss(), "huber", 1.0, "mean"),
    "MSELoss(sum)": (nn.MSELoss(reduction="sum"), "mse", 0.0, "sum"),
}
dev = torch.device("cuda")
stream = torch.cuda.current_stream().cuda_stream
one = torch.ones(1, device=dev)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def alternate(variants: dict, reps: int) -> dict:
    """{name: fn} -> {name: [seconds per call, one per round]}, every variant timed once per round, in turn."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(window(fn, reps))
    return times


def row(name: str, secs: list, nbytes: int) -> dict:
    s = statistics.median(secs)
    print(f"  {name:58s} {s * 1e6:9.1f} us  (min {min(secs) * 1e6:9.1f}, max {max(secs) * 1e6:9.1f})  {nbytes / s / 1e9:8.1f} GB/s  "
          f"{nbytes / s / HBM_PEAK:6.1%} of peak")
    return {"median_us": round(s * 1e6, 1), "min_us": round(min(secs) * 1e6, 1), "max_us": round(max(secs) * 1e6, 1),
            "algorithmic_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / s / 1e9, 1), "frac_of_8TBps": round(nbytes / s / HBM_PEAK, 4)}


out = {"dtype": "f32", "hbm_peak_TBps": HBM_PEAK / 1e12, "rounds": ROUNDS, "shapes": {}}
for (B, V, T), reps in SHAPES.items():
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(B, V, T, generator=g, device=dev).requires_grad_()
    true = 0.5 * pred.detach() + 0.8 * torch.randn(B, V, T, generator=g, device=dev)
    n = pred.numel()
    dpred = torch.empty(B, V, T, device=dev)
    print(f"[{B}, {V}, {T}]  ({4 * n / 1e6:.1f} MB per tensor), {reps} calls per window, {ROUNDS} rounds")
    variants, check_values = {}, {}
    for name, (stock, kind, param, reduction) in KINDS.items():
        hip = hip_loss_for(stock)

        def new_path(hip=hip):
            pred.grad = None
            hip.forward_bvt(pred, true).backward()

        def parent_path(stock=stock):
            pred.grad = None
            stock(pred.permute(0, 2, 1).reshape(-1, V), true.permute(0, 2, 1).reshape(-1, V)).backward()

        variants[f"{name}: HIP forward_bvt + backward"] = new_path
        variants[f"{name}: torch on '(b t) d' copies + backward"] = parent_path
        # both paths compute the same thing (f32 torch as the yardstick of this check; tests/test_gpu_robust_loss.py holds the f64 one)
        new_path()
        got_loss, got_grad = float(hip.forward_bvt(pred.detach(), true)), pred.grad.clone()
        parent_path()
        want_loss = float(stock(pred.detach(), true))
        check_values[name] = {"loss_rel_diff": abs(got_loss - want_loss) / abs(want_loss),
                              "grad_max_abs_diff_over_max": float((got_grad - pred.grad).abs().max() / pred.grad.abs().max())}
    shape_out = {"paths_fwd_bwd": {}, "agreement_with_torch_f32": check_values}
    for name, secs in alternate(variants, reps).items():
        shape_out["paths_fwd_bwd"][name] = row(name, secs, 20 * n)
    if B * T >= 64 * 1024:
        p, t = pred.detach(), true

        ws = torch.empty(lib().tribe_mse_workspace_bytes(n), dtype=torch.uint8, device=dev)
        loss = torch.empty((), device=dev)

        def mse_fwd():
            check(lib().tribe_mse_fwd(p.data_ptr(), t.data_ptr(), n, loss.data_ptr(), ws.data_ptr(), ws.numel(), stream), "tribe_mse_fwd")

        def mse_bwd():
            check(lib().tribe_mse_bwd(p.data_ptr(), t.data_ptr(), n, one.data_ptr(), dpred.data_ptr(), stream), "tribe_mse_bwd")

        def elem_bwd(kind, param, reduction):
            check(lib().tribe_elem_loss_bwd(p.data_ptr(), t.data_ptr(), n, ops.ELEM_LOSS_KINDS[kind], param, ops.ELEM_LOSS_REDUCTIONS[reduction],
                                            one.data_ptr(), dpred.data_ptr(), stream), "tribe_elem_loss_bwd")

        # the MSE pair twice, around the new kernels: the gap between its two figures is the spread
        kernels = {"mse_fwd (first)": mse_fwd, "mse_bwd (first)": mse_bwd}
        for name, (_, kind, param, reduction) in KINDS.items():
            kernels[f"{name} fwd"] = lambda a=(kind, param, reduction): ops.elem_loss(p, t, *a)
            kernels[f"{name} bwd"] = lambda a=(kind, param, reduction): elem_bwd(*a)
        kernels["mse_fwd (second)"] = mse_fwd
        kernels["mse_bwd (second)"] = mse_bwd
        shape_out["entry_points"] = {}
        print("  entry points alone:")
        for name, secs in alternate(kernels, reps).items():
            shape_out["entry_points"][name] = row(name, secs, (8 if "fwd" in name else 12) * n)
    out["shapes"][f"{B}x{V}x{T}"] = shape_out
    for name, v in check_values.items():
        print(f"  {name}: loss rel diff vs torch f32 {v['loss_rel_diff']:.2e}, gradient max diff / max {v['grad_max_abs_diff_over_max']:.2e}")
if len(sys.argv) > 1:
    Path(sys.argv[1]).write_text(json.dumps(out, indent=1))
