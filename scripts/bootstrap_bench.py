"""BootstrapPearsonCorrCoef.intervals() (csrc/bootstrap.hip) against a torch composition of the same resampling, at the validation shape.

GPU box:  python scripts/bootstrap_bench.py [out.txt]      (default: profiles/bootstrap_bench.txt)

Setup: 16 updates of predictions / targets f32 [64, 1000, 100] give 1024 blocks x 1000 parcels of f64 statistics (49 MB).  One round =
one intervals() with 1000 replicates: counts, the resampled r of every (replicate, parcel) and of the mean over parcels, then the
2.5 % / 97.5 % quantiles, the standard deviation and the p-value per column.  Each call is timed between two device synchronisations
(wall clock); the two routes alternate within every round; two untimed rounds of each come first.  The file records the median and
the range (min .. max) of ROUNDS rounds, and the time of the 16 updates (the same kernel on both routes) for scale.

Routes:
  hip     tribe_bootstrap_counts (Philox draw + LDS histogram), tribe_bootstrap_pearson (count-weighted f64 sums in registers, the
          finaliser, row means), tribe_bootstrap_summary twice (LDS sort per column)
  torch   counts by scatter_add_ from the same drawn indices (precomputed: the draw itself is not timed on this route),
          counts.double() @ stats.view(blocks, V * 6) (an f64 GEMM), the element-wise finaliser, torch.nanquantile / std / comparisons
"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from modeling_utils.metrics import BootstrapPearsonCorrCoef  # noqa: E402
from tribe_hip import ops  # noqa: E402

B, V, T, UPDATES, N_BOOT, ROUNDS, WARMUP = 64, 1000, 100, 16, 1000, 12, 2
Q = (0.025, 0.975)
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "bootstrap_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
pairs = []
for _ in range(UPDATES):
    true = torch.randn(B, V, T, generator=g, device=dev)
    pairs.append((0.3 * true + torch.randn(B, V, T, generator=g, device=dev), true))

metric = BootstrapPearsonCorrCoef(num_outputs=V, num_bootstraps=N_BOOT, quantiles=Q, seed=0)


def feed():
    metric.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for pred, true in pairs:
        metric.update(pred, true)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


update_times = [feed() for _ in range(3)][1:]
NB = metric._n
stats = metric._stats[:NB]
counts = ops.bootstrap_counts(0, N_BOOT, NB, dev)
indices = torch.repeat_interleave(torch.arange(NB, device=dev).repeat(N_BOOT), counts.flatten().long()).view(N_BOOT, NB)   # the same draws


def torch_intervals():
    c = torch.zeros(N_BOOT + 1, NB, dtype=torch.float64, device=dev)
    c[:N_BOOT].scatter_add_(1, indices, torch.ones(N_BOOT, NB, dtype=torch.float64, device=dev))
    c[N_BOOT] = 1.0
    s = (c @ stats.view(NB, V * 6)).view(N_BOOT + 1, V, 6)
    sx, sy, sxx, syy, sxy, n = s.unbind(-1)
    eps = torch.finfo(torch.float64).eps
    vx, vy = sxx - sx * sx / n, syy - sy * sy / n
    vx, vy = torch.where(vx > n * eps * sxx, vx, 0.0), torch.where(vy > n * eps * syy, vy, 0.0)
    r = ((sxy - sx * sy / n) / torch.sqrt(vx * vy)).clamp(-1.0, 1.0)
    r = torch.where((n >= 2) & (vx > 0) & (vy > 0), r, float("nan")).float()
    table = torch.cat([r, r.double().mean(1, keepdim=True).float()], 1)
    rep = table[:N_BOOT]
    q = torch.nanquantile(rep, torch.tensor(Q, device=dev), dim=0)
    valid = ~torch.isnan(rep)
    m = valid.sum(0)
    mean = torch.nansum(rep.double(), 0) / m
    sd = torch.sqrt(torch.nansum(torch.where(valid, (rep.double() - mean) ** 2, 0.0), 0) / (m - 1)).float()
    p = ((1.0 + (valid & (rep <= 0)).sum(0).double()) / (m.double() + 1.0)).float()
    return table[N_BOOT], q, sd, p


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


routes = {"hip": metric.intervals, "torch": torch_intervals}
for _ in range(WARMUP):
    outs = {name: timed(fn)[1] for name, fn in routes.items()}
# the two routes must agree before a time means anything
hip, (t_obs, t_q, t_sd, t_p) = outs["hip"], outs["torch"]
d_obs = float((torch.cat([hip.observed, hip.mean_observed[None]]).double() - t_obs.double()).abs().max())
d_q = float((torch.cat([torch.stack([hip.lower, hip.upper]), torch.stack([hip.mean_lower, hip.mean_upper])[:, None]], 1).double() - t_q.double()).abs().max())
d_sd = float((torch.cat([hip.std, hip.mean_std[None]]).double() / t_sd.double() - 1).abs().max())
p_same = bool(torch.equal(torch.cat([hip.p_value, hip.mean_p_value[None]]), t_p))
assert d_obs <= 2.0**-23 and d_q <= 2.0**-23 and d_sd <= 1e-5, (d_obs, d_q, d_sd)

times = {name: [] for name in routes}
for _ in range(ROUNDS):
    for name, fn in routes.items():
        times[name].append(timed(fn)[0])

lines = [f"block bootstrap of the per-parcel Pearson r: {NB} blocks ({UPDATES} updates of pred / true f32 [{B}, {V}, {T}]) x {V} parcels, "
         f"{N_BOOT} replicates, quantiles {Q}",
         f"{ROUNDS} rounds after {WARMUP} warm-up rounds, routes alternating within a round; wall clock between device synchronisations",
         f"{'route':6s} {'phase':22s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}"]
for name, ts in times.items():
    lines.append(f"{name:6s} {'intervals()':22s} {statistics.median(ts) * 1e3:10.2f} {min(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
lines.append(f"{'both':6s} {f'{UPDATES} updates':22s} {statistics.median(update_times) * 1e3:10.2f} {min(update_times) * 1e3:9.2f} "
             f"{max(update_times) * 1e3:9.2f}   (2 rounds; tribe_pearson_stats_update, one group per batch row)")
h, t = times["hip"], times["torch"]
verdict = "ahead, ranges do not overlap" if max(h) < min(t) else "not ahead, ranges do not overlap" if min(h) > max(t) else "ranges overlap"
lines.append(f"intervals(): hip / torch median = {statistics.median(h) / statistics.median(t):.3f} ({verdict})")
lines.append(f"agreement: observed r within {d_obs:.2e}, interval ends within {d_q:.2e}, std within relative {d_sd:.2e}, p-values equal: {p_same}")
lines.append(f"memory: state 48 * blocks * V = {48 * NB * V / 1e6:.1f} MB ({metric._stats.numel() * 8 / 1e6:.1f} MB allocated), counts "
             f"{4 * N_BOOT * NB / 1e6:.1f} MB, replicates {4 * (N_BOOT + 1) * (V + 1) / 1e6:.1f} MB; the torch route also writes the "
             f"[{N_BOOT + 1}, {V}, 6] f64 sums ({48 * (N_BOOT + 1) * V / 1e6:.1f} MB)")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
