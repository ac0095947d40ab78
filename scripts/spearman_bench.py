"""MultidimSpearmanCorrCoef (csrc/rank_corr.hip) against a torch composition of the same statistic, at the validation shape.

GPU box:  python scripts/spearman_bench.py [out.txt]      (default: profiles/spearman_bench.txt)

One round = 16 updates of predictions / targets f32 [64, 1000, 100] (n = 102400 samples per output column, 16 distinct input pairs)
followed by one compute().  The update phase and the compute phase are timed separately, each between two device synchronisations
(wall clock: the compute of the HIP route reads its sample counts back before it launches, and that belongs to its time).  The two
routes alternate within every round; one untimed round of each comes first.  The file records the median and the range (min .. max) of
ROUNDS rounds.

Routes:
  hip     MultidimSpearmanCorrCoef.update (tribe_rank_append: positions + tiled scatter into [1, V, capacity]) and .compute()
          (tribe_spearman_columns: n > 16384, so chunk sort in LDS, pairwise merge passes, ranking pass, int64 sums)
  torch   update: the batch copied into a preallocated [V, n] buffer as permute(1, 0, 2).reshape(V, B T); compute: per block of 50
          columns torch.sort, two torch.searchsorted (left, right) per tensor for the doubled centred ranks a = lb + ub - n -- the same
          average ranks -- then sum a b / sqrt(sum a^2 sum b^2) in f64 and the mean over columns
"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from modeling_utils.metrics import MultidimSpearmanCorrCoef  # noqa: E402
from tribe_hip import ops  # noqa: E402
from tribe_hip._lib import lib  # noqa: E402

B, V, T, UPDATES, ROUNDS, BLOCK = 64, 1000, 100, 16, 10, 50
N = B * T * UPDATES
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "spearman_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
pairs = []
for _ in range(UPDATES):
    pred = torch.randn(B, V, T, generator=g, device=dev)
    pred[:, ::7] = torch.round(pred[:, ::7] * 4)                       # every seventh column quantised: ties
    pairs.append((pred, 0.5 * pred + torch.randn(B, V, T, generator=g, device=dev)))


class TorchSpearman:
    def __init__(self):
        self.p = torch.empty(V, N, device=dev)
        self.t = torch.empty(V, N, device=dev)
        self.at = 0

    def update(self, pred, true):
        k = pred.shape[0] * pred.shape[2]
        self.p[:, self.at: self.at + k] = pred.permute(1, 0, 2).reshape(V, k)
        self.t[:, self.at: self.at + k] = true.permute(1, 0, 2).reshape(V, k)
        self.at += k

    @staticmethod
    def _ranks(x):
        s = torch.sort(x, dim=1).values
        return torch.searchsorted(s, x, right=False) + torch.searchsorted(s, x, right=True) - x.shape[1]

    def per_output(self):
        rho = torch.empty(V, dtype=torch.float64, device=dev)
        for v0 in range(0, V, BLOCK):
            a = self._ranks(self.p[v0: v0 + BLOCK, : self.at].contiguous()).double()
            b = self._ranks(self.t[v0: v0 + BLOCK, : self.at].contiguous()).double()
            rho[v0: v0 + BLOCK] = (a * b).sum(1) / torch.sqrt((a * a).sum(1) * (b * b).sum(1))
        return rho

    def compute(self):
        return self.per_output().mean().float()

    def reset(self):
        self.at = 0


def one_round(metric):
    metric.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for pred, true in pairs:
        metric.update(pred, true)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    value = float(metric.compute())
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1, value


routes = {"hip": MultidimSpearmanCorrCoef(num_outputs=V), "torch": TorchSpearman()}
values = {name: one_round(metric)[2] for name, metric in routes.items()}            # warm-up, and the buffers reach their size
# the two routes must agree before a time means anything: rho per column within 2^-24 (f32 rounding of the HIP route)
diff = float((routes["hip"].per_output()[0].double() - routes["torch"].per_output()).abs().max())
assert diff <= 2.0**-24, f"per-column rho differs by {diff:.3e}"
times = {name: ([], []) for name in routes}
for _ in range(ROUNDS):
    for name, metric in routes.items():
        up, comp, _ = one_round(metric)
        times[name][0].append(up)
        times[name][1].append(comp)

state_bytes = 2 * 4 * N * V
ws_bytes = lib().tribe_spearman_workspace_bytes(N, V, 0)
lines = [f"Spearman rank correlation, {UPDATES} updates of pred / true f32 [{B}, {V}, {T}] (n = {N} samples x {V} columns) then one compute()",
         f"{ROUNDS} rounds after one warm-up round, routes alternating within a round; wall clock between device synchronisations",
         f"{'route':6s} {'phase':22s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}"]
for name, (ups, comps) in times.items():
    for phase, ts in ((f"{UPDATES} updates", ups), ("compute", comps), ("round", [u + c for u, c in zip(ups, comps)])):
        lines.append(f"{name:6s} {phase:22s} {statistics.median(ts) * 1e3:10.2f} {min(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
for phase, k in (("updates", 0), ("compute", 1)):
    hip, ref = times["hip"][k], times["torch"][k]
    verdict = "ahead, ranges do not overlap" if max(hip) < min(ref) else "behind, ranges do not overlap" if min(hip) > max(ref) else "ranges overlap"
    lines.append(f"{phase}: hip / torch median = {statistics.median(hip) / statistics.median(ref):.3f} ({verdict})")
lines.append(f"compute() hip {values['hip']:.9f}, torch {values['torch']:.9f}; largest per-column difference of rho {diff:.2e}")
lines.append(f"sample state 2 * 4 * n * V = {state_bytes / 1e6:.1f} MB (capacity after doubling: {routes['hip']._pred.shape[2]} samples per column, "
             f"{2 * routes['hip']._pred.numel() * 4 / 1e6:.1f} MB allocated); merge workspace {ws_bytes / 1e6:.1f} MB; default chunk "
             f"{ops.spearman_default_chunk()}")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
