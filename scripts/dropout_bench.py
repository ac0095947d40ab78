"""tribe_dropout_apply against torch.nn.functional.dropout on the same tensors, and the synthetic training step with and without ff_dropout.

GPU box:  python scripts/dropout_bench.py [out.txt]      (default: profiles/dropout_bench.txt)

Kernel part, p = 0.1:
  bf16 [16384, 12288] in place   the feed-forward hidden of B = 16 x T = 1024 (402 MB: larger than the 256 MiB Infinity Cache by itself; two
                                 tensors in rotation), 2 + 2 bytes per element; torch: F.dropout(..., inplace=True)
  f32  [4768, 3072]   out of place  an MLP projector's output slice (B = 16 x 298 rows), 4 + 4 bytes per element, as many input / output
                                 pairs in rotation as exceed the cache; torch: F.dropout into a fresh tensor
Routes alternate; per route the HIP-event time of CALLS calls after a warm-up, REPEATS times; the file records the median, the spread
(max - min of the repeats) and the algorithmic bytes over the median as a share of the 6.29 TB/s streaming rate the README uses.
Step part: scripts/train_bench.py's synthetic model (three 2 x 2048 modalities, 1000 parcels, 8 layers, hidden 3072) at B = 16, T = 1024,
forward + backward + HipAdam, ONE model whose ff_dropout is switched between 0 (exactly the launches of a model built without it) and 0.1;
wall-clock time per step over STEPS steps, the two settings alternating, ROUNDS rounds."""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tribe_hip import ops  # noqa: E402

STREAM_RATE, CACHE, P = 6.29e12, 256 << 20, 0.1
WARMUP, REPEATS = 5, 5
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "dropout_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, n_sets, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i % n_sets)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e-3


def run(routes, n_sets, calls):
    """{name: [seconds per call] * REPEATS}, the routes alternating."""
    for fn in routes.values():
        timed(fn, n_sets, WARMUP)
    times = {name: [] for name in routes}
    for _ in range(REPEATS):
        for name, fn in routes.items():
            times[name].append(timed(fn, n_sets, calls))
    return times


lines = [f"dropout p = {P}: {REPEATS} repeats after {WARMUP} warm-up calls, routes alternating, tensors in rotation; device events",
         f"{'tensor':28s} {'route':8s} {'median us':>10s} {'spread us':>10s} {'bytes/elem':>10s} {'TB/s':>6s} {'of 6.29 TB/s':>12s}"]
for label, rows, dim, dtype, inplace, calls in (("bf16 [16384, 12288] in place", 16384, 12288, torch.bfloat16, True, 20),
                                                ("f32 [4768, 3072] out of place", 4768, 3072, torch.float32, False, 100)):
    esize = 2 if dtype == torch.bfloat16 else 4
    n_sets = CACHE // (rows * dim * esize * (1 if inplace else 2)) + 2
    xs = [torch.randn(rows, dim, generator=g, device=dev, dtype=torch.float32).to(dtype) for _ in range(n_sets)]
    outs = xs if inplace else [torch.empty_like(x) for x in xs]
    # the kept share is the binomial one before a time means anything (in place: checked on a copy)
    y = ops.dropout_apply(xs[0].clone(), P, 1234, 5)
    kept = float((y != 0).float().mean())
    n = rows * dim
    assert abs(kept - (1 - P)) < 6 * (P * (1 - P) / n) ** 0.5 + 1e-6, f"kept share {kept}"
    routes = {
        "hip": lambda i: ops.dropout_apply(xs[i], P, 1234 + i, 5, out=outs[i]),
        "torch": (lambda i: F.dropout(xs[i], P, True, True)) if inplace else (lambda i: F.dropout(xs[i], P, True, False)),
    }
    times = run(routes, n_sets, calls)
    for name, ts in times.items():
        med, bpe = statistics.median(ts), 2 * esize
        lines.append(f"{label:28s} {name:8s} {med * 1e6:10.1f} {(max(ts) - min(ts)) * 1e6:10.1f} {bpe:>10} {bpe * n / med / 1e12:6.2f} "
                     f"{bpe * n / med / STREAM_RATE:12.1%}")
    del xs, outs, y

# ---- the synthetic training step ---------------------------------------------------------------------------------------------------
from algonauts2025.model import FmriEncoderConfig  # noqa: E402
from algonauts2025.pl_module import BrainModule  # noqa: E402
from data_utils.dataloader import SegmentData  # noqa: E402
from modeling_utils.losses import TorchLossConfig  # noqa: E402
from modeling_utils.optim import HipAdam  # noqa: E402

B, T, L, D, V, S = 16, 1024, 2, 2048, 1000, 4
STEPS, ROUNDS = 3, 3
torch.manual_seed(0)
fdims = {"text": (L, D), "audio": (L, D), "video": (L, D)}
model = FmriEncoderConfig(n_subjects=S).build(fdims, V, T).to(dev).train()
bm = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {})
opt = HipAdam(model.parameters(), lr=1e-4)
gc = torch.Generator().manual_seed(1)
data = {m: torch.stack([torch.randn(l, d, T, generator=gc).bfloat16() for _ in range(B)]).to(dev) for m, (l, d) in fdims.items()}
data["subject_id"] = (torch.arange(B) % S).view(B, 1).to(dev)
data["fmri"] = torch.randn(B, V, T, generator=gc).to(dev)
batch = SegmentData(data=data, segments=[None] * B)


def set_ff_dropout(p):
    enc = model.encoder
    enc.ff_dropout = p
    for i in range(enc.depth):
        enc.layers[2 * i + 1][1].ff[1].p = p


def steps(p, n):
    set_ff_dropout(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        opt.zero_grad(set_to_none=True)
        loss = bm.training_step(batch, 0)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return (time.perf_counter() - t0) / n


for p in (0.0, P):
    steps(p, 2)
step_times = {0.0: [], P: []}
for _ in range(ROUNDS):
    for p in step_times:
        step_times[p].append(steps(p, STEPS))
lines.append(f"training step (forward + backward + HipAdam), synthetic B = {B} x T = {T}, hidden 3072, 8 layers; {STEPS} steps per timing, "
             f"{ROUNDS} rounds, settings alternating; wall clock")
lines.append(f"{'ff_dropout':>10s} {'median ms':>10s} {'spread ms':>10s}")
for p, ts in step_times.items():
    lines.append(f"{p:10.2f} {statistics.median(ts) * 1e3:10.1f} {(max(ts) - min(ts)) * 1e3:10.1f}")
extra = statistics.median(step_times[P]) - statistics.median(step_times[0.0])
lines.append(f"ff_dropout {P} adds {extra * 1e3:.1f} ms per step: 16 launches (8 layers, forward and backward) over the bf16 [{B * T}, 12288] hidden")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
