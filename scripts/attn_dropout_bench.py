"""The softmax-dropout row kernels against a torch composition on the same tensors, and the synthetic training step with and without
attn_dropout.

GPU box:  python scripts/attn_dropout_bench.py [out.txt]      (default: profiles/attn_dropout_bench.txt)

Kernel part, p = 0.1, the logical tensor [16 * 8 * 1024, 1024] of B = 16 x 8 heads x T = 1024 (f32 scores: 512 MiB, twice the Infinity
Cache by themselves):
  forward   hip: ops.softmax_dropout_fwd (f32 S -> bf16 Pd + lse2; 4 + 2 bytes per score)
            torch: F.dropout(torch.softmax(S, -1), p).to(bfloat16) -- softmax, dropout (which also writes its mask) and the cast
  backward  hip: ops.softmax_dropout_bwd in place (bf16 P, f32 dPd -> bf16 dS, bf16 Pd; 2 + 4 + 2 + 2 bytes per score; the mask is drawn again)
            torch: the matching backward from what torch's autograd would have saved -- the f32 softmax P and the scaled f32 mask m:
            g = dPd * m, dS = ((g - sum(g * P)) * P * scale).to(bfloat16), Pd = (P * m).to(bfloat16)
Routes alternate; per route the HIP-event time of CALLS calls after a warm-up, REPEATS times; the file records min / median / max and the
algorithmic bytes of the HIP route over the median as a share of the 6.29 TB/s streaming rate the README uses.
Step part: scripts/train_bench.py's synthetic model (three 2 x 2048 modalities, 1000 parcels, 8 layers, hidden 3072) at B = 16, T = 1024,
forward + backward + HipAdam, ONE model whose attn_dropout is switched between 0 (exactly the launches of a model built without it: the
flash forward, the fused-softmax backward) and 0.1 (materialised f32 scores both ways); wall-clock time per step over STEPS steps, the two
settings alternating, ROUNDS rounds."""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tribe_hip import ops  # noqa: E402

STREAM_RATE, P, SCALE = 6.29e12, 0.1, 384**-0.5
WARMUP, REPEATS, CALLS = 3, 5, 10
ROWS, T = 16 * 8 * 1024, 1024
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "attn_dropout_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e-3


def run(routes):
    """{name: [seconds per call] * REPEATS}, the routes alternating."""
    for fn in routes.values():
        timed(fn, WARMUP)
    times = {name: [] for name in routes}
    for _ in range(REPEATS):
        for name, fn in routes.items():
            times[name].append(timed(fn, CALLS))
    return times


S = torch.randn(ROWS, T, generator=g, device=dev) * 2.0
Pd = torch.empty(ROWS, T, dtype=torch.bfloat16, device=dev)
lse = torch.empty(ROWS, dtype=torch.float32, device=dev)
# the kept share is the binomial one and the kept values are the softmax's before a time means anything
ops.softmax_dropout_fwd(S, P, 1234, 5, out=Pd, lse=lse)
kept = float((Pd != 0).float().mean())
n = ROWS * T
assert abs(kept - (1 - P)) < 6 * (P * (1 - P) / n) ** 0.5 + 1e-6, f"kept share {kept}"
assert abs(float(Pd[:4096].float().sum(-1).mean()) - 1.0) < 1e-2
lines = [f"attention dropout p = {P}, logical tensor [{ROWS}, {T}]: {REPEATS} repeats of {CALLS} calls after {WARMUP} warm-up calls, routes "
         "alternating; device events",
         f"{'kernel':9s} {'route':6s} {'min us':>9s} {'median us':>10s} {'max us':>9s} {'bytes/elem':>10s} {'TB/s':>6s} {'of 6.29 TB/s':>12s}"]
fwd = run({"hip": lambda i: ops.softmax_dropout_fwd(S, P, 1234 + i, 5, out=Pd, lse=lse),
           "torch": lambda i: F.dropout(torch.softmax(S, -1), P, True, False).to(torch.bfloat16)})
P32 = torch.softmax(S, -1)
del S
Pb = P32.to(torch.bfloat16)
m = F.dropout(torch.ones_like(P32), P, True, False)
dPd = torch.randn(ROWS, T, generator=g, device=dev)
negD = -SCALE * (P32 * m * dPd).sum(-1)
dS = torch.empty(ROWS, T, dtype=torch.bfloat16, device=dev)
work = Pb.clone()


def hip_bwd(i):
    # (in place, as the training path runs it: after the first call `work` holds Pd -- the traffic and the arithmetic are the same)
    ops.softmax_dropout_bwd(work, dPd, negD, SCALE, P, 1234 + i, 5, dS=dS)


def torch_bwd(i):
    gr = dPd * m
    return ((gr - (gr * P32).sum(-1, keepdim=True)) * P32 * SCALE).to(torch.bfloat16), (P32 * m).to(torch.bfloat16)


bwd = run({"hip": hip_bwd, "torch": torch_bwd})
for kernel, times, bpe in (("forward", fwd, 6), ("backward", bwd, 10)):
    for name, ts in times.items():
        med = statistics.median(ts)
        rate = f"{bpe:>10} {bpe * n / med / 1e12:6.2f} {bpe * n / med / STREAM_RATE:12.1%}" if name == "hip" else f"{'':>10s} {'':>6s} {'':>12s}"
        lines.append(f"{kernel:9s} {name:6s} {min(ts) * 1e6:9.1f} {med * 1e6:10.1f} {max(ts) * 1e6:9.1f} {rate}".rstrip())
    ratio = statistics.median(times["torch"]) / statistics.median(times["hip"])
    lines.append(f"{kernel}: torch composition / hip kernel = {ratio:.2f}x" + ("" if ratio > 1 else "  (the hip kernel is NOT ahead)"))
del P32, Pb, m, dPd, negD, dS, work, Pd, lse
torch.cuda.empty_cache()

# ---- the synthetic training step ---------------------------------------------------------------------------------------------------
from algonauts2025.model import FmriEncoderConfig  # noqa: E402
from algonauts2025.pl_module import BrainModule  # noqa: E402
from data_utils.dataloader import SegmentData  # noqa: E402
from modeling_utils.losses import TorchLossConfig  # noqa: E402
from modeling_utils.optim import HipAdam  # noqa: E402

B, L, D, V, NS = 16, 2, 2048, 1000, 4
STEPS, ROUNDS = 3, 3
torch.manual_seed(0)
fdims = {"text": (L, D), "audio": (L, D), "video": (L, D)}
model = FmriEncoderConfig(n_subjects=NS).build(fdims, V, T).to(dev).train()
bm = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {})
opt = HipAdam(model.parameters(), lr=1e-4)
gc = torch.Generator().manual_seed(1)
data = {mod: torch.stack([torch.randn(l, d, T, generator=gc).bfloat16() for _ in range(B)]).to(dev) for mod, (l, d) in fdims.items()}
data["subject_id"] = (torch.arange(B) % NS).view(B, 1).to(dev)
data["fmri"] = torch.randn(B, V, T, generator=gc).to(dev)
batch = SegmentData(data=data, segments=[None] * B)


def steps(p, count):
    model.encoder.attn_dropout = p
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        opt.zero_grad(set_to_none=True)
        loss = bm.training_step(batch, 0)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return (time.perf_counter() - t0) / count


for p in (0.0, P):
    steps(p, 2)
step_times = {0.0: [], P: []}
for _ in range(ROUNDS):
    for p in step_times:
        step_times[p].append(steps(p, STEPS))
lines.append(f"training step (forward + backward + HipAdam), synthetic B = {B} x T = {T}, hidden 3072, 8 layers; {STEPS} steps per timing, "
             f"{ROUNDS} rounds, settings alternating; wall clock")
lines.append(f"{'attn_dropout':>12s} {'min ms':>9s} {'median ms':>10s} {'max ms':>9s}")
for p, ts in step_times.items():
    lines.append(f"{p:12.2f} {min(ts) * 1e3:9.1f} {statistics.median(ts) * 1e3:10.1f} {max(ts) * 1e3:9.1f}")
extra = statistics.median(step_times[P]) - statistics.median(step_times[0.0])
lines.append(f"attn_dropout {P} adds {extra * 1e3:.1f} ms per step ({extra / statistics.median(step_times[0.0]):+.1%}): per layer it replaces the "
             "flash forward by f32 scores + the softmax-dropout kernel + Pd V, and the backward's fused dS epilogue by f32 dO V^T + the row kernel"
             + ("" if extra > 0 else "  (not slower in this run)"))
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
