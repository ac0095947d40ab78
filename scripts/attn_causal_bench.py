"""The causal softmax row kernels against the non-causal ones and a torch composition, the encoder forward causal against non-causal, and
the synthetic training step causal against non-causal.

GPU box:  python scripts/attn_causal_bench.py [out.txt]      (default: profiles/attn_causal_bench.txt)

1. Kernels, p = 0 and 0.1, the logical tensor [16 * 8 * 1024, 1024] of B = 16 x 8 heads x T = 1024:
     forward   causal: ops.softmax_causal_fwd; full: ops.softmax_dropout_fwd on the same scores;
               torch: F.dropout(torch.softmax(S.masked_fill(future, -inf), -1), p).to(bfloat16)
     backward  causal: ops.softmax_causal_bwd in place; full: ops.softmax_dropout_bwd in place;
               torch: g = dPd * m, dS = ((g - sum(g * P)) * P * scale).to(bfloat16), Pd = (P * m).to(bfloat16) from the f32 causal softmax P
               and the scaled f32 mask m torch's autograd would have saved
   Algorithmic bytes per row: causal forward 4 (i + 1) + 2 T, backward 6 (i + 1) + 4 T (a row reads its visible part and writes whole
   rows); full forward 6 T, backward 10 T.  Averaged over i the causal kernels move 0.67 / 0.70 of the full kernels' bytes.
2. Encoder forward: HipEncoder(dim 3072, depth 8, 8 heads of dim_head 384), B = 16, T = 1024, bf16 out, ONE module whose `causal` is switched
   (non-causal: the one-wave-per-SIMD kernel with fused q rotary; causal: q and k through the stand-alone rotary, the 16-row kernel under the
   mask, half the score FLOPs).
3. Training step: scripts/train_bench.py's synthetic model at B = 16, T = 1024, forward + backward + HipAdam, ONE model switched between
   non-causal p = 0 (flash forward, fused-softmax backward), non-causal attn_dropout = 0.1 and causal p = 0 (both the materialised route).
Routes alternate within every round; the file records min / median / max."""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tribe_hip import ops  # noqa: E402

STREAM_RATE, SCALE = 6.29e12, 384**-0.5
WARMUP, REPEATS, CALLS = 3, 5, 10
B, H, T = 16, 8, 1024
ROWS = B * H * T
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "attn_causal_bench.txt"
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


def run(routes, warmup=WARMUP, repeats=REPEATS, calls=CALLS):
    """{name: [seconds per call] * repeats}, the routes alternating."""
    for fn in routes.values():
        timed(fn, warmup)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(timed(fn, calls))
    return times


def row(label, ts, unit=1e6, extra=""):
    return f"{label:34s} {min(ts) * unit:9.1f} {statistics.median(ts) * unit:10.1f} {max(ts) * unit:9.1f} {extra}".rstrip()


# algorithmic bytes of the whole tensor: every query index occurs ROWS / T times
VISIBLE = ROWS // T * (T * (T + 1) // 2)
BYTES = {"fwd causal": 4 * VISIBLE + 2 * ROWS * T, "fwd full": 6 * ROWS * T, "bwd causal": 6 * VISIBLE + 4 * ROWS * T, "bwd full": 10 * ROWS * T}
lines = [f"causal softmax row kernels, logical tensor [{ROWS}, {T}]: {REPEATS} repeats of {CALLS} calls after {WARMUP} warm-up calls, routes "
         "alternating; device events",
         f"derived bytes causal / full: forward {BYTES['fwd causal'] / BYTES['fwd full']:.3f}, backward {BYTES['bwd causal'] / BYTES['bwd full']:.3f}",
         f"{'kernel, p, route':34s} {'min us':>9s} {'median us':>10s} {'max us':>9s} {'TB/s':>6s} {'of 6.29 TB/s':>12s}"]


def rate(kind, ts):
    med = statistics.median(ts)
    return f"{BYTES[kind] / med / 1e12:6.2f} {BYTES[kind] / med / STREAM_RATE:12.1%}"


S = torch.randn(ROWS, T, generator=g, device=dev) * 2.0
future = torch.ones(T, T, dtype=torch.bool, device=dev).triu(1)
Pd = torch.empty(ROWS, T, dtype=torch.bfloat16, device=dev)
lse = torch.empty(ROWS, dtype=torch.float32, device=dev)
# the result is the causal softmax before a time means anything
ops.softmax_causal_fwd(S, 0.0, 1234, 5, out=Pd, lse=lse)
assert abs(float(Pd[: 4 * T].float().sum(-1).mean()) - 1.0) < 1e-2 and not bool(Pd.view(-1, T, T)[:2][:, future].any())
dPd = torch.randn(ROWS, T, generator=g, device=dev)
dS = torch.empty(ROWS, T, dtype=torch.bfloat16, device=dev)
for p in (0.0, 0.1):
    fwd = run({"causal": lambda i: ops.softmax_causal_fwd(S, p, 1234 + i, 5, out=Pd, lse=lse),
               "full": lambda i: ops.softmax_dropout_fwd(S, p, 1234 + i, 5, out=Pd, lse=lse),
               "torch": lambda i: F.dropout(torch.softmax(S.view(-1, T, T).masked_fill(future, float("-inf")), -1), p, True, False).to(torch.bfloat16)})
    P32 = torch.softmax(S.view(-1, T, T).masked_fill(future, float("-inf")), -1).view(ROWS, T)
    m = F.dropout(torch.ones_like(P32), p, True, False)
    negD = -SCALE * (P32 * m * dPd).sum(-1)
    work_c, work_f = P32.to(torch.bfloat16), P32.to(torch.bfloat16)

    def torch_bwd(i):
        gr = dPd * m
        return ((gr - (gr * P32).sum(-1, keepdim=True)) * P32 * SCALE).to(torch.bfloat16), (P32 * m).to(torch.bfloat16)

    # (in place, as the training path runs them: after the first call the work buffers hold Pd -- traffic and arithmetic are the same)
    bwd = run({"causal": lambda i: ops.softmax_causal_bwd(work_c, dPd, negD, SCALE, p, 1234 + i, 5, dS=dS),
               "full": lambda i: ops.softmax_dropout_bwd(work_f, dPd, negD, SCALE, p, 1234 + i, 5, dS=dS),
               "torch": torch_bwd})
    del P32, m, negD, work_c, work_f
    for kernel, key, times in (("forward", "fwd", fwd), ("backward", "bwd", bwd)):
        for name, ts in times.items():
            lines.append(row(f"{kernel} p={p} {name}", ts, extra=rate(f"{key} {name}", ts) if name != "torch" else ""))
        c, f, t = (statistics.median(times[k]) for k in ("causal", "full", "torch"))
        lines.append(f"{kernel} p={p}: causal / full = {c / f:.3f} (derived bytes {BYTES[key + ' causal'] / BYTES[key + ' full']:.3f})"
                     + ("" if c < f else "  (the causal kernel is NOT ahead of the full one)")
                     + f"; torch composition / causal = {t / c:.2f}x" + ("" if t > c else "  (the causal kernel is NOT ahead of torch)"))
del S, Pd, lse, dPd, dS
torch.cuda.empty_cache()

# ---- the encoder forward -----------------------------------------------------------------------------------------------------------
from modeling_utils.models.transformer import HipEncoder  # noqa: E402

torch.manual_seed(0)
enc = HipEncoder(dim=3072, depth=8, heads=8, dim_head=384).to(dev).eval()
x0 = torch.randn(B * T, 3072, generator=g, device=dev)
x = torch.empty_like(x0)


def encode(causal):
    def fn(i):
        enc.causal = causal
        x.copy_(x0)   # forward_tokens consumes its input
        return enc.forward_tokens(x, B, T)
    return fn


with torch.no_grad():
    ya, yb = encode(False)(0).float(), encode(True)(0).float()
    assert bool(torch.isfinite(ya).all()) and bool(torch.isfinite(yb).all()) and not torch.equal(ya, yb)
    del ya, yb
    et = run({"non-causal": encode(False), "causal": encode(True)}, warmup=2, repeats=5, calls=3)
lines += ["", f"encoder forward, dim 3072, 8 layers, 8 heads x 384, B = {B}, T = {T} (input copy included): 5 repeats of 3 calls, routes alternating; "
          "device events", f"{'route':34s} {'min ms':>9s} {'median ms':>10s} {'max ms':>9s}"]
for name, ts in et.items():
    lines.append(row(name, ts, unit=1e3))
c, f = statistics.median(et["causal"]), statistics.median(et["non-causal"])
lines.append(f"encoder forward: causal / non-causal = {c / f:.3f}" + ("" if c < f else "  (the causal forward is NOT ahead)"))
del enc, x, x0
torch.cuda.empty_cache()

# ---- the synthetic training step ---------------------------------------------------------------------------------------------------
from algonauts2025.model import FmriEncoderConfig  # noqa: E402
from algonauts2025.pl_module import BrainModule  # noqa: E402
from data_utils.dataloader import SegmentData  # noqa: E402
from modeling_utils.losses import TorchLossConfig  # noqa: E402
from modeling_utils.optim import HipAdam  # noqa: E402

L, D, V, NS = 2, 2048, 1000, 4
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
SETTINGS = {"non-causal p=0": (False, 0.0), "non-causal attn_dropout=0.1": (False, 0.1), "causal p=0": (True, 0.0)}


def steps(setting, count):
    model.encoder.causal, model.encoder.attn_dropout = SETTINGS[setting]
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


for s in SETTINGS:
    steps(s, 2)
step_times = {s: [] for s in SETTINGS}
for _ in range(ROUNDS):
    for s in SETTINGS:
        step_times[s].append(steps(s, STEPS))
lines += ["", f"training step (forward + backward + HipAdam), synthetic B = {B} x T = {T}, hidden 3072, 8 layers; {STEPS} steps per timing, "
          f"{ROUNDS} rounds, settings alternating; wall clock", f"{'setting':34s} {'min ms':>9s} {'median ms':>10s} {'max ms':>9s}"]
for s, ts in step_times.items():
    lines.append(row(s, ts, unit=1e3))
med = {s: statistics.median(ts) for s, ts in step_times.items()}
lines.append(f"causal p=0 against non-causal p=0: {(med['causal p=0'] - med['non-causal p=0']) * 1e3:+.1f} ms per step "
             f"({med['causal p=0'] / med['non-causal p=0'] - 1:+.1%}); against non-causal attn_dropout=0.1 (the same route): "
             f"{(med['causal p=0'] - med['non-causal attn_dropout=0.1']) * 1e3:+.1f} ms ({med['causal p=0'] / med['non-causal attn_dropout=0.1'] - 1:+.1%})")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
