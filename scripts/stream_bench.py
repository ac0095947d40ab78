"""Streaming a causal encoder step by step (HipEncoder.step on a KV cache) against the only route there was before: HipEncoder.forward on
the whole window [0 .. pos] for every new position.

GPU box:  python scripts/stream_bench.py [out.txt]      (default: profiles/stream_bench.txt)

Encoder: dim 3072, depth 8, 8 heads of dim_head 384, causal; B in {1, 4, 16}.
1. One step at pos in {0, 255, 1023} (the cache holds pos earlier positions): `step` = the input copy + HipEncoder.step_tokens (M = B rows
   per GEMM, tribe_kv_append + tribe_attention_decode_fwd per layer); `window` = the input copy + HipEncoder.forward_tokens on pos + 1
   positions, of which only the last row is wanted.  Routes alternate within every round; min / median / max over the rounds; device events.
   A step streams every encoder weight once: 8 x 113.25 M parameters x 2 bytes = 1.81 GB, 0.29 ms at the 6.29 TB/s streaming rate -- the
   floor each step is reported against.
2. The decode attention alone at n = pos + 1 keys, walking the 8 layers' caches in turn: 2 * n * dim_head * 2 bytes per (sequence, head),
   against the same streaming rate.  (The caches of a small B stay in the 256 MiB Infinity Cache between calls; the figure is what the call
   achieves, not an HBM measurement.)
3. A whole 1024-step timeline: 1024 steps from an empty cache against 1024 growing window forwards (T = 1 .. 1024); wall clock around a
   device synchronise."""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from modeling_utils.models.transformer import HipEncoder  # noqa: E402
from tribe_hip import ops  # noqa: E402

STREAM_RATE = 6.29e12
DIM, DEPTH, HEADS, DH, CAP = 3072, 8, 8, 384, 1024
WEIGHT_BYTES = DEPTH * (4 * DIM * DIM + 2 * 4 * DIM * DIM) * 2          # q, k, v, out + the two feed-forward matrices, bf16
FLOOR = WEIGHT_BYTES / STREAM_RATE
BATCHES, POSITIONS = (1, 4, 16), (0, 255, 1023)
ROUNDS = 5
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "stream_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e-3


def run(routes, rounds=ROUNDS):
    """{name: [seconds per call] * rounds}; routes = {name: (fn, calls per timing)}, alternating within a round, each warmed up first."""
    for fn, calls in routes.values():
        timed(fn, min(calls, 3))
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, (fn, calls) in routes.items():
            times[name].append(timed(fn, calls))
    return times


def spread(ts, unit):
    return f"{min(ts) * unit:9.3f} {statistics.median(ts) * unit:9.3f} {max(ts) * unit:9.3f}"


torch.manual_seed(0)
enc = HipEncoder(dim=DIM, depth=DEPTH, heads=HEADS, dim_head=DH, causal=True).to(dev).eval()
assert sum(p.numel() for n, p in enc.named_parameters() if n.endswith("weight")) * 2 == WEIGHT_BYTES
lines = [f"streamed causal encoder: dim {DIM}, depth {DEPTH}, {HEADS} heads x {DH}, cache capacity {CAP}; {ROUNDS} rounds, routes alternating; "
         f"weight-streaming floor of a step {WEIGHT_BYTES / 1e9:.2f} GB / {STREAM_RATE / 1e12:.2f} TB/s = {FLOOR * 1e3:.3f} ms",
         "", "1. one step at position pos (ms; input copy included in both routes; device events)",
         f"{'B':>3s} {'pos':>5s} {'route':8s} {'min':>9s} {'median':>9s} {'max':>9s}  notes"]
decode_lines = ["", "2. tribe_attention_decode_fwd alone, n = pos + 1 keys, the 8 layers' caches in turn (us per call; device events)",
                f"{'B':>3s} {'n':>5s} {'splits':>6s} {'min':>9s} {'median':>9s} {'max':>9s}  cache bytes per call, rate, share of 6.29 TB/s"]
timeline_lines = ["", "3. a 1024-step timeline from an empty cache (s; wall clock around a device synchronise; 3 runs of `step`, 1 of `window`)",
                  f"{'B':>3s} {'route':8s} {'min':>9s} {'median':>9s} {'max':>9s}  notes"]

with torch.no_grad():
    for B in BATCHES:
        cache = enc.new_cache(B, CAP)
        cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev))
        cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
        x0 = torch.randn(B * CAP, DIM, generator=g, device=dev)
        x = torch.empty_like(x0)
        q = torch.randn(B, 3 * HEADS * DH, generator=g, device=dev).to(torch.bfloat16)
        for pos in POSITIONS:
            n = pos + 1

            def step():
                x[:B].copy_(x0[:B])
                cache.pos = pos
                return enc.step_tokens(x[:B], cache)

            def window():
                x[: B * n].copy_(x0[: B * n])
                return enc.forward_tokens(x[: B * n], B, n)

            assert bool(torch.isfinite(step().float()).all()) and bool(torch.isfinite(window().float()).all())
            ts = run({"step": (step, 50), "window": (window, 50 if B * n <= 1024 else 5)})
            s, w = statistics.median(ts["step"]), statistics.median(ts["window"])
            lines.append(f"{B:3d} {pos:5d} {'step':8s} {spread(ts['step'], 1e3)}  floor / step = {FLOOR / s:.1%}")
            lines.append(f"{B:3d} {pos:5d} {'window':8s} {spread(ts['window'], 1e3)}  window / step = {w / s:.2f}x"
                         + ("" if w > s else "  (streaming is NOT ahead here)"))
            layer = [0]

            def decode():
                layer[0] = (layer[0] + 1) % DEPTH
                return ops.attention_decode(q, cache.k[layer[0]], cache.v[layer[0]], n, DH**-0.5)

            td = run({"decode": (decode, 200)})["decode"]
            nbytes = B * HEADS * 2 * n * DH * 2
            med = statistics.median(td)
            decode_lines.append(f"{B:3d} {n:5d} {ops.attention_decode_splits(B, HEADS, n):6d} {spread(td, 1e6)}  {nbytes / 1e6:8.3f} MB, "
                                f"{nbytes / med / 1e12:6.3f} TB/s, {nbytes / med / STREAM_RATE:6.1%}")

        def follow_stream():
            cache.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(CAP):
                x[:B].copy_(x0.view(B, CAP, DIM)[:, t])
                enc.step_tokens(x[:B], cache)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def follow_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(CAP):
                x[: B * (t + 1)].copy_(x0[: B * (t + 1)])
                enc.forward_tokens(x[: B * (t + 1)], B, t + 1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        fs = [follow_stream() for _ in range(3)]
        fw = [follow_window()]
        s, w = statistics.median(fs), fw[0]
        timeline_lines.append(f"{B:3d} {'step':8s} {spread(fs, 1.0)}  {s / CAP * 1e3:.3f} ms per step")
        timeline_lines.append(f"{B:3d} {'window':8s} {spread(fw, 1.0)}  window / step = {w / s:.1f}x" + ("" if w > s else "  (streaming is NOT ahead here)"))
        del cache, x0, x
        torch.cuda.empty_cache()

text = "\n".join(lines + decode_lines + timeline_lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
