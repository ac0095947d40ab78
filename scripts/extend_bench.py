"""Appending a block of k positions to a filled KV cache (HipEncoder.extend) against the two routes there were before: k calls of
HipEncoder.step from the same cache state, and HipEncoder.forward on the whole window [0 .. pos + k).

GPU box:  python scripts/extend_bench.py [out.txt]      (default: profiles/extend_bench.txt)

Encoder: dim 3072, depth 8, 8 heads of dim_head 384, causal (the shape of scripts/stream_bench.py); B in {1, 16}; the cache holds pos in
{0, 255, 768} earlier positions; k in {1, 4, 16, 64, 256}.
1. One block: `extend` = the input copy + HipEncoder.extend_tokens (M = B * k rows per GEMM, tribe_kv_append_block +
   tribe_attention_extend_fwd per layer); `steps` = k times (the input copy + HipEncoder.step_tokens), positions pos .. pos + k - 1;
   `window` = the input copy + HipEncoder.forward_tokens on pos + k positions, of which only the last k rows are wanted.  Routes alternate
   within every round; min / median / max over the rounds; device events.  A route is called "ahead" of another only where its slowest
   round is faster than the other's fastest; where the ranges overlap it is "not ahead".
2. tribe_attention_extend_fwd alone, walking the 8 layers' caches in turn: it occupies B * heads * ceil(k / 128) workgroups, each walking
   its pos + k keys serially."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from modeling_utils.models.transformer import HipEncoder  # noqa: E402
from tribe_hip import ops  # noqa: E402

DIM, DEPTH, HEADS, DH, CAP = 3072, 8, 8, 384, 1024
BATCHES, POSITIONS, BLOCKS = (1, 16), (0, 255, 768), (1, 4, 16, 64, 256)
ROUNDS = 5
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "extend_bench.txt"
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
        timed(fn, min(calls, 2))
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, (fn, calls) in routes.items():
            times[name].append(timed(fn, calls))
    return times


def spread(ts, unit):
    return f"{min(ts) * unit:9.3f} {statistics.median(ts) * unit:9.3f} {max(ts) * unit:9.3f}"


def verdict(mine, other, name):
    """`mine` against `other` by their ranges over the rounds."""
    ratio = statistics.median(other) / statistics.median(mine)
    if max(mine) < min(other):
        return f"{name} / extend = {ratio:.2f}x"
    if min(mine) > max(other):
        return f"{name} / extend = {ratio:.2f}x  (extend is BEHIND {name})"
    return f"{name} / extend = {ratio:.2f}x  (ranges overlap: extend is NOT ahead of {name})"


torch.manual_seed(0)
enc = HipEncoder(dim=DIM, depth=DEPTH, heads=HEADS, dim_head=DH, causal=True).to(dev).eval()
lines = [f"block append on a streamed causal encoder: dim {DIM}, depth {DEPTH}, {HEADS} heads x {DH}, cache capacity {CAP}; {ROUNDS} rounds, "
         "routes alternating",
         "", "1. one block of k positions onto a cache that holds pos (ms per block; input copies included in every route; device events)",
         f"{'B':>3s} {'pos':>5s} {'k':>4s} {'route':8s} {'min':>9s} {'median':>9s} {'max':>9s}  notes"]
attn_lines = ["", "2. tribe_attention_extend_fwd alone, the 8 layers' caches in turn (us per call; device events)",
              f"{'B':>3s} {'pos':>5s} {'k':>4s} {'wgs':>5s} {'min':>9s} {'median':>9s} {'max':>9s}  per query row"]

with torch.no_grad():
    for B in BATCHES:
        cache = enc.new_cache(B, CAP)
        cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev))
        cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
        x0 = torch.randn(B * CAP, DIM, generator=g, device=dev)
        x = torch.empty_like(x0)
        for pos in POSITIONS:
            for k in BLOCKS:
                n = pos + k

                def extend():
                    x[: B * k].copy_(x0[: B * k])
                    cache.pos = pos
                    return enc.extend_tokens(x[: B * k], B, k, cache)

                def steps():
                    cache.pos = pos
                    for t in range(k):
                        x[:B].copy_(x0[t * B:(t + 1) * B])
                        y = enc.step_tokens(x[:B], cache)
                    return y

                def window():
                    x[: B * n].copy_(x0[: B * n])
                    return enc.forward_tokens(x[: B * n], B, n)

                for fn in (extend, steps, window):
                    assert bool(torch.isfinite(fn().float()).all())
                ts = run({"extend": (extend, 20 if B * k <= 256 else 5), "steps": (steps, max(1, 20 // k)),
                          "window": (window, 20 if B * n <= 1024 else 3)})
                lines.append(f"{B:3d} {pos:5d} {k:4d} {'extend':8s} {spread(ts['extend'], 1e3)}  "
                             f"{statistics.median(ts['extend']) / k * 1e3:.3f} ms per position")
                lines.append(f"{B:3d} {pos:5d} {k:4d} {'steps':8s} {spread(ts['steps'], 1e3)}  {verdict(ts['extend'], ts['steps'], 'steps')}")
                lines.append(f"{B:3d} {pos:5d} {k:4d} {'window':8s} {spread(ts['window'], 1e3)}  {verdict(ts['extend'], ts['window'], 'window')}")

                q = torch.randn(B * k, 3 * HEADS * DH, generator=g, device=dev).to(torch.bfloat16)
                layer = [0]

                def attend():
                    layer[0] = (layer[0] + 1) % DEPTH
                    return ops.attention_extend(q, cache.k[layer[0]], cache.v[layer[0]], pos, k, DH**-0.5)

                ta = run({"attend": (attend, 100)})["attend"]
                attn_lines.append(f"{B:3d} {pos:5d} {k:4d} {B * HEADS * ((k + 127) // 128):5d} {spread(ta, 1e6)}  "
                                  f"{statistics.median(ta) / (B * k) * 1e6:8.3f} us")
        del cache, x0, x
        torch.cuda.empty_cache()

text = "\n".join(lines + attn_lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
