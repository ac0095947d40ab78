"""Independent timelines in one KV cache (HipEncoder.step_slots on an EncoderSlots: a position per sequence) against the uniform route
(HipEncoder.step on an EncoderCache: one position for the whole batch).

GPU box:  python scripts/slots_bench.py [out.txt]      (default: profiles/slots_bench.txt)

Encoder: that of scripts/stream_bench.py -- dim 3072, depth 8, 8 heads of dim_head 384, causal, cache capacity 1024.
(a) One call at B = 16.  `step` = the input copy + HipEncoder.step_tokens at position pos (code this change does not touch: it stands for
    the parent commit); `step_slots` = the input copy + HipEncoder.step_slots_tokens, which also sends the 16 positions to the device.
    Positions all equal (255, 1023) against `step` there; positions spread evenly over 0 .. 1023 against `step` at 1023.  Routes alternate
    within every round; min / median / max over the rounds; device events.
(b) The use case: 16 timelines of the lengths 1000, 940, 880, ... (step -60, floor 100), 8800 steps in all.  `one by one` follows them one
    after another with `step` at B = 1; `8 slots` follows them through one 8-slot EncoderSlots that refills a slot as soon as its timeline
    ends (slots fall idle only when no timeline is left).  Wall clock around a device synchronise; timeline-steps per second."""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from modeling_utils.models.transformer import HipEncoder  # noqa: E402

DIM, DEPTH, HEADS, DH, CAP = 3072, 8, 8, 384, 1024
B, SLOTS, ROUNDS = 16, 8, 5
LENGTHS = [max(100, 1000 - 60 * i) for i in range(16)]
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "slots_bench.txt"
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


def verdict(slot_ts, step_ts):
    """Is the slot form slower than `step` by more than the rounds spread?"""
    s, u = statistics.median(slot_ts), statistics.median(step_ts)
    noise = max(max(slot_ts) - min(slot_ts), max(step_ts) - min(step_ts))
    if s - u > noise:
        return f"step_slots / step = {s / u:.3f}x: SLOWER by {(s - u) * 1e6:.1f} us, more than the spread of the rounds ({noise * 1e6:.1f} us)"
    return f"step_slots / step = {s / u:.3f}x: within the spread of the rounds ({noise * 1e6:.1f} us)" if s >= u else \
        f"step_slots / step = {s / u:.3f}x"


torch.manual_seed(0)
enc = HipEncoder(dim=DIM, depth=DEPTH, heads=HEADS, dim_head=DH, causal=True).to(dev).eval()
lines = [f"independent timelines in one cache: dim {DIM}, depth {DEPTH}, {HEADS} heads x {DH}, cache capacity {CAP}; {ROUNDS} rounds, routes "
         "alternating", "", f"(a) one call at B = {B} (ms; input copy included in both routes; device events)",
         f"{'positions':>16s} {'route':10s} {'min':>9s} {'median':>9s} {'max':>9s}  notes"]

with torch.no_grad():
    cache, slots = enc.new_cache(B, CAP), enc.new_slots(B, CAP)
    cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev))
    cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
    slots.k.copy_(cache.k)
    slots.v.copy_(cache.v)
    x0 = torch.randn(B, DIM, generator=g, device=dev)
    x = torch.empty_like(x0)
    every = [True] * B
    spread_pos = [round(i * (CAP - 1) / (B - 1)) for i in range(B)]
    for label, positions, pos in (("all 255", [255] * B, 255), ("all 1023", [1023] * B, 1023), ("0 .. 1023 evenly", spread_pos, 1023)):

        def step():
            x.copy_(x0)
            cache.pos = pos
            return enc.step_tokens(x, cache)

        def step_slots():
            x.copy_(x0)
            slots.positions = list(positions)
            return enc.step_slots_tokens(x, slots, every)

        a, b = step(), step_slots()
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
        same = ""
        if len(set(positions)) == 1:
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "equal positions: step_slots must give the bits of step"
            same = "; output bits equal to step's"
        ts = run({"step": (step, 50), "step_slots": (step_slots, 50)})
        lines.append(f"{label:>16s} {'step':10s} {spread(ts['step'], 1e3)}  at pos {pos}")
        lines.append(f"{label:>16s} {'step_slots':10s} {spread(ts['step_slots'], 1e3)}  {verdict(ts['step_slots'], ts['step'])}{same}")
    del cache, slots

    total = sum(LENGTHS)
    lines += ["", f"(b) {len(LENGTHS)} timelines of lengths {LENGTHS[0]}, {LENGTHS[1]}, {LENGTHS[2]}, ... , {LENGTHS[-1]} ({total} steps); wall clock around "
              "a device synchronise, 3 runs each, alternating",
              f"{'route':12s} {'min s':>9s} {'median s':>9s} {'max s':>9s}  timeline-steps per second (median)"]
    feed = torch.randn(64, SLOTS, DIM, generator=g, device=dev)                       # inputs, cycled
    one, many = enc.new_cache(1, CAP), enc.new_slots(SLOTS, CAP)
    x1, x8 = torch.empty(1, DIM, device=dev), torch.empty(SLOTS, DIM, device=dev)

    def one_by_one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in LENGTHS:
            one.reset()
            for t in range(n):
                x1.copy_(feed[t & 63, :1])
                enc.step_tokens(x1, one)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def through_slots():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        many.reset()
        queue = list(LENGTHS)
        left = [queue.pop(0) for _ in range(SLOTS)]                                    # steps left in the timeline each slot follows
        calls = 0
        while any(left):
            flags = [n > 0 for n in left]
            x8.copy_(feed[calls & 63])
            enc.step_slots_tokens(x8, many, flags)
            calls += 1
            for b in range(SLOTS):
                if left[b]:
                    left[b] -= 1
                    if left[b] == 0 and queue:                                        # the timeline ended: the slot takes the next one
                        many.reset([b])
                        left[b] = queue.pop(0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, calls

    one_by_one(), through_slots()
    t_one, t_many, n_calls = [], [], 0
    for _ in range(3):
        t_one.append(one_by_one())
        t, n_calls = through_slots()
        t_many.append(t)
    m1, m8 = statistics.median(t_one), statistics.median(t_many)
    lines.append(f"{'one by one':12s} {spread(t_one, 1.0)}  {total / m1:9.0f}   ({total} calls of `step` at B = 1, {m1 / total * 1e3:.3f} ms each)")
    lines.append(f"{f'{SLOTS} slots':12s} {spread(t_many, 1.0)}  {total / m8:9.0f}   ({n_calls} calls of `step_slots` at B = {SLOTS}, "
                 f"{m8 / n_calls * 1e3:.3f} ms each; {total / n_calls:.2f} of {SLOTS} slots busy on average); speed-up {m1 / m8:.2f}x")

text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
