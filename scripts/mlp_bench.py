"""Hidden block of an MLP (LayerNorm + GELU) as the HIP row kernels against stock torch, and one MLP on both routes of `Mlp.forward`.

GPU box:  python scripts/mlp_bench.py [out.txt]      (default: profiles/mlp_bench.txt)

Kernel part, rows = 16 * 298 = 4768 at dim 1024 and 3072: every call works on the next of N input sets whose footprint together
exceeds the 256 MiB Infinity Cache, so a call does not re-read what the call before it left on the die.  Routes alternate; per route the
HIP-event time of CALLS calls after a warm-up, REPEATS times; the file records the median, the spread (max - min of the repeats) and the
algorithmic bytes over the median as a share of the 6.29 TB/s streaming rate the README uses.
  hip fwd        tribe_norm_act_fwd, z f32 -> bf16 operand + mean, rstd                      (4 + 2 bytes per element)
  hip bwd        tribe_norm_act_bwd, dy bf16 + saved z -> dz f32, dgamma, dbeta                (2 + 4 + 4 bytes per element; the column-sum
                 launch reads dy and z a second time, which the share does NOT count as useful bytes)
  torch fwd      nn.GELU()(nn.LayerNorm(dim)(z)), f32 in and out, no grad                      (4 + 4)
  torch fwd+bwd  the same with autograd and y.backward(dy)
MLP part: MlpConfig(hidden_sizes=[1024], norm_layer="layer", activation_layer="gelu").build(6144, 1024) on 4768 rows, forward (no
grad) and forward + backward, on the HIP route and on the stock route (nn.Sequential.forward of the same module: f32 GEMMs).
"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

from modeling_utils.models.common import MlpConfig  # noqa: E402
from tribe_hip import ops  # noqa: E402

ROWS, STREAM_RATE, CACHE = 16 * 298, 6.29e12, 256 << 20
WARMUP, CALLS, REPEATS = 10, 100, 5
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mlp_bench.txt"
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


lines = [f"LayerNorm + GELU between two Linear layers, rows = {ROWS}; {CALLS} calls per timing after {WARMUP} warm-up calls, {REPEATS} repeats, "
         "routes alternating, inputs in rotation; device events",
         f"{'dim':>5s} {'route':14s} {'median us':>10s} {'spread us':>10s} {'bytes/elem':>10s} {'TB/s':>6s} {'of 6.29 TB/s':>12s}"]
for dim in (1024, 3072):
    n_sets = CACHE // (ROWS * dim * 6) + 2                                   # the forward's 6 bytes per element is the smallest footprint
    zs = [torch.randn(ROWS, dim, generator=g, device=dev) for _ in range(n_sets)]
    dys = [torch.randn(ROWS, dim, generator=g, device=dev).bfloat16() for _ in range(n_sets)]
    dy32 = [d.float() for d in dys]
    ys = [torch.empty(ROWS, dim, dtype=torch.bfloat16, device=dev) for _ in range(n_sets)]
    dzs = [torch.empty(ROWS, dim, device=dev) for _ in range(n_sets)]
    ln, act = nn.LayerNorm(dim).to(dev), nn.GELU()
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.3, generator=g)
        ln.bias.normal_(0.0, 0.3, generator=g)
    gamma, beta = ln.weight.detach(), ln.bias.detach()
    stats = [ops.norm_act(z, gamma, beta, ln.eps, "gelu", want_stats=True)[1:] for z in zs]
    zs_grad = [z.clone().requires_grad_() for z in zs]

    def torch_fwd(i):
        with torch.no_grad():
            act(ln(zs[i]))

    def torch_fwd_bwd(i):
        zs_grad[i].grad = None
        act(ln(zs_grad[i])).backward(dy32[i])

    routes = {
        "hip fwd": lambda i: ops.norm_act(zs[i], gamma, beta, ln.eps, "gelu", want_stats=True, out=ys[i]),
        "hip bwd": lambda i: ops.norm_act_bwd(dys[i], zs[i], stats[i][0], stats[i][1], gamma, beta, "gelu", out=dzs[i]),
        "torch fwd": torch_fwd,
        "torch fwd+bwd": torch_fwd_bwd,
    }
    # both routes must agree before a time means anything
    y, _, _ = routes["hip fwd"](0)
    want = act(ln(zs[0])).detach()
    rel = float((y.float() - want).norm() / want.norm())
    assert rel < 4e-3, f"HIP forward differs from torch by {rel:.2e} (bf16 output: 2e-3 expected)"
    torch_fwd_bwd(0)
    dz, dgamma, dbeta = routes["hip bwd"](0)
    for name, got, ref in (("dz", dz, zs_grad[0].grad), ("dgamma", dgamma, ln.weight.grad), ("dbeta", dbeta, ln.bias.grad)):
        rel = float((got - ref).norm() / ref.norm())
        assert rel < 1e-4, f"HIP backward {name} differs from torch autograd by {rel:.2e}"
    ln.zero_grad()
    bytes_per = {"hip fwd": 6, "hip bwd": 10, "torch fwd": 8, "torch fwd+bwd": None}
    times = run(routes, n_sets, CALLS)
    for name, ts in times.items():
        med, bpe = statistics.median(ts), bytes_per[name]
        rate = "" if bpe is None else f"{bpe * ROWS * dim / med / 1e12:6.2f} {bpe * ROWS * dim / med / STREAM_RATE:12.1%}"
        lines.append(f"{dim:5d} {name:14s} {med * 1e6:10.1f} {(max(ts) - min(ts)) * 1e6:10.1f} {'' if bpe is None else bpe:>10} {rate}")
    hip = statistics.median(times["hip fwd"]) + statistics.median(times["hip bwd"])
    lines.append(f"{dim:5d} hip fwd + hip bwd {hip * 1e6:.1f} us against torch fwd+bwd {statistics.median(times['torch fwd+bwd']) * 1e6:.1f} us")
    del zs, dys, dy32, ys, dzs, zs_grad, stats

# ---- one MLP on both routes --------------------------------------------------------------------------------------------------------
SIZES, MLP_CALLS = [6144, 1024, 1024], 20
mlp = MlpConfig(hidden_sizes=SIZES[1:-1], norm_layer="layer", activation_layer="gelu").build(SIZES[0], SIZES[-1]).to(dev)
n_sets = CACHE // (ROWS * SIZES[0] * 4) + 2
xs = [torch.randn(ROWS, SIZES[0], generator=g, device=dev) for _ in range(n_sets)]
cot = torch.randn(ROWS, SIZES[-1], generator=g, device=dev)


def forward(route, i):
    with torch.no_grad():
        return mlp(xs[i]) if route == "hip" else nn.Sequential.forward(mlp, xs[i])


def forward_backward(route, i):
    mlp.zero_grad(set_to_none=True)
    (mlp(xs[i]) if route == "hip" else nn.Sequential.forward(mlp, xs[i])).backward(cot)


rel = float((forward("hip", 0) - forward("stock", 0)).norm() / forward("stock", 0).norm())
assert rel < 2e-2, f"the two routes differ by {rel:.2e}"
forward_backward("stock", 0)
stock_grads = {n: p.grad.clone() for n, p in mlp.named_parameters()}
forward_backward("hip", 0)
worst = max(float((p.grad - stock_grads[n]).norm() / stock_grads[n].norm()) for n, p in mlp.named_parameters())
assert worst < 3e-2, f"gradients of the two routes differ by {worst:.2e}"
routes = {"hip fwd": lambda i: forward("hip", i), "stock fwd": lambda i: forward("stock", i),
          "hip fwd+bwd": lambda i: forward_backward("hip", i), "stock fwd+bwd": lambda i: forward_backward("stock", i)}
times = run(routes, n_sets, MLP_CALLS)
lines.append(f"MLP {SIZES} (Linear, LayerNorm, GELU, Linear), rows = {ROWS}, f32 input; {MLP_CALLS} calls per timing, {REPEATS} repeats; the HIP "
             f"route differs from the stock (f32 GEMM) route by {rel:.1e} forward, {worst:.1e} in the worst gradient (relative L2)")
lines.append(f"{'route':14s} {'median us':>10s} {'spread us':>10s}")
for name, ts in times.items():
    lines.append(f"{name:14s} {statistics.median(ts) * 1e6:10.1f} {(max(ts) - min(ts)) * 1e6:10.1f}")
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
