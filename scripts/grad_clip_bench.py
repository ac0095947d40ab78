"""Gradient clipping in front of the optimiser step, on the full-size parameter list (the 0.94 G-parameter reference-defaults model
that scripts/train_bench.py builds).

GPU box:  python scripts/grad_clip_bench.py [out.txt]      (default: profiles/grad_clip_bench.txt)

Every parameter gets an N(0, 1e-4) gradient; no forward or backward runs.  Variants (each call between two device events, REPEATS
rounds after WARMUP rounds, the variants alternating inside every round so that drift shows as spread and not as a difference):

  norm                      ops.grad_norm: tribe_grad_norm's two launches (reads 4 B per parameter)
  scale in place            ops.grad_scale_ with a coefficient below 1 (reads 4 B and writes 4 B per parameter)
  adam                      HipAdam.step(): tribe_adam_step (16 B read + 12 B written per parameter)
  norm + fused adam         ops.grad_norm, then HipAdam.step(grad_scale=coef): tribe_adam_step_clipped, no extra bytes
  norm + scale + adam       ops.grad_norm, ops.grad_scale_, HipAdam.step()
  torch clip + adam         torch.nn.utils.clip_grad_norm_ (foreach), HipAdam.step()

The variants that rewrite the gradients get them restored from a pristine copy before each call, outside the events.  A time is what
the device events bracket: kernels plus whatever gaps the host leaves between their launches (the table upload of every call is in).
"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402

from algonauts2025.model import FmriEncoderConfig  # noqa: E402
from modeling_utils.optim import HipAdam  # noqa: E402
from tribe_hip import ops  # noqa: E402

WARMUP, REPEATS, HBM_STREAM = 2, 20, 6.29e12     # 6.29 TB/s: the measured float4-copy rate of the MI355X (8 TB/s is the spec sheet's)
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "grad_clip_bench.txt"
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)
fdims = {"text": (2, 3072), "audio": (2, 1024), "video": (2, 1408)}
model = FmriEncoderConfig(n_subjects=4, modality_dropout=0.3, contrastive_enabled=True, contrastive_modalities=["video"], contrastive_weight=0.1,
                          contrastive_temperature=0.07).build(fdims, 1000, 100).to(dev).train()
params = [p for p in model.parameters() if p.requires_grad]
P = sum(p.numel() for p in params)
gen = torch.Generator(device=dev).manual_seed(1)
pristine = [torch.randn(p.shape, generator=gen, device=dev) * 1e-2 for p in params]
for p, g in zip(params, pristine):
    p.grad = g.clone()
grads = [p.grad for p in params]
opt = HipAdam(params, lr=1e-4)
norm0 = float(ops.grad_norm(grads, 1.0)[0])
max_norm = 0.5 * norm0                                            # every clipped variant really scales (coefficient ~0.5)
half = torch.tensor(0.5, device=dev)


def restore():
    torch._foreach_copy_(grads, pristine)


def v_norm():
    ops.grad_norm(grads, max_norm)


def v_scale():
    ops.grad_scale_(grads, half)


def v_adam():
    opt.step()


def v_fused():
    opt.step(grad_scale=ops.grad_norm(grads, max_norm)[1])


def v_scale_adam():
    ops.grad_scale_(grads, ops.grad_norm(grads, max_norm)[1])
    opt.step()


def v_torch_adam():
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()


# name -> (call, rewrites the gradients, bytes per parameter)
variants = {
    "norm": (v_norm, False, 4),
    "scale in place": (v_scale, True, 8),
    "adam": (v_adam, False, 28),
    "norm + fused adam": (v_fused, False, 4 + 28),
    "norm + scale + adam": (v_scale_adam, True, 4 + 8 + 28),
    "torch clip + adam": (v_torch_adam, True, None),
}
times = {name: [] for name in variants}
for r in range(WARMUP + REPEATS):
    for name, (fn, rewrites, _) in variants.items():
        if rewrites:
            restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= WARMUP:
            times[name].append(a.elapsed_time(b))

# what the timed calls compute must agree before a time means anything: the fused step against scale-then-step, bit for bit
restore()
state = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params[:8]]
v_fused()
fused = [p.detach().clone() for p in params[:8]]
with torch.no_grad():
    for p, (w, m, v) in zip(params[:8], state):
        p.copy_(w), opt.state[p]["exp_avg"].copy_(m), opt.state[p]["exp_avg_sq"].copy_(v)
        opt.state[p]["step"] -= 1
    for p in params[8:]:
        opt.state[p]["step"] -= 1
grads_before = [g.clone() for g in grads[:8]]
v_scale_adam()
same = all(torch.equal(a, p.detach()) for a, p in zip(fused, params[:8]))
rewritten = not any(torch.equal(a, b) for a, b in zip(grads_before, grads[:8]))

med = {name: statistics.median(ts) for name, ts in times.items()}
floor_ms = 4 * P / HBM_STREAM * 1e3
lines = [f"gradient clipping on the full-size parameter list: {len(params)} tensors, {P / 1e9:.3f} G parameters, {4 * P / 1e9:.2f} GB of f32 gradients; "
         f"total norm {norm0:.4f}, max_norm {max_norm:.4f} (coefficient 0.5)",
         f"{REPEATS} timed rounds after {WARMUP} warm-up rounds, variants alternating inside every round; device events around each call",
         f"{'variant':22s} {'median ms':>10s} {'min ms':>8s} {'max ms':>8s} {'B/param':>8s} {'TB/s':>6s}"]
for name, ts in times.items():
    nb = variants[name][2]
    rate = f"{nb * P / (med[name] * 1e-3) / 1e12:6.2f}" if nb else "     -"
    lines.append(f"{name:22s} {med[name]:10.3f} {min(ts):8.3f} {max(ts):8.3f} {str(nb) if nb else '-':>8s} {rate}")
lines += [
    f"bytes from the shapes: the norm reads 4 B per parameter = {4 * P / 1e9:.2f} GB; the in-place scale adds 8 B per parameter = {8 * P / 1e9:.2f} GB; "
    "the fused step adds none",
    f"floor of the norm at the measured 6.29 TB/s streaming rate: {floor_ms:.3f} ms; measured {med['norm']:.3f} ms, i.e. {floor_ms / med['norm']:.0%} of that rate",
    ("the norm is bound by HBM bandwidth (one f32 -> f64 convert and one f64 FMA per 4 bytes read stay under the loads)"
     if med["norm"] <= 1.25 * floor_ms else
     "the norm is NOT at the HBM bound: its time is more than 1.25x the streaming floor, so the per-element f64 convert + FMA issue or "
     "the launch pair's fixed cost bounds it, not the memory system"),
    f"fused clipped step over plain step: {med['norm + fused adam'] - med['norm'] - med['adam']:+.3f} ms beyond norm + adam",
    f"fused against scale-then-step: {med['norm + scale + adam'] - med['norm + fused adam']:+.3f} ms saved "
    f"(spreads: {max(times['norm + fused adam']) - min(times['norm + fused adam']):.3f} / "
    f"{max(times['norm + scale + adam']) - min(times['norm + scale + adam']):.3f} ms)",
    f"fused clipped step == in-place scale + plain step on the first 8 tensors, bit for bit: {same}; the in-place route rewrote p.grad: {rewritten}",
]
text = "\n".join(lines) + "\n"
print(text, end="")
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)

assert same and rewritten, "the fused clipped step and scale-then-step disagree"
