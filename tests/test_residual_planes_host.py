"""CPU (no GPU): what the +1-ulp tie rule of the residual planes (include/tribe_hip.h, enum tribe_c_planes) does to an encoder forward.
The stream of tests/test_gpu_residual_planes.py's encoder comparison is restated here -- NumPy bit operations for the stream (split into
hi / lo, tie rule, decode), f32 torch on the CPU for the two branches of a layer, which read hi = bf16(x) as the kernels do -- and run twice,
with and without the tie rule.  The relative L2 difference of the final x and y is the figure that test's bound is an order of magnitude over:

    depth 3 (5 plane stores of 600 x 256 words): 8 tie-ups, x 9.3e-10, y 1.0e-9, 0.003 % of the y elements differ
    depth 1 (1 plane store):                     3 tie-ups, x 4.4e-10, y 5.7e-9, 0.17 % of the y elements differ (one row of 600: the
                                                 + 1 ulp moved that row's final ScaleNorm factor by an ulp)

REL_L2_MEASURED holds the larger of x and y per depth, REL_L2_BOUND ten times that.  The figures are printed, and held under the bound, so
that a BLAS that rounds the branches differently (other tie-ups, same order of magnitude) shows in the log."""

import math

import numpy as np
import torch

REL_L2_MEASURED = {3: 1.03e-9, 1: 5.71e-9}
REL_L2_BOUND = {depth: 10 * v for depth, v in REL_L2_MEASURED.items()}

B, T, DIM, HEADS, DIM_HEAD = 3, 200, 256, 2, 128


def make_encoder(depth: int):
    """dim 256, 2 heads x 128, ff_inner 1024; seeded weights, residual scales away from 1."""
    from modeling_utils.models.transformer import HipEncoder

    torch.manual_seed(100 + depth)
    enc = HipEncoder(dim=DIM, depth=depth, heads=HEADS, dim_head=DIM_HEAD, ff_mult=4).eval()
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith("residual_scale"):
                p.copy_(torch.rand(p.shape) * 0.5 + 0.75)
    return enc


def encoder_input():
    return torch.randn(B * T, DIM, generator=torch.Generator().manual_seed(42))


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def through_planes(x: torch.Tensor, tie_rule: bool) -> tuple[torch.Tensor, int]:
    """x -> (hi, lo) -> x as the plane epilogues store and re-read it.  Returns the decoded stream and the number of tie-ups."""
    w = x.numpy().view(np.uint32)
    hi = bf(x).numpy().view(np.uint32) >> 16                      # RNE, as f32_to_bf16
    tie = (w & 0x1FFFF) == 0x18000
    lo = np.where(tie, 0x8001, w & 0xFFFF).astype(np.uint32)
    back = ((hi - (lo > 0x8000)) << 16) | lo
    assert np.array_equal(back, w + tie)                          # the format itself: lossless but for + 1 ulp at the tie-ups
    out = back if tie_rule else w
    return torch.from_numpy(out.view(np.float32).copy()), int(tie.sum())


def _rotary(q: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, rot: int) -> torch.Tensor:
    """interleaved pairs (2 i, 2 i + 1) of the first `rot` features of every head; q [B, T, heads, dim_head]"""
    a, b = q[..., 0:rot:2], q[..., 1:rot:2]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    out = q.clone()
    out[..., 0:rot:2], out[..., 1:rot:2] = a * c - b * s, a * s + b * c
    return out


def restated_forward(enc, x: torch.Tensor, tie_rule: bool):
    """The encoder forward with the stream kept as the kernels keep it: branches read hi = bf16(x) times the ScaleNorm factor of the f32 x."""
    depth, inner, rot = enc.depth, HEADS * DIM_HEAD, enc.rotary_emb_dim
    t = torch.arange(T, dtype=torch.float32)
    freqs = torch.einsum("i,j->ij", t, enc.rotary_pos_emb.inv_freq.float())
    cos, sin = freqs.cos(), freqs.sin()
    ties, factor = 0, None

    def norm_factor(x, norm):
        return norm.g.detach() * norm.gain_scale / x.norm(dim=1, keepdim=True).clamp_min(norm.eps)

    for l in range(depth):
        norms_a, attn, ares = enc.layers[2 * l]
        norms_f, ff, fres = enc.layers[2 * l + 1]
        wqkv = bf(torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]).detach())
        qkv = bf((factor if l else norm_factor(x, norms_a[0])) * (bf(x) @ wqkv.t()))
        q, k, v = (qkv[:, i * inner:(i + 1) * inner].reshape(B, T, HEADS, DIM_HEAD) for i in range(3))
        q, k = bf(_rotary(q, cos, sin, rot)), bf(_rotary(k, cos, sin, rot))
        s = torch.einsum("bthd,bshd->bhts", q, k) / math.sqrt(DIM_HEAD)
        ao = bf(torch.einsum("bhts,bshd->bthd", s.softmax(-1), v).reshape(B * T, inner))
        x = ao @ bf(attn.to_out.weight.detach()).t() + x * ares.residual_scale.detach()
        factor = norm_factor(x, norms_f[0])   # row_sumsq is taken from the f32 value BEFORE the split
        x, n = through_planes(x, tie_rule)
        ties += n
        h = bf(torch.nn.functional.gelu(factor * (bf(x) @ bf(ff.ff[0][0].weight.detach()).t()) + ff.ff[0][0].bias.detach()))
        x = h @ bf(ff.ff[2].weight.detach()).t() + ff.ff[2].bias.detach() + x * fres.residual_scale.detach()
        if l + 1 < depth:
            factor = norm_factor(x, enc.layers[2 * l + 2][0][0])
            x, n = through_planes(x, tie_rule)
            ties += n
    return x, x * norm_factor(x, enc.final_norm), ties


def measure(depth: int):
    enc = make_encoder(depth)
    with torch.no_grad():
        x_f, y_f, ties = restated_forward(enc, encoder_input(), False)
        x_p, y_p, _ = restated_forward(enc, encoder_input(), True)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())   # noqa: E731
    return rel(x_p, x_f), rel(y_p, y_f), ties, float((y_p != y_f).float().mean())


def test_cpu_restatement_of_the_tie_rule():
    for depth in (3, 1):
        rel_x, rel_y, ties, differing = measure(depth)
        print(f"depth {depth}: {ties} tie-ups; rel L2 x {rel_x:.3e}, y {rel_y:.3e}; y elements that differ {differing:.3e}")
        assert max(rel_x, rel_y) <= REL_L2_BOUND[depth], (depth, rel_x, rel_y)
        assert differing <= 0.01


def test_tie_rule_on_chosen_words():
    words = np.array([0x3F808000, 0x3F818000, 0xBF818000, 0x3F818001, 0x3F807FFF, 0x7F7F8000, 0x00000000, 0x80000000, 0x7F800000], dtype=np.uint32)
    back, ties = through_planes(torch.from_numpy(words.view(np.float32).copy()), True)
    want = words + np.array([0, 1, 1, 0, 0, 1, 0, 0, 0], dtype=np.uint32)
    assert ties == 3 and np.array_equal(back.numpy().view(np.uint32), want)
