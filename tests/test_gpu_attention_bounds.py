"""GPU: every attention kernel, element by element, against float64 (oracle/attention_ref.py) on every branch its launcher takes.

Forward bound, asserted on ALL elements: |got - out64| <= forward_bound = 2^-8 (P @ |v|) + 2^-7 |out64| + 1e-6, u = 2^-8 being the
unit roundoff of bf16 (round to nearest even):
  * each p_j is rounded to bf16 once before P V:                  u sum_j P_ij |v_jd|
  * the denominator may be the sum of the rounded p:              u |out|
  * the output is rounded to bf16 once:                           u |out|
  * f32 score accumulation, exp2, the running sum:                under the constant 1e-6
The deferred maximum (p up to 2^8) scales numerator and denominator alike and leaves the relative roundings unchanged.

Log-sum-exp bound per row: 2 [ K 2^-24 scale log2e max_j sum_d |q_id k_jd| + (T + 16) 2^-24 / ln 2 ]: f32 accumulation of the K
products of a score, then an f32 sum of T terms plus exp2 / log2.  The only kernel with the output (dim_head 384, one wave per SIMD)
adds the unrounded p to its running sum, so the term log2(1 + 2^-8) of a kernel that sums rounded p (lse_bound(rounded_p_sum=True))
is NOT granted to it.

Backward: gradients of the fused qkv buffer against the closed-form float64 gradients, two metrics per (tensor in dq / dk / dv,
sequence, head):
  * row:  e_t = |got_t - want_t|_2 / RMS_t |want_t|_2 for every row t -- a garbage or zeroed row scores ~1 whatever the tensor's size;
  * gain: <got, want> / <want, want> - 1 over the slice -- rounding noise averages out of it, a wrong scale does not.
Their bounds are 4 x the largest error of the clean CPU emulation (emulate_backward: bf16 dO, O inside D on the fused path, P, dS, the
three gradients) over all cases of a path; the factor covers MFMA summation order and the hardware exp2.  Measured on the CPU by
tests/test_attention_host.py, which also shows every injected fault at >= 3 x the bound; never taken from GPU output:
      path           row floor   row bound   gain floor   gain bound
      fused          0.0252      0.104       1.27e-3      5.2e-3
      materialised   0.0208      0.084       1.16e-3      4.8e-3
Backward inputs are `diffuse` and `conc` = perm(c) with c = 0.6 sqrt(64 / d), i.e. perm(0.6) at the logit lead (4.8) it has at dim_head
64.  perm(0.6) itself leads by 11.8 at dim_head 384 and is one-hot there, the regime in which dS = P (dP - D) cancels against a D made
from the bf16 O: the clean emulation errs by 4.6 row norms on it, legitimate noise that would make any floor useless.

Forward grid of attention(): head size x mode x length x input kind in full -- dim_head 64: modes 0 1 2 4 5, 128 / 192: 0 1 2,
384: 0 1 2 3; lengths 1 7 32 33 128 129 161 300 (+ 1000 at dim_head 64); diffuse, perm(2), perm(0.6).  Pruned is only (B, heads): the
pair at (length index i, kind index j) is ((1,1), (3,1), (2,4), (3,3))[(i + j) % 4] whatever the kernel, so every (kernel, length,
kind) occurs, every kernel meets all four pairs (B heads % 8 = 1, 3, 0, 1; (3,3) is more than one group of 8), and kernels share
the float64 reference of a (length, kind).

Worst |got - out64| / bound seen on an MI355X, for the record (the bounds are not tuned to these):
  forward, |got - out64| / forward_bound:
      16-row kernel, dim_head 64 / 128 / 192 / 384      0.54 / 0.44 / 0.48 / 0.51     causal: 0.66 / 0.63 / 0.62 / 0.62
      dim_head 64, 64-row kernels (by grid, 4-wave, 8-wave)   0.54 each; grouped-query 0.52 each; relative-key 0.40 each (16-row: 0.42)
      dim_head 128 grouped-query                        0.45
      dim_head 384 one wave per SIMD / key-split        0.51 / 0.51            with the in-kernel Q rotary: 0.61, bit-equal to the
                                                                               stand-alone pass in all 36 runs
      materialised (three kernels)                      0.62
  log-sum-exp (dim_head 384, one wave per SIMD), |lse2 - lse2_64| / lse_bound: 0.009
  backward, row metric: fused 0.0252, materialised 0.0208 (bounds 0.104 / 0.084); gain metric: 1.3e-3 / 1.2e-3 (bounds 5.2e-3 / 4.8e-3)
  -- the kernels land on the CPU emulation's own worst rows, so a quarter of each bound.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention_ref as ar  # noqa: E402

_worst = {}   # kernel -> (ratio, where): printed when the module is done (pytest -s)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    yield _ops
    for name in sorted(_worst):
        print(f"\nworst ratio {name:32s} {_worst[name][0]:8.4f}  {_worst[name][1]}", end="")
    print()


def kernel_name(d: int, mode: int, *, causal: bool = False, rel: bool = False, entry: str = "") -> str:
    if d not in (64, 128, 192, 384) or (mode == 1 and entry == "attention"):
        return "materialised"
    if rel:
        return {0: "d64 64-row by grid, relkey", 2: "16-row<64> relkey", 4: "d64 4-wave relkey", 5: "d64 8-wave relkey"}[mode]
    if causal:
        return f"16-row<{d}> causal"
    if d == 64:
        return {0: "d64 64-row by grid", 2: "16-row<64>", 4: "d64 4-wave", 5: "d64 8-wave"}.get(mode, "d64 64-row by grid")
    if d == 384:
        return {0: "wide384", 2: "16-row<384>", 3: "ksplit384"}.get(mode, "wide384")
    return f"16-row<{d}>"


@functools.lru_cache(maxsize=6)
def reference(kind: str, B: int, T: int, hq: int, hkv: int, d: int, causal: bool = False, rel: tuple | None = None):
    """Computed once per input, shared by every kernel that runs it, never modified: the packed bf16-exact qkv, the float64 output
    [B, hq, T, d], its bound, the float64 log-sum-exp, q, k and the relative-key table."""
    q, k, v = ar.make_inputs(kind, B, T, hq, d, seed=1000 * d + T, heads_kv=hkv, causal=causal)
    scale = d**-0.5
    kk, vv = ar.repeat_kv(k, hq), ar.repeat_kv(v, hq)
    qe = bias = None
    if rel is not None:
        qe = ar.relative_key_table(q, *rel, seed=5)
        bias = ar.relative_key_bias(qe, T, *rel)
    out64, P, lse64 = ar.attention_f64(q, kk, vv, scale, causal=causal, bias=bias)
    return ar.pack_qkv(q, k, v), out64, ar.forward_bound(P, vv, out64), lse64, q, kk, qe


def check(got_dev: torch.Tensor, out64: torch.Tensor, bound: torch.Tensor, kernel: str, what: str) -> None:
    """|got - out64| <= bound on all elements; on failure the worst ratio and its (b, t, head, d)."""
    B, h, T, d = out64.shape
    got = ar.unpack_out(got_dev.float().cpu(), B, T, h, d)
    ratio, (b, hd, t, e) = ar.ratio_report(got, out64, bound)
    if ratio > _worst.get(kernel, (0.0, ""))[0]:
        _worst[kernel] = (ratio, what)
    assert ratio <= 1.0, f"{kernel}, {what}: |got - float64| is {ratio:.2f} x the bound at (b, t, head, d) = ({b}, {t}, {hd}, {e})"


def _dev(t: torch.Tensor) -> torch.Tensor:
    return t.cuda().bfloat16()


MODES = {64: (0, 1, 2, 4, 5), 128: (0, 1, 2), 192: (0, 1, 2), 384: (0, 1, 2, 3)}
GRID = [(d, T, mode) for d in MODES for T in ar.forward_lengths(d) for mode in MODES[d]]


@pytest.mark.parametrize("d,T,mode", GRID)
def test_attention_all_kernels(ops, d, T, mode):
    it = ar.forward_lengths(d).index(T)
    ops.attention_set_mode(mode)
    try:
        for ik, kind in enumerate(ar.KINDS):
            B, h = ar.forward_batch_heads(it, ik)
            qkv, out64, bound, *_ = reference(kind, B, T, h, h, d)
            got = ops.attention(_dev(qkv), B, T, h, d, d**-0.5)
            check(got, out64, bound, kernel_name(d, mode, entry="attention"), f"d={d} T={T} B={B} h={h} mode={mode} {kind}")
    finally:
        ops.attention_set_mode(0)


@pytest.mark.parametrize("T", [7, 129, 300])
def test_attention_head_size_without_fused_kernel(ops, T):
    """dim_head 256 has no fused kernel: mode 0 falls to the three-kernel path."""
    for ik, kind in enumerate(ar.KINDS):
        B, h = ar.forward_batch_heads(T % 3, ik)
        qkv, out64, bound, *_ = reference(kind, B, T, h, h, 256)
        check(ops.attention(_dev(qkv), B, T, h, 256, 256**-0.5), out64, bound, kernel_name(256, 0), f"d=256 T={T} B={B} h={h} {kind}")


def test_attention_materialised_in_two_chunks(ops):
    """(B, T, h, d) = (7, 1024, 8, 64): 32 MiB of f32 scores per sequence against the 192 MiB budget -> chunks of 6 and 1 sequences."""
    B, T, h, d = 7, 1024, 8, 64
    q, k, v = ar.make_inputs("diffuse", B, T, h, d, seed=77)
    ops.attention_set_mode(1)
    try:
        got = ops.attention(_dev(ar.pack_qkv(q, k, v)), B, T, h, d, d**-0.5).float().cpu().view(B, T * h * d)
    finally:
        ops.attention_set_mode(0)
    for b in range(B):   # the reference one sequence at a time: P is 64 MiB per sequence in float64
        out64, P, _ = ar.attention_f64(q[b:b + 1], k[b:b + 1], v[b:b + 1], d**-0.5)
        check(got[b].view(T, h * d), out64, ar.forward_bound(P, v[b:b + 1], out64), "materialised", f"two chunks, sequence {b}")


GQA_SHAPES = ((1, 1, 1), (3, 3, 1), (2, 4, 2))   # (B, heads_q, heads_kv): plain, groups of 3 and of 2


@pytest.mark.parametrize("T", [1, 7, 33, 128, 161, 300])
@pytest.mark.parametrize("d", [64, 128, 192, 384])
def test_attention_gqa_causal(ops, d, T):
    for ik, kind in enumerate(ar.KINDS):
        B, hq, hkv = GQA_SHAPES[(T + ik) % 3]
        qkv, out64, bound, *_ = reference(kind, B, T, hq, hkv, d, True)
        got = ops.attention_gqa(_dev(qkv), B, T, hq, hkv, d, d**-0.5, True)
        check(got, out64, bound, kernel_name(d, 0, causal=True), f"causal d={d} T={T} B={B} heads {hq}/{hkv} {kind}")


@pytest.mark.parametrize("T", [7, 33, 129, 300])
@pytest.mark.parametrize("d,mode", [(64, 0), (64, 4), (64, 5), (128, 0)])
def test_attention_gqa_bidirectional(ops, d, mode, T):
    ops.attention_set_mode(mode)
    try:
        for ik, kind in enumerate(ar.KINDS):
            B, hq, hkv = GQA_SHAPES[1 + (T + ik) % 2]
            qkv, out64, bound, *_ = reference(kind, B, T, hq, hkv, d)
            got = ops.attention_gqa(_dev(qkv), B, T, hq, hkv, d, d**-0.5, False)
            check(got, out64, bound, kernel_name(d, mode) + " gqa", f"d={d} T={T} B={B} heads {hq}/{hkv} mode={mode} {kind}")
    finally:
        ops.attention_set_mode(0)


@pytest.mark.parametrize("mode", [0, 2, 4, 5])
@pytest.mark.parametrize("T,left,right", ar.RELATIVE_KEY_GEOMETRIES)
def test_attention_relative_key(ops, T, left, right, mode):
    """The table is q . E with E ~ N(0, 1): the bias has the spread of the content scores q . k."""
    d, B, h = 64, 2, 3
    npos = left + right + 1
    stride = (npos + 7) // 8 * 8
    ops.attention_set_mode(mode)
    try:
        for kind in ("diffuse", "perm06"):
            qkv, out64, bound, _, _, _, qe = reference(kind, B, T, h, h, d, False, (left, right))
            qe_dev = torch.zeros(B * T, h, stride)
            qe_dev[:, :, :npos] = qe.permute(0, 2, 1, 3).reshape(B * T, h, npos)
            got = ops.attention_relative_key(_dev(qkv), B, T, h, d, d**-0.5, qe_dev.cuda(), left, right)
            check(got, out64, bound, kernel_name(d, mode, rel=True), f"T={T} band -{left}..{right} mode={mode} {kind}")
    finally:
        ops.attention_set_mode(0)


@pytest.mark.parametrize("T", [7, 129, 300])
def test_attention_log_sum_exp(ops, T):
    d = 384
    it = ar.forward_lengths(d).index(T)
    for ik, kind in enumerate(ar.KINDS):
        B, h = ar.forward_batch_heads(it, ik)
        qkv, out64, bound, lse64, q, k, _ = reference(kind, B, T, h, h, d)
        dev = _dev(qkv)
        out, lse = ops.attention_with_lse(dev, B, T, h, d, d**-0.5)
        assert torch.equal(out, ops.attention(dev, B, T, h, d, d**-0.5)), "asking for the log-sum-exp changed the output"
        check(out, out64, bound, "wide384", f"with lse, T={T} B={B} h={h} {kind}")
        lb = ar.lse_bound(q, k, d**-0.5, T, d)          # unrounded p in the running sum: no log2(1 + 2^-8) term
        ratio, (b, hd, t) = ar.ratio_report(lse.cpu(), lse64, lb)
        if ratio > _worst.get("wide384 lse", (0.0, ""))[0]:
            _worst["wide384 lse"] = (ratio, f"T={T} {kind}")
        assert ratio <= 1.0, f"lse2 off by {ratio:.2f} x its bound at (b, head, t) = ({b}, {hd}, {t}), T={T} {kind}"


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("rot_dim", [32, 192, 384])
@pytest.mark.parametrize("T", [7, 129, 300])
def test_attention_rotates_q_in_kernel(ops, T, rot_dim, h):
    """The production path at dim_head 384: the stand-alone rotary pass runs on the k heads only, the attention kernel rotates Q as it
    loads it.  Its output must be bit-equal to attention() on the buffer with q and k both rotated by the stand-alone pass, and
    within forward_bound of float64 on those rotated values."""
    from tribe_hip._lib import check as rc_check, lib

    d, B = 384, (2 if h == 1 else 3)
    inner, scale = h * d, d**-0.5
    stream = torch.cuda.current_stream().cuda_stream
    cos, sin = (t.cuda() for t in ar.rotary_tables(T, rot_dim))
    for kind in ("diffuse", "perm06"):
        q, k, v = ar.make_inputs(kind, B, T, h, d, seed=rot_dim + T)
        raw = _dev(ar.pack_qkv(q, k, v))
        both = ops.rotary_(raw.clone(), T, h, d, rot_dim, cos, sin, True)
        k_only = raw.clone()
        rc_check(lib().tribe_rotary_fwd(k_only.data_ptr() + 2 * inner, B * T, T, 3 * inner, h, d, rot_dim, cos.data_ptr(), sin.data_ptr(), 1,
                                        stream), "tribe_rotary_fwd")
        assert torch.equal(k_only[:, inner:], both[:, inner:]) and torch.equal(k_only[:, :inner], raw[:, :inner])
        want = ops.attention(both, B, T, h, d, scale)
        got = torch.empty_like(want)
        rc_check(lib().tribe_debug_attention_qrot(k_only.data_ptr(), B, T, h, d, scale, got.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                  rot_dim, stream), "tribe_debug_attention_qrot")
        qr, kr, vr = ar.unpack_qkv(both.float().cpu(), B, T, h, d)
        out64, P, _ = ar.attention_f64(qr, kr, vr, scale)
        check(got, out64, ar.forward_bound(P, vr, out64), "wide384 q rotary", f"T={T} rot_dim={rot_dim} B={B} h={h} {kind}")
        n_diff = int((got != want).sum())
        assert n_diff == 0, f"in-kernel Q rotary differs from the stand-alone pass in {n_diff} of {got.numel()} outputs ({kind})"


BACKWARD = [(case, kind) for case in ar.BACKWARD_CASES for kind in ar.BACKWARD_KINDS]


@pytest.mark.parametrize("case,kind", BACKWARD, ids=["-".join(str(x) for x in c) + "-" + k for c, k in BACKWARD])
def test_attention_backward(ops, case, kind):
    from modeling_utils import autograd as ag

    path, B, T, h, d, chunk_seqs, rot = case
    q, k, v, dout, scale, rotary, want = ar.backward_case_inputs(case, kind)
    keep = ag.Attention.CHUNK_BYTES, ag.Attention.CHUNK_BYTES_FUSED, ag.Attention.FUSED_SOFTMAX
    try:
        ag.Attention.CHUNK_BYTES = ag.Attention.CHUNK_BYTES_FUSED = chunk_seqs * h * T * ops.round_up(T, 64) * 4
        if path == "materialised" and d == 384:
            ag.Attention.FUSED_SOFTMAX = False
        x = _dev(ar.pack_qkv(q, k, v)).requires_grad_()
        if rot:
            cos, sin = (t.cuda() for t in rotary)
            out, _ = ag.RotaryAttention.apply(x * 1, cos, sin, (-sin).contiguous(), B, T, h, d, scale, rot, True)
        else:
            out = ag.Attention.apply(x, B, T, h, d, scale)
        assert (len(out.grad_fn.saved_tensors) == 3) == (path == "fused")
        out.backward(_dev(dout.transpose(1, 2).reshape(B * T, h * d)))
    finally:
        ag.Attention.CHUNK_BYTES, ag.Attention.CHUNK_BYTES_FUSED, ag.Attention.FUSED_SOFTMAX = keep
    got = x.grad.float().cpu().view(B, T, 3, h, d)
    e = ar.row_errors(got, want)
    gain = ar.gain_errors(got, want).abs()
    b, t, i, hd = (int(n) for n in torch.unravel_index(e.argmax(), e.shape))
    for name, val in ((f"backward {path} row", float(e.max())), (f"backward {path} gain", float(gain.max()))):
        if val > _worst.get(name, (0.0, ""))[0]:
            _worst[name] = (val, f"{case} {kind}")
    row_bound = ar.BACKWARD_MARGIN * ar.BACKWARD_ROW_FLOOR[path]
    gain_bound = ar.BACKWARD_MARGIN * ar.BACKWARD_GAIN_FLOOR[path]
    assert float(e.max()) <= row_bound, (f"row {t} of {'dq dk dv'.split()[i]}[b={b}, head={hd}] is {float(e.max()):.4f} typical row norms "
                                         f"from float64 (bound {row_bound:.3f})")
    assert float(gain.max()) <= gain_bound, (f"gain errors (b, tensor, head) {gain.flatten().tolist()} beyond {gain_bound:.1e}")
