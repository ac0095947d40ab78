"""GPU: modeling_utils.autograd.Attention / RotaryAttention with causal=True against a float64 torch composition (scores with key > query at
-inf before the softmax, attention dropout as the restated mask of tests/dropout_restatement.py on the logical [B * heads * T, T] tensor).
Bounds are the ones tests/test_gpu_training.py and tests/test_gpu_attn_dropout.py apply: 2e-2 relative L2 on the output, 3e-2 per q / k / v
third of dqkv.  Causality itself is checked exactly: the materialised route computes a query row from its own visible keys only, and what it
multiplies by the masked ones is an exact zero."""

import functools

import pytest
import torch

from tests.dropout_restatement import multiplier

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SITE = (4 << 56) | 1
SHAPES = [(2, 70, 2, 64), (2, 64, 3, 128), (1, 298, 2, 384)]   # (B, T, h, d)
CUTS = [(2, 70, 2, 64, 40), (1, 298, 2, 384, 130)]            # ... and the last visible position t of the exact-causality checks


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pad(T):
    return (T + 63) // 64 * 64


def _rot_dim(d):
    return max(d // 2, 32)


@functools.lru_cache(maxsize=None)
def _inputs(B, T, h, d):
    g = torch.Generator().manual_seed(14)
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)  # noqa: E731
    return bf(torch.randn(B * T, 3 * h * d, generator=g)), bf(torch.randn(B * T, h * d, generator=g))


@functools.lru_cache(maxsize=None)
def _case(B, T, h, d, rotary, p):
    """(float64 output, float64 dqkv) of softmax(causal(scale q k^T)) * m @ v: computed once per case, never modified."""
    from oracle import xt_encoder

    qkv, dout = _inputs(B, T, h, d)
    qt = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in qt.view(B, T, 3, h, d).unbind(2))          # [B, h, T, d]
    if rotary:
        freqs = xt_encoder.RotaryEmbedding(_rot_dim(d), interleaved=True)(T).double()
        q, k = (xt_encoder.apply_rotary_pos_emb(t, freqs, True) for t in (q, k))
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * d**-0.5
    att = sim.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf")).softmax(-1)
    if p > 0:
        att = att * multiplier(B * h * T, T, p, SEED, SITE).view(B, h, T, T)
    out = torch.einsum("bhij,bhjd->bhid", att, v).transpose(1, 2).reshape(B * T, h * d)
    out.backward(dout.double())
    return out.detach(), qt.grad


def _run(B, T, h, d, rotary, qkv, dout, *extra):
    from modeling_utils import autograd as ag
    from oracle import xt_encoder

    qg = qkv.cuda().bfloat16().requires_grad_()
    if rotary:
        rot = _rot_dim(d)
        half = torch.einsum("i,j->ij", torch.arange(T).float(), xt_encoder.RotaryEmbedding(rot).inv_freq.float())
        cos, sin = half.cos().cuda().contiguous(), half.sin().cuda().contiguous()
        out, _ = ag.RotaryAttention.apply(qg * 1, cos, sin, (-sin).contiguous(), B, T, h, d, d**-0.5, rot, True, *extra)
    else:
        out = ag.Attention.apply(qg, B, T, h, d, d**-0.5, *extra)
    out.backward(dout.cuda().bfloat16())
    return out.detach(), qg.grad


def _thirds(grad, B, T, h, d):
    g = grad.view(B, T, 3, h, d)
    return {"dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", SHAPES)
def test_causal_attention_vs_float64(B, T, h, d, rotary, p):
    qkv, dout = _inputs(B, T, h, d)
    want, want_grad = _case(B, T, h, d, rotary, p)
    got, grad = _run(B, T, h, d, rotary, qkv, dout, p, SEED, SITE, True)
    err = _rel(got.float().cpu(), want)
    print(f"(B, T, h, d) = {(B, T, h, d)} rotary={rotary} p={p}: output rel L2 {err:.2e}")
    assert err < 2e-2
    wants = _thirds(want_grad, B, T, h, d)
    for name, g in _thirds(grad.float().cpu(), B, T, h, d).items():
        err = _rel(g, wants[name])
        print(f"(B, T, h, d) = {(B, T, h, d)} rotary={rotary} p={p}: {name} rel L2 {err:.2e}")
        assert err < 3e-2, name


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", [s for s in SHAPES if s[0] > 1])
def test_result_does_not_depend_on_the_chunking(B, T, h, d, rotary, p, monkeypatch):
    """One sequence per chunk against every sequence in one chunk: row0 carries both the mask's index and the query index."""
    from modeling_utils import autograd as ag

    qkv, dout = _inputs(B, T, h, d)
    monkeypatch.setattr(ag.Attention, "CHUNK_BYTES", B * h * T * _pad(T) * 4)
    whole, whole_grad = _run(B, T, h, d, rotary, qkv, dout, p, SEED, SITE, True)
    monkeypatch.setattr(ag.Attention, "CHUNK_BYTES", h * T * _pad(T) * 4)
    each, each_grad = _run(B, T, h, d, rotary, qkv, dout, p, SEED, SITE, True)
    assert torch.equal(_bits(each), _bits(whole)) and torch.equal(_bits(each_grad), _bits(whole_grad))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d,t", CUTS)
def test_forward_is_exactly_causal(B, T, h, d, t, rotary, p):
    """Replacing the rows at positions > t of every sequence changes no output value at positions <= t."""
    qkv, dout = _inputs(B, T, h, d)
    other = qkv.view(B, T, -1).clone()
    g = torch.Generator().manual_seed(3)
    other[:, t + 1:] = (torch.randn(B, T - t - 1, other.shape[-1], generator=g) * 3.0).to(torch.bfloat16).float()
    a, _ = _run(B, T, h, d, rotary, qkv, dout, p, SEED, SITE, True)
    b, _ = _run(B, T, h, d, rotary, other.view(B * T, -1), dout, p, SEED, SITE, True)
    a, b = a.view(B, T, -1), b.view(B, T, -1)
    assert torch.equal(_bits(a[:, : t + 1]), _bits(b[:, : t + 1]))
    assert not torch.equal(a[:, t + 1:], b[:, t + 1:])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d,t", CUTS)
def test_backward_is_exactly_causal(B, T, h, d, t, rotary, p):
    """The backward of out[positions <= t].sum() leaves the rows of dqkv at positions > t exactly zero."""
    qkv, _ = _inputs(B, T, h, d)
    dout = torch.zeros(B, T, h * d)
    dout[:, : t + 1] = 1.0
    _, grad = _run(B, T, h, d, rotary, qkv, dout.view(B * T, -1), p, SEED, SITE, True)
    grad = grad.view(B, T, -1)
    assert bool((grad[:, t + 1:] == 0).all()) and bool((grad[:, : t + 1] != 0).any())
    assert torch.isfinite(grad.float()).all()


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", SHAPES)
def test_causal_false_is_the_call_without_the_argument(B, T, h, d, rotary, monkeypatch):
    """causal=False through the new trailing argument launches what it did before -- the causal kernels are never called -- and gives the bits
    of a call that does not pass it, at p = 0 and with attention dropout."""
    from tribe_hip import ops

    def never(*a, **kw):
        raise AssertionError("a causal kernel was launched for causal=False")

    monkeypatch.setattr(ops, "softmax_causal_fwd", never)
    monkeypatch.setattr(ops, "softmax_causal_bwd", never)
    qkv, dout = _inputs(B, T, h, d)
    for drop in ((), (0.1, SEED, SITE)):
        a, ga = _run(B, T, h, d, rotary, qkv, dout, *drop)
        b, gb = _run(B, T, h, d, rotary, qkv, dout, *(drop or (0.0, 0, 0)), False)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ga), _bits(gb))
