"""CPU: the bounds of tests/test_gpu_attention_bounds.py have teeth, shown without a GPU.

oracle/attention_ref.py restates the attention kernels and `modeling_utils/autograd.py::Attention.backward` in torch f32 with their
bf16 roundings (`emulate_forward`, `emulate_backward`).  Here, on the shapes and inputs of the GPU tests:
  * the clean emulation stays inside `forward_bound` (worst ratio seen: 0.59) and at or under the recorded backward floors;
  * every injected fault breaks its bound by >= 3x in the inputs its docstring line names.
The backward floors are the largest clean error per path; the GPU tests hold the kernels to 4 x that.  A 2.5 % scale error of dQ moves
a row by 0.05 - 0.16 row norms, 0.5 - 1.9 x the row bound, so the row metric alone cannot promise to see it; the gain metric (the
projection of a whole (sequence, head) slice on the reference, where rounding noise averages out) sees it at 4.8 x its bound.
"""

import math

import pytest
import torch

from oracle import attention_ref as ar

HEAD_SIZES = (64, 128, 192, 384)
FAULT_FACTOR = 3.0


def _forward_ratio(q, k, v, scale, out64, bound, **kw):
    got, _ = ar.emulate_forward(ar.repeat_kv(q, q.shape[1]), ar.repeat_kv(k, q.shape[1]), ar.repeat_kv(v, q.shape[1]), scale, **kw)
    return ar.ratio_report(got, out64, bound)[0]


def _forward_cases(d):
    """(T, B, h, kind) of the attention() grid of the GPU tests at this head size."""
    for it, T in enumerate(ar.forward_lengths(d)):
        for ik, kind in enumerate(ar.KINDS):
            yield (T, *ar.forward_batch_heads(it, ik), kind)


def test_input_builders():
    for causal in (False, True):
        q, k, v = ar.perm(0.6, 2, 33, 3, 64, seed=1, causal=causal)
        for t in (q, k, v):
            assert torch.equal(t, ar.bf(t))
        pi = ar.perm_targets(33, 3, causal)
        if causal:
            assert (pi <= torch.arange(33)).all() and (pi[:, 0::2] == torch.arange(0, 33, 2)).all()
        else:   # every key is some row's target, in every head; row 0 of head 0 aims at the last key
            assert all(sorted(row.tolist()) == list(range(33)) for row in pi) and pi[0, 0] == 32
        assert torch.equal(q, ar.bf(0.6 * torch.gather(k, 2, pi[None, :, :, None].expand(2, 3, 33, 64))))
    q, k, v = ar.perm(2.0, 1, 40, 4, 64, seed=2, heads_kv=2)
    assert k.shape[1] == 2 and torch.equal(q[0, 3, 0], ar.bf(2.0 * k[0, 1, ar.perm_targets(40, 4, False)[3, 0]]))
    qkv = ar.pack_qkv(q, k, v)
    assert qkv.shape == (40, (4 + 2 * 2) * 64) and torch.equal(qkv[:, 4 * 64:5 * 64], k[0, 0])


def test_float64_backward_is_autograd():
    q, k, v = (t.double().requires_grad_() for t in ar.diffuse(2, 19, 2, 16, seed=3))
    dout = torch.randn(2, 2, 19, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    ((torch.einsum("bhid,bhjd->bhij", q, k) * 0.25).softmax(-1) @ v).backward(dout)
    out, P, lse2 = ar.attention_f64(q.detach(), k.detach(), v.detach(), 0.25)
    for got, want in zip(ar.attention_backward_f64(q.detach(), k.detach(), v.detach(), P, dout, 0.25), (q.grad, k.grad, v.grad)):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    s = torch.einsum("bhid,bhjd->bhij", q.detach(), k.detach()) * 0.25
    torch.testing.assert_close(lse2, torch.logsumexp(s, -1) / math.log(2.0), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(out, s.softmax(-1) @ v.detach(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("d", HEAD_SIZES)
def test_forward_clean_emulation_within_bound_and_faults_break_it(d):
    """Bidirectional and causal, every length and input kind of the GPU grid.  Named inputs per fault: emulate_forward's docstring."""
    scale = d**-0.5
    worst = 0.0
    for causal in (False, True):
        for T, B, h, kind in _forward_cases(d):
            q, k, v = ar.make_inputs(kind, B, T, h, d, seed=T + d, causal=causal)
            out64, P, _ = ar.attention_f64(q, k, v, scale, causal=causal)
            bound = ar.forward_bound(P, v, out64)
            r = _forward_ratio(q, k, v, scale, out64, bound, causal=causal)
            worst = max(worst, r)
            assert r <= 1.0, f"clean emulation at {r:.2f} x the bound: d={d} T={T} causal={causal} {kind}"
            named = []
            if T >= 7 and not causal and kind in ("perm2", "perm06"):
                named.append("drop_last_key")
            if T >= 7 and not causal and (kind == "diffuse" or (kind == "perm06" and d == 64)):
                named.append("double_last_key")
            if T >= 7 and causal:
                named.append("exclude_diagonal")
            if T > ar.KEY_TILE and not causal and kind == "perm2":
                named.append("skip_rescale")
            for fault in named:
                rf = _forward_ratio(q, k, v, scale, out64, bound, causal=causal, fault=fault)
                assert rf >= FAULT_FACTOR, f"{fault} reaches only {rf:.2f} x the bound: d={d} T={T} causal={causal} {kind}"
    print(f"dim_head {d}: clean emulation at most {worst:.3f} x forward_bound")


@pytest.mark.parametrize("T,left,right", ar.RELATIVE_KEY_GEOMETRIES)
def test_relative_key_clean_and_band_faults(T, left, right):
    d, B, h = 64, 2, 3
    for kind in ("diffuse", "perm06"):
        q, k, v = ar.make_inputs(kind, B, T, h, d, seed=T + left)
        qe = ar.relative_key_table(q, left, right, seed=5)
        out64, P, _ = ar.attention_f64(q, k, v, d**-0.5, bias=ar.relative_key_bias(qe, T, left, right))
        bound = ar.forward_bound(P, v, out64)
        assert _forward_ratio(q, k, v, d**-0.5, out64, bound, rel=(qe, left, right)) <= 1.0
        for fault, width in (("band_left_short", left), ("band_right_short", right)):
            if width >= 1:
                rf = _forward_ratio(q, k, v, d**-0.5, out64, bound, rel=(qe, left, right), fault=fault)
                assert rf >= FAULT_FACTOR, f"{fault} reaches only {rf:.2f} x the bound at {kind}"


def test_grouped_query_heads_are_repeated_not_cycled():
    """q head i reads kv head i // group: the emulation on repeated heads is within the bound, on cycled heads (i % heads_kv) far outside."""
    q, k, v = ar.make_inputs("perm06", 2, 33, 6, 64, seed=9, heads_kv=2)
    kk, vv = ar.repeat_kv(k, 6), ar.repeat_kv(v, 6)
    out64, P, _ = ar.attention_f64(q, kk, vv, 0.125)
    bound = ar.forward_bound(P, vv, out64)
    assert ar.ratio_report(ar.emulate_forward(q, kk, vv, 0.125)[0], out64, bound)[0] <= 1.0
    assert ar.ratio_report(ar.emulate_forward(q, k.repeat(1, 3, 1, 1), v.repeat(1, 3, 1, 1), 0.125)[0], out64, bound)[0] >= FAULT_FACTOR


def test_lse_bound_holds_for_unrounded_sum_and_not_for_a_dropped_key():
    for kind in ar.KINDS:
        q, k, v = ar.make_inputs(kind, 1, 129, 2, 384, seed=11)
        scale = 384**-0.5
        _, _, lse64 = ar.attention_f64(q, k, v, scale)
        bound = ar.lse_bound(q, k, scale, 129, 384)
        _, lse = ar.emulate_forward(q, k, v, scale)
        assert ((lse.double() - lse64).abs() <= bound).all()
        _, lse = ar.emulate_forward(q, k, v, scale, fault="drop_last_key")
        assert ((lse.double() - lse64).abs() > FAULT_FACTOR * bound).any()


def _emulated(case, kind, fault=None):
    path, _, _, _, _, chunk_seqs, _ = case
    q, k, v, dout, scale, rotary, want = ar.backward_case_inputs(case, kind)
    got = ar.grads_view(*ar.emulate_backward(q, k, v, dout, scale, fused=path == "fused", chunk_seqs=chunk_seqs, rotary=rotary, fault=fault))
    return float(ar.row_errors(got, want).max()), float(ar.gain_errors(got, want).abs().max())


@pytest.fixture(scope="module")
def clean():
    """(row error, gain error) of the clean emulation on every backward case and input kind."""
    return {(case, kind): _emulated(case, kind) for case in ar.BACKWARD_CASES for kind in ar.BACKWARD_KINDS}


def test_backward_floors_are_the_measured_ones(clean):
    """The recorded floors are what the clean emulation reaches (rounded up in the second digit), not a looser figure; the bound is
    4 x the floor, so the clean emulation sits at bound / 4 or under."""
    for path in ("fused", "materialised"):
        e = max(v[0] for (case, _), v in clean.items() if case[0] == path)
        g = max(v[1] for (case, _), v in clean.items() if case[0] == path)
        print(f"{path}: row floor {e:.4f}, gain floor {g:.2e}")
        assert 0.9 * ar.BACKWARD_ROW_FLOOR[path] <= e <= ar.BACKWARD_ROW_FLOOR[path]
        assert 0.9 * ar.BACKWARD_GAIN_FLOOR[path] <= g <= ar.BACKWARD_GAIN_FLOOR[path]


@pytest.mark.parametrize("case", ar.BACKWARD_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_backward_faults_break_bound(case, clean):
    path, B, T, _, _, chunk_seqs, _ = case
    row_bound = ar.BACKWARD_MARGIN * ar.BACKWARD_ROW_FLOOR[path]
    gain_bound = ar.BACKWARD_MARGIN * ar.BACKWARD_GAIN_FLOOR[path]
    for kind in ar.BACKWARD_KINDS:
        e, g = clean[(case, kind)]
        assert e <= row_bound / 4 and g <= gain_bound / 4, f"clean emulation {kind}: row {e:.4f}, gain {g:.2e}"
        assert _emulated(case, kind, "zero_last_dk_row")[0] >= FAULT_FACTOR * row_bound, kind
        assert _emulated(case, kind, "scale_dq")[1] >= FAULT_FACTOR * gain_bound, kind
        if T % 64 != 0:
            assert _emulated(case, kind, "stale_pad_column")[0] >= FAULT_FACTOR * row_bound, kind
        if path == "fused" and chunk_seqs < B:
            assert _emulated(case, kind, "chunk_bias_off_by_one")[0] >= FAULT_FACTOR * row_bound, kind
