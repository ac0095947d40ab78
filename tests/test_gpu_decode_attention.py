"""GPU: the KV cache kernels of streamed causal encoders (csrc/attn_decode.hip).

tribe_attention_decode_fwd, element by element against oracle.attention_ref.attention_f64: the last query row of a causal problem of length n
(row n - 1 sees keys 0 .. n - 1, so the mask hides nothing from it and the reference is computed for that row alone).  Bound: the project's
derived forward bound, ar.forward_bound = 2^-8 (P |v|) + 2^-7 |out64| + 1e-6 -- p is rounded to bf16 once before P V, the output once; the
split parts are f32, so nothing new enters.  Grid: every head size the kernel is built for; n = 1, 2, 63, 64, 65, 300, 1024 plus the n either
side of each change of the split count (EDGE_N, itself checked against tribe_attention_decode_splits); (B, heads) = (1, 1), (3, 2); inputs
`diffuse` and `perm2`.  The caches have cap > n and every slot >= n holds bf16 NaN: a finite result within the bound shows nothing beyond n
is read.  Two identical calls give equal bits.

tribe_kv_append, bit for bit against ops.rotary_ on a full-length buffer, both pairings and rot_dim = 0."""

import functools

import pytest
import torch

from oracle import attention_ref as ar

pytestmark = pytest.mark.gpu

DIM_HEADS = (64, 128, 192, 384)
BASE_N = (1, 2, 63, 64, 65, 300, 1024)
EDGE_N = (127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048)   # splits 1 | 2 | 4 | 8 | 16 | 32 at both (B, heads) below
BATCH_HEADS = ((1, 1), (3, 2))
KINDS = ("diffuse", "perm2")
SPARE = 5                                                          # slots beyond n, NaN-filled


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=4)
def _case(kind, B, heads, d, n):
    """(q row [B, heads*d] bf16, K and V caches [B, heads, n + SPARE, d] bf16 with NaN beyond n, float64 out [B, heads*d], bound): computed
    on the CPU, never modified (each grid point belongs to one test: only the last few are kept)."""
    q, k, v = ar.make_inputs(kind, B, n, heads, d, seed=1000 * d + n, causal=True)
    scale = d**-0.5
    out, P, _ = ar.attention_f64(q[:, :, n - 1:], k, v, scale)                    # the last row of the causal problem
    bound = ar.forward_bound(P, v, out)
    kc = torch.full((B, heads, n + SPARE, d), float("nan"), dtype=torch.bfloat16)
    vc = kc.clone()
    kc[:, :, :n], vc[:, :, :n] = k.to(torch.bfloat16), v.to(torch.bfloat16)
    row = q[:, :, n - 1].reshape(B, heads * d).to(torch.bfloat16).contiguous()
    return row, kc, vc, out.reshape(B, heads * d), bound.reshape(B, heads * d)


def test_edge_lengths_are_where_the_split_count_changes():
    from tribe_hip import ops

    for B, heads in BATCH_HEADS:
        changes = [n for n in range(2, 4200) if ops.attention_decode_splits(B, heads, n) != ops.attention_decode_splits(B, heads, n - 1)]
        assert sorted(set(EDGE_N)) == sorted(changes + [n - 1 for n in changes]), (B, heads, changes)
        assert ops.attention_decode_splits(B, heads, 10**6) == ops.attention_decode_splits(B, heads, 4200)


@pytest.mark.parametrize("n", sorted(set(BASE_N + EDGE_N)))
@pytest.mark.parametrize("d", DIM_HEADS)
def test_decode_attention_vs_float64(d, n):
    from tribe_hip import ops

    for B, heads in BATCH_HEADS:
        for kind in KINDS:
            row, kc, vc, want, bound = _case(kind, B, heads, d, n)
            q, kc, vc = row.cuda(), kc.cuda(), vc.cuda()
            got = ops.attention_decode(q, kc, vc, n, d**-0.5)
            again = ops.attention_decode(q, kc, vc, n, d**-0.5)
            assert got.shape == (B, heads * d) and got.dtype == torch.bfloat16
            assert torch.equal(_bits(got), _bits(again)), "two identical calls differ"
            worst, where = ar.ratio_report(got.cpu(), want, bound)
            print(f"d={d} n={n} (B, heads)=({B}, {heads}) {kind}: splits {ops.attention_decode_splits(B, heads, n)}, "
                  f"worst |err| / bound {worst:.3f} at {where}")
            assert bool(torch.isfinite(got).all()), "a slot at or beyond n was read (NaN reached the output)"
            assert worst <= 1.0


def test_decode_reads_q_from_a_fused_row():
    """q given as the step's fused [B, 3*inner] buffer (row stride 3*inner) equals q given on its own."""
    from tribe_hip import ops

    B, heads, d, n = 3, 2, 128, 300
    row, kc, vc, *_ = _case("diffuse", B, heads, d, n)
    fused = torch.full((B, 3 * heads * d), float("nan"), dtype=torch.bfloat16)
    fused[:, : heads * d] = row
    a = ops.attention_decode(row.cuda(), kc.cuda(), vc.cuda(), n, d**-0.5)
    b = ops.attention_decode(fused.cuda(), kc.cuda(), vc.cuda(), n, d**-0.5)
    assert torch.equal(_bits(a), _bits(b))


SENTINEL = 0x5A5A


@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "half_split"])
@pytest.mark.parametrize("heads,d,rot", [(2, 64, 32), (3, 384, 192), (2, 128, 0), (1, 192, 96)])
def test_kv_append_matches_the_rotary_pass_bit_for_bit(heads, d, rot, interleaved):
    from tribe_hip import ops

    B, T = 3, 11
    inner = heads * d
    g = torch.Generator().manual_seed(7 * d + rot)
    full = torch.randn(B * T, 3 * inner, generator=g).to(torch.bfloat16).cuda()
    cos, sin = (t.cuda() for t in ar.rotary_tables(T, rot)) if rot else (None, None)
    want = full.clone()
    if rot:
        ops.rotary_(want, T, heads, d, rot, cos, sin, interleaved)
        assert not torch.equal(_bits(want), _bits(full))
    want = want.view(B, T, 3, heads, d)
    kc = torch.full((B, heads, T, d), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    vc = kc.clone()
    order = [4, 0, T - 1, 7]                                                        # any order: a slot depends on its own position only
    for pos in order:
        step = full.view(B, T, 3 * inner)[:, pos].clone()
        out = ops.kv_append(step, kc, vc, pos, rot, cos, sin, interleaved)
        assert out.data_ptr() == step.data_ptr()
        got = step.view(B, 3, heads, d)
        assert torch.equal(_bits(got[:, 0]), _bits(want[:, pos, 0])), "q heads in the buffer"
        assert torch.equal(_bits(got[:, 1]), _bits(want[:, pos, 1])), "k heads in the buffer"
        assert torch.equal(_bits(got[:, 2]), _bits(full.view(B, T, 3, heads, d)[:, pos, 2])), "v heads are left alone"
        assert torch.equal(_bits(kc[:, :, pos]), _bits(want[:, pos, 1])), "slot pos of K"
        assert torch.equal(_bits(vc[:, :, pos]), _bits(want[:, pos, 2])), "slot pos of V"
    rest = [t for t in range(T) if t not in order]
    assert bool((_bits(kc[:, :, rest]) == SENTINEL).all()) and bool((_bits(vc[:, :, rest]) == SENTINEL).all()), "another slot was touched"
