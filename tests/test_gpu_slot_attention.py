"""GPU: the slot forms of the KV cache kernels -- every sequence of a cache at a position of its own (csrc/attn_decode.hip:
tribe_kv_append_slots, tribe_attention_decode_slots_fwd; csrc/attention.hip: tribe_attention_extend_slots_fwd, attn_fwd_kernel<.., EXTEND = 2>).

Append: bit for bit against ops.kv_append_block run on each sequence alone, both pairings and rot_dim = 0; every other slot of the
sentinel-filled caches stays untouched; a sequence at -1, or at the out-of-range value cap (given to the C entry point directly: the ops
wrapper refuses it on the host), keeps its cache run and its qkv rows bit for bit.

Decode: (B, heads) = (3, 2), each sequence with its own key count n_b <= n_max, element by element against oracle.attention_ref.attention_f64
of the last row of ITS causal problem of length n_b, within the project's derived bound ar.forward_bound (the parts are f32: nothing new
enters).  The chunk is computed here from the stated rule (the split count of tribe_attention_decode_fwd at n = n_max) and the lengths sit on
and either side of its edges; a length the rule puts beyond n_max is clamped to n_max.  Slots at and beyond n_b hold bf16 NaN: a finite
result shows they are not read.  An inactive row is exactly zero.  Two calls give equal bits; all lengths equal to n_max give
ops.attention_decode's bits.

Extend: (B, heads) = (3, 2), the ragged-wave, sub-tile and query-block crossings of tests/extend_cases.POS_K as position triples with one k
per call; each sequence within ar.forward_bound of its own rectangular float64 problem and bit-equal to ops.attention_extend run on that
sequence alone; NaN beyond pos_b + k; inactive rows zero."""

import functools

import pytest
import torch

from oracle import attention_ref as ar
from tests.extend_cases import DIM_HEADS, POS_K, problem

pytestmark = pytest.mark.gpu

B, HEADS = 3, 2
KINDS = ("diffuse", "perm2")
SPARE = 5
SENTINEL = 0x5A5A
OFF = None                                                                            # a sequence that takes no part


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- append -----------------------------------------------------------------------------------------------------------------------------
def _append_alone(ops, block, pos, k, heads, d, rot, cos, sin, interleaved, cap):
    """ops.kv_append_block on one sequence's rows in sentinel-filled caches of its own: (rows, K run, V run)."""
    rows = block.clone()
    kc = torch.full((1, heads, cap, d), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    vc = kc.clone()
    ops.kv_append_block(rows, kc, vc, pos, k, rot, cos, sin, interleaved)
    return rows, kc[0], vc[0]


@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "half_split"])
@pytest.mark.parametrize("heads,d,rot", [(2, 64, 32), (3, 384, 192), (2, 128, 0), (1, 192, 96)])
def test_kv_append_slots_matches_the_block_append_of_each_sequence(heads, d, rot, interleaved):
    from tribe_hip import _lib, ops

    cap, inner = 11, heads * d
    cos, sin = (t.cuda() for t in ar.rotary_tables(cap, rot)) if rot else (None, None)
    g = torch.Generator().manual_seed(7 * d + rot)
    for k, positions in ((1, (0, 7, 10)), (5, (0, 3, 6)), (1, (4, -1, 2)), (5, (4, -1, 2)), (1, (4, cap, 2)), (5, (4, cap, 2)),
                         (5, (4, cap - 4, 2))):
        block = torch.randn(B * k, 3 * inner, generator=g).to(torch.bfloat16).cuda()
        kc = torch.full((B, heads, cap, d), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        vc = kc.clone()
        got = block.clone()
        in_range = [0 <= p <= cap - k for p in positions]
        if all(p == -1 or ok for p, ok in zip(positions, in_range)):
            out = ops.kv_append_slots(got, kc, vc, list(positions), k, rot, cos, sin, interleaved)
            assert out.data_ptr() == got.data_ptr()
        else:   # an out-of-range position: the wrapper refuses it on the host, the kernel must treat it as inactive
            with pytest.raises(ValueError, match="tribe_kv_append_slots: pos"):
                ops.kv_append_slots(got, kc, vc, list(positions), k, rot, cos, sin, interleaved)
            dpos = torch.tensor(positions, dtype=torch.int32, device="cuda")
            _lib.check(_lib.lib().tribe_kv_append_slots(got.data_ptr(), B, k, heads, d, rot, int(interleaved), cos.data_ptr() if rot else None,
                                                        sin.data_ptr() if rot else None, dpos.data_ptr(), kc.data_ptr(), vc.data_ptr(), cap,
                                                        ops._stream()), "tribe_kv_append_slots")
        if rot:
            assert not torch.equal(_bits(got), _bits(block)), "nothing was rotated"
        for b, p in enumerate(positions):
            rows_b = slice(b * k, (b + 1) * k)
            if in_range[b]:
                want_rows, want_k, want_v = _append_alone(ops, block[rows_b], p, k, heads, d, rot, cos, sin, interleaved, cap)
                written = list(range(p, p + k))
            else:
                want_rows, want_k, want_v = block[rows_b], None, None
                written = []
            assert torch.equal(_bits(got[rows_b]), _bits(want_rows)), (k, positions, b, "qkv rows")
            if written:
                assert torch.equal(_bits(kc[b]), _bits(want_k)) and torch.equal(_bits(vc[b]), _bits(want_v)), (k, positions, b, "cache run")
                assert bool((_bits(kc[b, :, written]) != SENTINEL).any()), (k, positions, b, "the slots were not written")
            rest = [t for t in range(cap) if t not in written]
            assert bool((_bits(kc[b][:, rest]) == SENTINEL).all()) and bool((_bits(vc[b][:, rest]) == SENTINEL).all()), \
                (k, positions, b, "another slot was touched")


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
def _stated_chunk(n_max):
    """The split count and chunk of tribe_attention_decode_fwd at n = n_max, from the documented rule: a power of two of workgroups per
    (b, h), enough for 256 in all, at most 32, each split at least 64 keys; the chunk is ceil(n / splits) rounded up to 8."""
    want = 1
    while want < 32 and B * HEADS * want < 256:
        want *= 2
    splits = 1
    while splits * 2 <= want and splits * 2 * 64 <= n_max:
        splits *= 2
    return splits, (-(-n_max // splits) + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def _decode_row(kind, d, n):
    """One sequence of length n: (q row [HEADS*d] bf16, k, v [HEADS, n, d] bf16, float64 out [HEADS*d], bound) -- CPU, never modified."""
    q, k, v = ar.make_inputs(kind, 1, n, HEADS, d, seed=1000 * d + n, causal=True)
    out, P, _ = ar.attention_f64(q[:, :, n - 1:], k, v, d**-0.5)
    bound = ar.forward_bound(P, v, out)
    return (q[0, :, n - 1].reshape(HEADS * d).to(torch.bfloat16), k[0].to(torch.bfloat16), v[0].to(torch.bfloat16), out.reshape(HEADS * d),
            bound.reshape(HEADS * d))


def _decode_case(kind, d, lengths, cap):
    q = torch.randn(B, HEADS * d, generator=torch.Generator().manual_seed(d)).to(torch.bfloat16)
    kc = torch.full((B, HEADS, cap, d), float("nan"), dtype=torch.bfloat16)
    vc = kc.clone()
    want = []
    for b, n in enumerate(lengths):
        if n is OFF:
            want.append(None)
            continue
        row, k, v, out, bound = _decode_row(kind, d, n)
        q[b], kc[b, :, :n], vc[b, :, :n] = row, k, v
        want.append((out, bound))
    return q.cuda(), kc.cuda(), vc.cuda(), want


@pytest.mark.parametrize("n_max", (65, 300, 1024))
@pytest.mark.parametrize("d", DIM_HEADS)
def test_decode_slots_vs_float64_of_each_sequence(d, n_max):
    from tribe_hip import ops

    splits, chunk = _stated_chunk(n_max)
    assert splits == ops.attention_decode_splits(B, HEADS, n_max)
    clamp = lambda n: max(1, min(n, n_max))                                            # noqa: E731
    triples = [(1, clamp(chunk), n_max), (clamp(chunk - 1), clamp(chunk + 1), n_max - 1), (n_max, 2, min(2 * chunk, n_max)),
               (clamp(chunk + 1), OFF, n_max), (OFF, OFF, 3), (n_max, n_max, n_max)]
    cap, scale = n_max + SPARE, d**-0.5
    for lengths in triples:
        for kind in KINDS:
            q, kc, vc, want = _decode_case(kind, d, lengths, cap)
            pos = [-1 if n is OFF else n - 1 for n in lengths]
            got = ops.attention_decode_slots(q, kc, vc, pos, n_max, scale)
            again = ops.attention_decode_slots(q, kc, vc, pos, n_max, scale)
            assert got.shape == (B, HEADS * d) and got.dtype == torch.bfloat16
            assert torch.equal(_bits(got), _bits(again)), "two identical calls differ"
            assert bool(torch.isfinite(got).all()), (lengths, kind, "a slot at or beyond n_b was read (NaN reached the output)")
            for b, n in enumerate(lengths):
                if n is OFF:
                    assert bool((_bits(got[b]) == 0).all()), (lengths, kind, b, "the row of an inactive sequence is not +0")
                    continue
                worst, where = ar.ratio_report(got[b].cpu(), *want[b])
                print(f"d={d} n_max={n_max} splits={splits} chunk={chunk} lengths={lengths} {kind} sequence {b}: worst |err| / bound "
                      f"{worst:.3f} at {where}")
                assert worst <= 1.0, (lengths, kind, b, worst)
            if all(n == n_max for n in lengths):
                same = ops.attention_decode(q, kc, vc, n_max, scale)
                assert torch.equal(_bits(got), _bits(same)), "equal positions: not the bits of tribe_attention_decode_fwd"


@pytest.mark.parametrize("n_max", (256, 1024))
@pytest.mark.parametrize("d", DIM_HEADS)
def test_decode_slots_gives_the_bits_of_decode_at_the_encoders_shapes(d, n_max):
    """(B, heads) = (16, 8): 128 (sequence, head) pairs, two splits with chunks of 128 / 512 keys -- the grid a streamed encoder runs, where
    the four-wave merge and the combine kernel carry whole chunks.  2048 rows x d outputs: a product rounded differently in either form
    flips bf16 results here (at (3, 2) too few rows see it).  Also (2, 2) at the same lengths: 32 splits."""
    from tribe_hip import ops

    for nb, heads in ((16, 8), (2, 2)):
        g = torch.Generator().manual_seed(d + n_max + nb)
        q = torch.randn(nb, heads * d, generator=g).to(torch.bfloat16).cuda()
        kc = torch.randn(nb, heads, n_max + SPARE, d, generator=g).to(torch.bfloat16).cuda()
        vc = torch.randn(nb, heads, n_max + SPARE, d, generator=g).to(torch.bfloat16).cuda()
        if nb == 16:
            assert ops.attention_decode_splits(nb, heads, n_max) == 2
        want = ops.attention_decode(q, kc, vc, n_max, d**-0.5)
        got = ops.attention_decode_slots(q, kc, vc, [n_max - 1] * nb, n_max, d**-0.5)
        differ = int((_bits(got) != _bits(want)).sum())
        print(f"d={d} n_max={n_max} (B, heads)=({nb}, {heads}): {differ} of {got.numel()} outputs differ from tribe_attention_decode_fwd")
        assert differ == 0


# ---- extend -----------------------------------------------------------------------------------------------------------------------------
EXTEND_CAP = 448
POS_TRIPLES = ((0, 5, 31), (127, 0, 300), (100, -1, 32))
BLOCKS = (1, 16, 17, 129)


@pytest.mark.parametrize("k", BLOCKS)
@pytest.mark.parametrize("d", DIM_HEADS)
def test_extend_slots_vs_float64_and_the_block_append_of_each_sequence(d, k):
    from tribe_hip import ops

    # the triples and block lengths are tests/extend_cases.POS_K's crossings (one row at 0 and 5; a full and a ragged wave at 5; a block across a
    # 32-key sub-tile at 31 and from a sub-tile's first key; across the 128-row query block from 127; many tiles), and all fit the cap
    assert {0, 5, 31, 127, 300, 100, 32} <= {p for p, _ in POS_K} and set(BLOCKS) <= {kk for _, kk in POS_K}
    assert all(p + kk <= EXTEND_CAP for t in POS_TRIPLES for p in t for kk in BLOCKS)
    scale = d**-0.5
    for positions in POS_TRIPLES:
        if any(p + k > EXTEND_CAP for p in positions):
            continue
        for kind in KINDS:
            rows = torch.randn(B, k, HEADS * d, generator=torch.Generator().manual_seed(d + k)).to(torch.bfloat16)
            kc = torch.full((B, HEADS, EXTEND_CAP, d), float("nan"), dtype=torch.bfloat16)
            vc = kc.clone()
            want = []
            for b, p in enumerate(positions):
                if p < 0:
                    want.append(None)
                    continue
                q, kk, v, _, out, _, bound = problem(kind, 1, HEADS, d, p, k)
                rows[b] = q[0, :, p:].transpose(0, 1).reshape(k, HEADS * d).to(torch.bfloat16)
                kc[b, :, : p + k], vc[b, :, : p + k] = kk[0].to(torch.bfloat16), v[0].to(torch.bfloat16)
                want.append((out[0], bound[0]))
            rows, kc, vc = rows.view(B * k, HEADS * d).cuda(), kc.cuda(), vc.cuda()
            got = ops.attention_extend_slots(rows, kc, vc, list(positions), k, scale)
            again = ops.attention_extend_slots(rows, kc, vc, list(positions), k, scale)
            assert got.shape == (B * k, HEADS * d) and got.dtype == torch.bfloat16
            assert torch.equal(_bits(got), _bits(again)), "two identical calls differ"
            assert bool(torch.isfinite(got).all()), (positions, kind, "a slot at or beyond pos_b + k was read (NaN reached the output)")
            got = got.view(B, k, HEADS * d)
            for b, p in enumerate(positions):
                if p < 0:
                    assert bool((_bits(got[b]) == 0).all()), (positions, kind, b, "the rows of an inactive sequence are not zero")
                    continue
                out = got[b].cpu().view(k, HEADS, d).transpose(0, 1)
                worst, where = ar.ratio_report(out, *want[b])
                print(f"d={d} k={k} positions={positions} {kind} sequence {b}: worst |err| / bound {worst:.3f} at {where}")
                assert worst <= 1.0, (positions, kind, b, worst)
                alone = ops.attention_extend(rows.view(B, k, HEADS * d)[b].contiguous(), kc[b:b + 1].contiguous(), vc[b:b + 1].contiguous(), p, k,
                                             scale)
                assert torch.equal(_bits(got[b]), _bits(alone)), (positions, kind, b, "not the bits of tribe_attention_extend_fwd on this sequence")
