"""GPU: the block-append kernels of streamed causal encoders.

tribe_attention_extend_fwd (csrc/attention.hip, attn_fwd_kernel<.., EXTEND = 1>), element by element against
oracle.attention_ref.attention_f64 on the causal problem of length pos + k, rows pos ..: query t of the block sees keys j <= pos + t.
Bound: the project's derived forward bound, ar.forward_bound = 2^-8 (P |v|) + 2^-7 |out64| + 1e-6, on ALL elements, ratio <= 1.  Grid
(tests/extend_cases.py): every head size; (pos, k) from one row to many key tiles; (B, heads) = (1, 1), (3, 2); inputs `diffuse` and `perm2`.
tests/test_extend_host.py shows on the CPU what this grid detects: each of five wrong masks leaves the bound by >= 3x on the diffuse
inputs.  The caches have cap = pos + k + 5 and every slot >= pos + k holds bf16 NaN: a finite result shows nothing beyond is read.  Two
identical calls give equal bits.

tribe_kv_append_block, bit for bit against ops.rotary_ on a full-length buffer, both pairings and rot_dim = 0; slots outside [pos, pos + k)
stay untouched."""

import pytest
import torch

from oracle import attention_ref as ar
from tests.extend_cases import BATCH_HEADS, DIM_HEADS, POS_K, problem

pytestmark = pytest.mark.gpu

KINDS = ("diffuse", "perm2")
SPARE = 5                                                          # slots beyond pos + k, NaN-filled


def _bits(t):
    return t.contiguous().view(torch.int16)


def _device_case(kind, B, heads, d, pos, k):
    """(q rows [B*k, heads*d] bf16, K and V caches [B, heads, pos + k + SPARE, d] bf16 with NaN beyond pos + k) on the CPU."""
    q, kk, v, *_ = problem(kind, B, heads, d, pos, k)
    Tk = pos + k
    kc = torch.full((B, heads, Tk + SPARE, d), float("nan"), dtype=torch.bfloat16)
    vc = kc.clone()
    kc[:, :, :Tk], vc[:, :, :Tk] = kk.to(torch.bfloat16), v.to(torch.bfloat16)
    rows = q[:, :, pos:].transpose(1, 2).reshape(B * k, heads * d).to(torch.bfloat16).contiguous()
    return rows, kc, vc


@pytest.mark.parametrize("pos,k", POS_K)
@pytest.mark.parametrize("d", DIM_HEADS)
def test_extend_attention_vs_float64(d, pos, k):
    from tribe_hip import ops

    for B, heads in BATCH_HEADS:
        for kind in KINDS:
            *_, scale, want, _, bound = problem(kind, B, heads, d, pos, k)
            rows, kc, vc = (t.cuda() for t in _device_case(kind, B, heads, d, pos, k))
            got = ops.attention_extend(rows, kc, vc, pos, k, scale)
            again = ops.attention_extend(rows, kc, vc, pos, k, scale)
            assert got.shape == (B * k, heads * d) and got.dtype == torch.bfloat16
            assert torch.equal(_bits(got), _bits(again)), "two identical calls differ"
            out = got.cpu().view(B, k, heads, d).transpose(1, 2)
            worst, where = ar.ratio_report(out, want, bound)
            print(f"d={d} (pos, k)=({pos}, {k}) (B, heads)=({B}, {heads}) {kind}: worst |err| / bound {worst:.3f} at {where}")
            assert bool(torch.isfinite(got).all()), "a slot at or beyond pos + k was read (NaN reached the output)"
            assert worst <= 1.0


def test_extend_reads_q_from_the_fused_rows():
    """q given as the block's fused [B*k, 3*inner] buffer (row stride 3*inner) equals q given on its own."""
    from tribe_hip import ops

    B, heads, d, pos, k = 3, 2, 128, 100, 29
    rows, kc, vc = _device_case("diffuse", B, heads, d, pos, k)
    fused = torch.full((B * k, 3 * heads * d), float("nan"), dtype=torch.bfloat16)
    fused[:, : heads * d] = rows
    a = ops.attention_extend(rows.cuda(), kc.cuda(), vc.cuda(), pos, k, d**-0.5)
    b = ops.attention_extend(fused.cuda(), kc.cuda(), vc.cuda(), pos, k, d**-0.5)
    assert torch.equal(_bits(a), _bits(b))


def test_one_row_block_agrees_with_the_decode_kernel_within_the_bound():
    """k = 1 is the decode problem: both kernels sit within the same bound of the same float64 rows."""
    from tribe_hip import ops

    B, heads, d, pos = 3, 2, 192, 31
    *_, scale, want, _, bound = problem("diffuse", B, heads, d, pos, 2)
    rows, kc, vc = (t.cuda() for t in _device_case("diffuse", B, heads, d, pos, 2))
    first = rows.view(B, 2, heads * d)[:, 0].contiguous()
    block = ops.attention_extend(first, kc, vc, pos, 1, scale).cpu().view(B, 1, heads, d).transpose(1, 2)
    decode = ops.attention_decode(first, kc, vc, pos + 1, scale).cpu().view(B, 1, heads, d).transpose(1, 2)
    assert ar.ratio_report(block, want[:, :, :1], bound[:, :, :1])[0] <= 1.0
    assert ar.ratio_report(decode, want[:, :, :1], bound[:, :, :1])[0] <= 1.0


SENTINEL = 0x5A5A


@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "half_split"])
@pytest.mark.parametrize("heads,d,rot", [(2, 64, 32), (3, 384, 192), (2, 128, 0), (1, 192, 96)])
def test_kv_append_block_matches_the_rotary_pass_bit_for_bit(heads, d, rot, interleaved):
    from tribe_hip import ops

    B, T = 3, 23
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
    blocks = [(9, 5), (0, 1), (17, 6), (3, 2)]                                        # (pos, k), any order; 17 + 6 = T: the last slot
    for pos, k in blocks:
        block = full.view(B, T, 3 * inner)[:, pos:pos + k].reshape(B * k, 3 * inner).clone()
        out = ops.kv_append_block(block, kc, vc, pos, k, rot, cos, sin, interleaved)
        assert out.data_ptr() == block.data_ptr()
        got = block.view(B, k, 3, heads, d)
        assert torch.equal(_bits(got[:, :, 0]), _bits(want[:, pos:pos + k, 0])), "q heads in the buffer"
        assert torch.equal(_bits(got[:, :, 1]), _bits(want[:, pos:pos + k, 1])), "k heads in the buffer"
        assert torch.equal(_bits(got[:, :, 2]), _bits(full.view(B, T, 3, heads, d)[:, pos:pos + k, 2])), "v heads are left alone"
        assert torch.equal(_bits(kc[:, :, pos:pos + k]), _bits(want[:, pos:pos + k, 1].transpose(1, 2))), "slots pos .. of K"
        assert torch.equal(_bits(vc[:, :, pos:pos + k]), _bits(want[:, pos:pos + k, 2].transpose(1, 2))), "slots pos .. of V"
    seen = {t for pos, k in blocks for t in range(pos, pos + k)}
    rest = [t for t in range(T) if t not in seen]
    assert rest and bool((_bits(kc[:, :, rest]) == SENTINEL).all()) and bool((_bits(vc[:, :, rest]) == SENTINEL).all()), "another slot was touched"
