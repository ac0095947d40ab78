"""The grid of the block-append attention (tribe_attention_extend_fwd), shared by tests/test_extend_host.py (CPU: what the grid can detect)
and tests/test_gpu_extend_attention.py (GPU: the kernel on it).

A grid point is a causal problem of length Tk = pos + k of which the kernel computes the last k rows: query t of the block (position
pos + t) sees keys j <= pos + t.  (pos, k) are the smallest shapes at which the kernel can go wrong: one row; a ragged wave; a full wave
plus one; a block that crosses a 32-key sub-tile; one that crosses the 128-row query block; two query blocks; many key tiles."""

import functools

from oracle import attention_ref as ar

DIM_HEADS = (64, 128, 192, 384)
POS_K = ((0, 1), (0, 33), (5, 1), (5, 16), (5, 17), (31, 2), (32, 32), (100, 29), (127, 129), (300, 200), (1000, 24))
BATCH_HEADS = ((1, 1), (3, 2))


@functools.lru_cache(maxsize=8)
def problem(kind, B, heads, d, pos, k):
    """(q, k, v [B, heads, pos + k, d] bf16-exact f32, scale, float64 out / P of rows pos .., forward bound of those rows): computed once on
    the CPU, never modified."""
    q, kk, v = ar.make_inputs(kind, B, pos + k, heads, d, seed=1000 * d + 7 * pos + k, causal=True)
    scale = d**-0.5
    out, P, _ = ar.attention_f64(q, kk, v, scale, causal=True)
    out, P = out[:, :, pos:], P[:, :, pos:]
    return q, kk, v, scale, out, P, ar.forward_bound(P, v, out)
