"""Float64 references for the layout, gather and packing kernels (csrc/elementwise.hip, csrc/features.hip and the pool / cast
kernels of csrc/backward.hip).  CPU only: numpy and torch float64, no GPU import.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Every function restates an operation from its definition (a reshape, a sum
over a window, a matrix) and not from the index arithmetic of the kernel it checks; tests/test_layout_host.py pins each of
them to an independent implementation (torch.nn.functional, the transformers classes, float64 autograd), so that a wrong
reference cannot bless a wrong kernel.  tests/test_gpu_layout.py holds the kernels to them.

Two kinds of result:
  * float64 values (im2col, rotary, the conv module, the pools, the means): the test rounds or bounds them itself;
  * float32 values summed in a stated order (piece sums, CSR row sums): the kernels promise that order, so the test is bit-exact.
"""

from __future__ import annotations

import numpy as np
import torch

U_F32 = 2.0**-24      # unit roundoff of f32
U_BF16 = 2.0**-8      # unit roundoff of bf16 (8 significant bits, round to nearest even)


# ------------------------------------------------------------------------------------------------
# bf16 round-to-nearest-even on bit patterns
# ------------------------------------------------------------------------------------------------
def bf16_bits(x) -> np.ndarray:
    """uint16 bf16 patterns of f32 values, round to nearest, ties to even, computed on the bit patterns: bf16 is the upper half of an
    f32, so rounding adds 0x7FFF plus the lowest kept bit and drops the lower half.  The carry may run through the exponent: the
    largest finite f32 becomes inf, which is what round-to-nearest gives.  A NaN keeps its upper half and gets the quiet bit, so
    that a payload held in the lower half alone cannot turn it into inf."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """The f32 value of bf16_bits(x), as a torch tensor of x's shape."""
    bits = bf16_bits(x).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).copy()).reshape(x.shape)


def special_f32_values() -> torch.Tensor:
    """The values a cast has to get right beyond the ordinary ones (32 of them, so that they also fill whole vector chunks): ties
    that round down to even and up to even, the neighbours of a tie, the largest finite f32 (rounds to inf) and the largest
    value that stays finite, +-inf, +-0, f32 subnormals (the largest, the smallest, one that is a tie), the smallest normal, and
    a NaN."""
    bits = [
        0x3F808000, 0x3F818000,              # 1 + 2^-8: tie, down to even;  1 + 3 * 2^-8: tie, up to even
        0x3F808001, 0x3F807FFF,              # just above / below the first tie
        0xBF808000, 0xBF818000,              # the same ties, negative
        0x7F7FFFFF, 0xFF7FFFFF,              # +-FLT_MAX -> +-inf
        0x7F7F7FFF, 0x7F7F8000,              # the largest f32 that stays finite in bf16; the tie above it (up to even = inf)
        0x7F800000, 0xFF800000,              # +-inf
        0x00000000, 0x80000000,              # +-0
        0x007FFFFF, 0x00000001, 0x80000001,  # subnormals: the largest (rounds up to the smallest normal), the smallest (+-: to +-0)
        0x00018000, 0x00008000, 0x00008001,  # subnormal tie up to even, tie down to even (to 0), just above it
        0x00800000, 0x00010000,              # the smallest normal; a subnormal that bf16 holds exactly
        0x7FC00000,                          # NaN
        0x3F800000, 0xBF800000, 0x40490FDB, 0x3EAAAAAB, 0x42F6E979, 0xC2F6E979, 0x3DCCCCCD, 0x477FE000, 0x33800000,
    ]
    assert len(bits) == 32
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


# ------------------------------------------------------------------------------------------------
# Conv3d(stride == kernel) patch unfold
# ------------------------------------------------------------------------------------------------
def im2col3d(pix: torch.Tensor, tub: int, p: int) -> torch.Tensor:
    """pixels [B, F, C, H, W] -> float64 rows [B * (F/tub) * (H/p) * (W/p), C * tub * p * p], tokens in (frame, row, column) order and
    k = ((c * tub + dt) * p + dy) * p + dx, the flattening of a Conv3d weight [out, C, tub, p, p]."""
    B, F, C, H, W = pix.shape
    x = pix.double().reshape(B, F // tub, tub, C, H // p, p, W // p, p)
    #            b  ft  gy  gx  c  dt  dy  dx
    x = x.permute(0, 1, 4, 6, 3, 2, 5, 7)
    return x.reshape(B * (F // tub) * (H // p) * (W // p), C * tub * p * p)


# ------------------------------------------------------------------------------------------------
# rotary embedding on the q and k heads of a fused buffer
# ------------------------------------------------------------------------------------------------
def rotary(x: torch.Tensor, T: int, n_heads: int, dim_head: int, rot_dim: int, cos: torch.Tensor, sin: torch.Tensor,
           mode: int) -> torch.Tensor:
    """x [rows, width >= n_heads * dim_head] -> float64 of the same shape: the first rot_dim elements of each of the first n_heads
    heads are rotated by the angles of position row % T, everything else is copied.  A rotation acts on a pair (a, b) of elements:
        a' = a cos_a - b sin_a,   b' = b cos_b + a sin_b.
    mode 0: pairs (j, j + rot_dim/2), tables [T, rot_dim/2], both elements use column j       (x-transformers, half split);
    mode 1: pairs (2j, 2j + 1),       tables [T, rot_dim/2], both elements use column j       (interleaved);
    mode 2: pairs (2j, 2j + 1),       tables [T, rot_dim],   every element uses its own column (V-JEPA2, whose frequencies are
            tiled across a segment while the pairs are adjacent, so the two angles of a pair differ)."""
    rows = x.shape[0]
    half = rot_dim // 2
    j = torch.arange(half)
    if mode == 0:
        ia, ib, ca, cb = j, j + half, j, j
    elif mode == 1:
        ia, ib, ca, cb = 2 * j, 2 * j + 1, j, j
    elif mode == 2:
        ia, ib, ca, cb = 2 * j, 2 * j + 1, 2 * j, 2 * j + 1
    else:
        raise ValueError(f"rotary: mode {mode}")
    want_cols = rot_dim if mode == 2 else half
    if cos.shape != (T, want_cols) or sin.shape != cos.shape:
        raise ValueError(f"rotary: mode {mode} takes tables [{T}, {want_cols}], got {tuple(cos.shape)}")
    pos = torch.arange(rows) % T
    c, s = cos.double()[pos], sin.double()[pos]                 # [rows, cols]
    out = x.double().clone()
    heads = out[:, : n_heads * dim_head].view(rows, n_heads, dim_head)       # a view: writes land in out
    a, b = heads[:, :, ia].clone(), heads[:, :, ib].clone()
    heads[:, :, ia] = a * c[:, None, ca] - b * s[:, None, ca]
    heads[:, :, ib] = b * c[:, None, cb] + a * s[:, None, cb]
    return out


# ------------------------------------------------------------------------------------------------
# causal depthwise conv + LayerNorm + SiLU (Wav2Vec2BertConvolutionModule's middle)
# ------------------------------------------------------------------------------------------------
def dwconv_ln_swish(x: torch.Tensor, w_kc: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float):
    """x [B, T, C], taps w_kc [K, C] (tap k joins input t - (K - 1) + k to output t; inputs before 0 are zero).  Returns float64
    (y, conv, abs_conv, rstd): the module's output, the conv sums, the sums of the magnitudes of their terms (what an f32
    accumulation errs in proportion to) and the LayerNorm's 1 / sqrt(var + eps) per row [B, T, 1]."""
    B, T, C = x.shape
    K = w_kc.shape[0]
    x64, w64 = x.double(), w_kc.double()
    conv = torch.zeros(B, T, C, dtype=torch.float64)
    mag = torch.zeros(B, T, C, dtype=torch.float64)
    for k in range(K):
        shift = K - 1 - k                                       # output t takes input t - shift
        if shift >= T:
            continue
        term = x64[:, : T - shift] * w64[k]
        conv[:, shift:] += term
        mag[:, shift:] += term.abs()
    mean = conv.mean(-1, keepdim=True)
    rstd = ((conv - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    v = (conv - mean) * rstd * ln_w.double() + ln_b.double()
    return v / (1.0 + torch.exp(-v)), conv, mag, rstd


# ------------------------------------------------------------------------------------------------
# adaptive average pool along the last axis, and its adjoint
# ------------------------------------------------------------------------------------------------
def adaptive_pool_matrix(T_in: int, T_out: int) -> torch.Tensor:
    """P float64 [T_out, T_in]: row i averages the inputs floor(i T_in / T_out) .. ceil((i + 1) T_in / T_out) - 1 (windows overlap
    when T_in is no multiple of T_out and repeat inputs when T_out > T_in).  pool(x) = x P^T; its adjoint is dy P."""
    P = torch.zeros(T_out, T_in, dtype=torch.float64)
    for i in range(T_out):
        a = (i * T_in) // T_out
        b = -((-(i + 1) * T_in) // T_out)
        P[i, a:b] = 1.0 / (b - a)
    return P


def adaptive_avg_pool(x: torch.Tensor, T_out: int) -> torch.Tensor:
    return x.double() @ adaptive_pool_matrix(x.shape[-1], T_out).t()


def adaptive_avg_pool_adjoint(dy: torch.Tensor, T_in: int) -> torch.Tensor:
    return dy.double() @ adaptive_pool_matrix(T_in, dy.shape[-1])


# ------------------------------------------------------------------------------------------------
# means over windows of time / over groups of layers
# ------------------------------------------------------------------------------------------------
def _window(start: int, length: int, T: int) -> tuple[int, int]:
    """[start, start + length) intersected with [0, T): a window that begins before 0 or ends after T is CUT, never moved."""
    lo, hi = max(int(start), 0), min(int(start) + int(length), T)
    return lo, max(hi, lo)


def segment_mean(x: torch.Tensor, start, length) -> torch.Tensor:
    """x [B, T, dim] -> float64 [B, dim]: the mean over the window of each sequence; an empty window gives zeros.  start / length
    None: the whole sequence."""
    B, T, dim = x.shape
    out = torch.zeros(B, dim, dtype=torch.float64)
    for b in range(B):
        lo, hi = _window(0 if start is None else start[b], T if length is None else length[b], T)
        if hi > lo:
            out[b] = x[b, lo:hi].double().mean(0)
    return out


def window_mean(x: torch.Tensor, win_row, win_start, win_len) -> torch.Tensor:
    """x [B, T, dim] -> float64 [W, dim]: window w averages its rows of sequence win_row[w]; an empty window or a sequence outside
    [0, B) gives zeros."""
    B, T, dim = x.shape
    out = torch.zeros(len(win_row), dim, dtype=torch.float64)
    for w, (b, s, n) in enumerate(zip(win_row, win_start, win_len)):
        lo, hi = _window(s, n, T)
        if 0 <= int(b) < B and hi > lo:
            out[w] = x[int(b), lo:hi].double().mean(0)
    return out


def group_mean(states: torch.Tensor, lo, hi) -> torch.Tensor:
    """states [batch, n_states, ...] -> float64 [batch, n_groups, ...]: group g is the mean of states lo[g] .. hi[g] - 1."""
    return torch.stack([states[:, int(a):int(b)].double().mean(1) for a, b in zip(lo, hi)], dim=1)


# ------------------------------------------------------------------------------------------------
# gathers
# ------------------------------------------------------------------------------------------------
def gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x [B, T, dim], idx [n] -> x[:, clamp(idx, 0, T - 1)] (the nearest-neighbour resample along time)."""
    return x[:, idx.clamp(0, x.shape[1] - 1)]


def embedding(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """table [vocab, dim] (any float type), ids of any shape -> f32 [ids.numel(), dim]; ids are clamped into the table."""
    return table[ids.flatten().clamp(0, table.shape[0] - 1)].float()


# ------------------------------------------------------------------------------------------------
# f32 sums in a stated order
# ------------------------------------------------------------------------------------------------
def piece_sum(pieces, B: int, C: int, T: int) -> np.ndarray:
    """Assembly of segment outputs from time slices of cached arrays.  pieces: a list, in order, of
    (segment, src f32 [C, n], src_first, src_count, dst_first, dst_count): steps dst_first .. dst_first + dst_count - 1 of the
    segment receive columns src_first .. of src (src_count == dst_count), or column src_first alone at every step (src_count == 1,
    a broadcast).  Steps outside [0, T) are dropped.  f32 [B, C, T], every cell summed from 0 in the order of the list
    (`out += piece`)."""
    out = np.zeros((B, C, T), dtype=np.float32)
    for seg, src, src_first, src_count, dst_first, dst_count in pieces:
        src = np.asarray(src, dtype=np.float32)
        for i in range(dst_count):
            t = dst_first + i
            if 0 <= t < T:
                col = src[:, src_first + (0 if src_count == 1 else i)]
                out[seg, :, t] = out[seg, :, t] + col
    return out


def csr_row_sums(table: torch.Tensor, row_ptr, word_idx) -> np.ndarray:
    """table f32 [n_words, C]; row r sums the table rows word_idx[row_ptr[r] : row_ptr[r + 1]] from 0 in list order.  f32 [rows, C]."""
    tab = table.detach().cpu().numpy().astype(np.float32)
    rows = len(row_ptr) - 1
    out = np.zeros((rows, tab.shape[1]), dtype=np.float32)
    for r in range(rows):
        for w in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            out[r] = out[r] + tab[int(word_idx[w])]
    return out


# ------------------------------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests (the CPU test measures on them what the GPU test then asserts)
# ------------------------------------------------------------------------------------------------
def layer_features(B: int, L: int, D: int, T: int, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """[B, L, D, T] extractor states: N(0, 1) at scales from 1e-2 to 1e2 across d, feature rows 1-2 at 1e3 + N(0, 1) in every
    layer (a mean of nearly equal large numbers), row 0 all zero; rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, D, T, generator=g, dtype=torch.float64) * torch.logspace(-2, 2, D, dtype=torch.float64)[None, None, :, None]
    x[:, :, 1:3] = 1e3 + torch.randn(B, L, min(D, 3) - 1, T, generator=g, dtype=torch.float64)
    x[:, :, 0] = 0
    return x.to(dtype)


def layer_mean_f32(feat: torch.Tensor) -> torch.Tensor:
    """What an f32 kernel makes of the layer mean: every state converted to f32, summed from 0 in layer order, times f32(1 / L).
    [B, L, D, T] -> f32 [B, D, T]."""
    L = feat.shape[1]
    acc = torch.zeros(feat.shape[0], *feat.shape[2:], dtype=torch.float32)
    for l in range(L):
        acc = acc + feat[:, l].float()
    return acc * torch.tensor(1.0 / L, dtype=torch.float32)


# the smallest share of bf16(dwconv_ln_swish_f32) == bf16(float64 value) over CONV_SHAPES with conv_case(B, T, C, K, seed=C + K), as
# tests/test_layout_host.py::test_conv_module_f32_share measures it (and fails if it drops); tests/test_gpu_layout.py asserts it
# less one percentage point
CONV_SHAPES = [(2, 19, 128, 31), (1, 7, 1024, 5), (1, 40, 256, 33), (1, 12, 2048, 31), (1, 9, 1028, 3)]
MEASURED_CONV_SHARE = 0.9999


def conv_case(B: int, T: int, C: int, K: int, seed: int):
    """Inputs of the conv module: x [B, T, C] bf16-exact N(0, 1) with every 16th channel at 1e2 + N(0, 1) (their conv sums are far
    from the row mean, so the mean subtraction matters) and time step 3 of sequence 0 all zero; taps N(0, 1) / sqrt(K);
    LayerNorm weight in [0.5, 1.5) and bias 0.1 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g)
    x[:, :, ::16] = 1e2 + torch.randn(B, T, len(range(0, C, 16)), generator=g)
    x[0, min(3, T - 1)] = 0
    x = x.to(torch.bfloat16).float()
    w = torch.randn(K, C, generator=g) / K**0.5
    ln_w = torch.rand(C, generator=g) + 0.5
    ln_b = 0.1 * torch.randn(C, generator=g)
    return x, w, ln_w, ln_b


def dwconv_ln_swish_f32(x: torch.Tensor, w_kc: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float) -> torch.Tensor:
    """The conv module's formula in plain f32 (products and sums rounded one by one, taps in order): what a correct f32 kernel
    computes, up to the order of its sums.  Used to MEASURE how often bf16(f32 result) equals bf16(float64 result)."""
    B, T, C = x.shape
    K = w_kc.shape[0]
    conv = torch.zeros(B, T, C, dtype=torch.float32)
    for k in range(K):
        shift = K - 1 - k
        if shift < T:
            conv[:, shift:] += x[:, : T - shift] * w_kc[k]
    mean = conv.sum(-1, keepdim=True) / C
    d = conv - mean
    rstd = ((d * d).sum(-1, keepdim=True) / C + torch.tensor(eps, dtype=torch.float32)).rsqrt()
    v = d * rstd * ln_w + ln_b
    return v / (1.0 + torch.exp(-v))
