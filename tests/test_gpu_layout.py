"""GPU: the layout, gather and packing kernels between the GEMMs (csrc/elementwise.hip, csrc/features.hip, the pool / scale / cast
kernels of csrc/backward.hip) per element against the float64 references of oracle/layout_ref.py, on every branch their launchers
pick.  Entry points without an ops wrapper are called through `_call`; wherever the test calls the C ABI itself it owns the output
buffer and fills it with NaN first, so a pad column or a row the kernel skipped shows.

Branches and the parameters that reach them (grid_for caps a grid at 2048 workgroups of 256: "beyond the cap" = more than 524 288
work items, so the grid-stride loop makes a second trip):
  pack_weight_kernel        vector chunks: (50, 100) -> (56, 128); unpadded but rows * cols % 32 != 0: (9, 24); a scalar last chunk
                            beside vector chunks in one launch: (7, 20) -> (7, 24); every chunk scalar: the source offset by one
                            float; beyond the cap: (2050, 2056) -> (2050, 2112), 541 200 chunks
  cast_flat_kernel          (33, 64): one ragged span; (4100, 4096): exactly 2050 spans of 8192 (> 2048 workgroups: the span loop's
                            second trip, all spans full); (4101, 4096): 2050.5 spans, so 2051 with a half-full last span that a
                            workgroup meets on its second trip
  cast_bf16_kernel          n = 4 (one lane), 32 (special values), 2112, 4100 * 4096 (beyond the cap)
  transpose_cast_kernel     <float> without a layer sum: pack_subject_weights (3, 70, 45), (1, 64, 128) unpadded, (2, 65, 129) one past
                            a tile both ways; <float / bf16 / double> with a layer mean, <double> without: pack_features, K_pad > K
  transpose_kernel          pack_features 'cat' of f32 / bf16: <., 4> at T = 64, <., 1> at T = 70 and 129 (T % 4 != 0)
  rotary_kernel             interleaved 0 / 1 / 2 x rot_dim in {dim_head, dim_head / 2, 8} x dim_head in {64, 192}, 3 + 2 heads (GQA row
                            stride), rows = 2 * 19 (position = row % T); beyond the cap: 2048 rows x 16 heads x rot_dim 384
  embedding_kernel          <float>, <bf16> x dim in {64, 100, 3}, 21 ids (a partly idle last workgroup), ids -1 and vocab clamped
  gather_rows_kernel        (2, 333, 128, 13), repeats (1, 7, 4, 20), two trips per lane (3, 50, 1408, 1), indices -1 and T clamped
  im2col3d_kernel           H != W; K_pad > K; tubelet 3; the ViT-g geometry (602 112 chunks: beyond the cap)
  dwconv_ln_swish_tile_kernel  (2, 19, 128, 31), (1, 7, 1024, 5): T % 8 != 0, T < K
  dwconv_ln_swish_kernel<1> (1, 40, 256, 33): K > 31; (2, 19, 128, 31) with w_kc offset by one float
  dwconv_ln_swish_kernel<4> (1, 12, 2048, 31), (1, 9, 1028, 3): 257 groups, the second slot live in one lane only
  segment_mean4_kernel      dim 64 and 1408; segment_mean_kernel: dim 30 (dim % 4 != 0); windows: full, interior, past T, empty,
                            start >= T, start -2 with length 5 (cut to 3 rows, not moved); no start / length arrays at all
  adaptive_pool_kernel, pool_bwd_kernel  (298, 100), (14, 5), (64, 64), (100, 7), (5, 14) x rows 37 and 5000; 9000 rows of (64, 64)
                            put the forward beyond the cap as well
  fill_embed_kernel         pos only / subject only / both / neither; 20 x 700 rows beyond the cap
  scale_cols_kernel         (37, 100) with and without the scale vector; (6000, 100) beyond the cap
  segment_gather_packed_kernel / segment_gather_rows_kernel  (3, 70, 130), C_pad 128 and 72: a piece over steps 60..69 (the 64-step
                            tile edge), overlapping pieces, a broadcast piece (src_count 1), a piece running past T, a segment
                            without pieces, steps no piece covers
  word_bag_kernel           <4, .> at C = 64 and 1100 (a second trip of the column loop), <1, .> at C = 30; bf16 and f32 rows; an empty
                            row, a word twice in a row; C_pad > C with bf16 rows (the f32 entry point takes no C_pad)
  transpose_f32_kernel      (2, 65, 129), (1, 1, 300)

Bounds (u = 2^-24, one f32 rounding):
  * copies, casts and sums in a promised order are compared bit for bit: bf16 against round-to-nearest-even of the f32 value
    (oracle.layout_ref.bf16_bits, pinned to torch's cast in tests/test_layout_host.py), NaN by isnan; pad rows and columns
    are exactly +0.
  * pack_features layer mean: an f32 sum of L <= 3 states times f32(1 / L), no cancellation: within one bf16 ulp of the float64
    mean and >= 99 % equal to round-to-nearest of it (the bf16 criterion of test_gpu_reductions.py; the CPU restatement of this
    arithmetic reaches 100.00 % on these inputs, tests/test_layout_host.py::test_layer_mean_f32_share).
  * rotary: a' = a c - b s is two f32 products and one add (or a product and an FMA), so it is within 3 u (|a c| + |b s|) of the
    float64 value before the one rounding to bf16: one bf16 ulp plus that floor, >= 99 % equal to round-to-nearest.  Everything
    outside the rotated span is bit-identical to the input.
  * dwconv + LayerNorm + swish: with k = K + C / 64 + 10 roundings (K for a conv sum, C / 64 + 10 for the row mean's chain),
    d_c = conv_c - mean is off by dd_c <= k u (m_c + mean_c m), m_c the sum of the magnitudes of the K terms.  The variance sees
    those errors as d var <= 2 mean |d| dd <= 2 max dd / rstd, so rstd is off by <= rstd^2 max dd relative, and
    v = d rstd w + b by  dv <= rstd |w| (dd_c + |d_c| rstd max dd) + 4 u |v|.  swish has slope <= 1.1, and the fast exponential
    of an f32 argument errs by (2 |v| + 3) u relative (as for exp in test_gpu_reductions.py), which the quotient passes on:
    floor = 1.1 dv + (2 |v| + 8) u |y|, on top of one bf16 ulp.  Share equal to round-to-nearest: a plain f32 restatement reaches
    >= 99.99 % on these inputs (tests/test_layout_host.py::test_conv_module_f32_share, kept as oracle.layout_ref.MEASURED_CONV_SHARE); asserted here less
    one point, 98.99 %.
  * f32 means and pools: `assert_f32_rows` of test_gpu_reductions.py (1e-5 of the row's largest reference magnitude) plus
    k u x the mean of the magnitudes summed, k = 80 as there (the longest chain here is 64 rows of a slice, a divide and the
    atomic adds of <= 6 slices); an empty window gives exactly 0.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout_ref as ref  # noqa: E402

U = 2.0**-24
ROWS = 37
CONV_SHARE = ref.MEASURED_CONV_SHARE - 0.01      # measured on the CPU (tests/test_layout_host.py::test_conv_module_f32_share) less one point


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tribe_hip import ops as _ops

    return _ops


def _call(name: str, *args) -> None:
    """A C-ABI entry point without an ops wrapper, on the current stream (the calling convention of modeling_utils/autograd.py)."""
    from tribe_hip._lib import check, lib

    check(getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    from tribe_hip import _lib

    return {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float64: _lib.F64}[dtype]


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _wide(*shape, seed: int) -> torch.Tensor:
    """f32 N(0, 1) at magnitudes from 1e-6 to 1e6, a few exact zeros."""
    g = _gen(seed)
    x = torch.randn(*shape, generator=g) * 10.0 ** (12 * torch.rand(*shape, generator=g) - 6)
    x.view(-1)[::97] = 0
    return x


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def _bits16(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bits32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def assert_bf16_bits(got: torch.Tensor, want_f32: torch.Tensor, what: str):
    """got bf16 == round-to-nearest-even of the f32 values, bit for bit; NaN by isnan."""
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(want_f32.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want_f32.shape)}"
    g, w = _bits16(got), ref.bf16_bits(want_f32).reshape(got.shape)
    nan = torch.isnan(want_f32).numpy().reshape(got.shape)
    gnan = (g & 0x7FFF) > 0x7F80
    assert np.array_equal(gnan, nan), f"{what}: NaN pattern differs"
    bad = (g != w) & ~nan
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} bf16 outputs differ from round-to-nearest-even; first at "
                           f"{tuple(int(i) for i in np.argwhere(bad)[0])}: {int(g[bad][0]):#06x} vs {int(w[bad][0]):#06x}")


def assert_f32_bits(got: torch.Tensor, want: torch.Tensor, what: str):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bad = _bits32(got) != _bits32(want.float())
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} f32 outputs differ in bits; first at {tuple(int(i) for i in np.argwhere(bad)[0])}"


def assert_zero_bits(t: torch.Tensor, what: str):
    """Pads: exactly +0 (the buffers start as NaN, so a pad the kernel skipped shows)."""
    t = t.detach().cpu().contiguous()
    view = t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)
    assert t.numel() == 0 or not view.any(), f"{what}: not exactly +0"


def assert_f32_rows(got, want, floor=0.0, what=""):
    got, want = got.detach().cpu().double(), want.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bound = 1e-5 * want.abs().amax(dim=-1, keepdim=True) + floor
    err = (got - want).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} f32 outputs beyond 1e-5 of the row's largest magnitude; "
                           f"first at {tuple(bad.nonzero()[0].tolist())}, worst excess {float((err - bound).max()):.3e}")


def _bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 numbers (8 significant bits) in the binade of |v|; the sub-normal spacing below the smallest normal."""
    _, e = torch.frexp(v.abs())
    return torch.where(v.abs() >= 2.0**-126, torch.ldexp(torch.ones_like(v), e - 8), torch.full_like(v, 2.0**-133))


def assert_bf16(got, want, floor=0.0, what="", share=0.99):
    got, want = got.detach().cpu().double(), want.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bound = _bf16_ulp(want) + floor
    err = (got - want).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} bf16 outputs more than one ulp from the float64 value; "
                           f"first at {tuple(bad.nonzero()[0].tolist())}, worst excess {float((err - bound).max()):.3e}")
    same = float((got == want.to(torch.bfloat16).double()).double().mean())
    print(f"{what}: {same:.5f} of the bf16 outputs equal round-to-nearest of the float64 value")
    assert same >= share, f"{what}: only {same:.4f} of the bf16 outputs equal round-to-nearest of the float64 value (need {share})"


# ------------------------------------------------------------------------------------------------
# pack_weight (pack_weight_kernel / cast_flat_kernel) and tribe_cast_bf16_fwd
# ------------------------------------------------------------------------------------------------
def _pack_weight(src: torch.Tensor, rows: int, cols: int, rows_pad: int, cols_pad: int) -> torch.Tensor:
    out = _nan(rows_pad, cols_pad, dtype=torch.bfloat16)
    _call("tribe_pack_weight_bf16", src.data_ptr(), rows, cols, cols, out.data_ptr(), rows_pad, cols_pad)
    return out


def _check_packed(out, w, what):
    rows, cols = w.shape
    assert_bf16_bits(out[:rows, :cols], w, what)
    assert_zero_bits(out[rows:], f"{what}: pad rows")
    assert_zero_bits(out[:, cols:], f"{what}: pad columns")


@pytest.mark.parametrize("rows,cols,rows_pad,cols_pad", [(50, 100, 56, 128), (9, 24, 9, 24), (7, 20, 7, 24), (33, 64, 33, 64),
                                                         (2050, 2056, 2050, 2112), (4100, 4096, 4100, 4096),
                                                         (4101, 4096, 4101, 4096)])
def test_pack_weight(rows, cols, rows_pad, cols_pad):
    w = _wide(rows, cols, seed=rows + cols)
    wd = w.cuda()
    assert wd.data_ptr() % 16 == 0
    _check_packed(_pack_weight(wd, rows, cols, rows_pad, cols_pad), w, f"pack_weight {rows}x{cols}")


@pytest.mark.parametrize("rows,cols,rows_pad,cols_pad", [(50, 100, 56, 128), (8, 64, 8, 64)])
def test_pack_weight_unaligned_source(rows, cols, rows_pad, cols_pad):
    """The source one float past a 16-byte boundary: every chunk of the generic kernel takes the scalar branch ((8, 64) would be the
    flat cast's were it aligned)."""
    w = _wide(rows * cols + 1, seed=rows)
    wd = w.cuda()
    src = wd[1:].view(rows, cols)
    assert src.data_ptr() % 16 == 4
    _check_packed(_pack_weight(src, rows, cols, rows_pad, cols_pad), w[1:].view(rows, cols), f"pack_weight unaligned {rows}x{cols}")


def test_cast_special_values():
    """Ties both ways, FLT_MAX -> inf, +-inf, +-0, f32 subnormals and a NaN through the generic pack kernel (vector and scalar
    branch), the flat cast and tribe_cast_bf16_fwd."""
    v = ref.special_f32_values()
    vd = v.cuda()
    assert_bf16_bits(_pack_weight(vd, 1, 32, 1, 32)[0], v, "cast_flat_kernel special values")
    out = _pack_weight(vd, 1, 32, 2, 40)
    assert_bf16_bits(out[0, :32], v, "pack_weight_kernel special values")
    assert_zero_bits(out[1], "pad row")
    assert_zero_bits(out[0, 32:], "pad columns")
    shifted = torch.cat([torch.zeros(1), v]).cuda()[1:]
    assert_bf16_bits(_pack_weight(shifted, 1, 32, 1, 32)[0], v, "pack_weight_kernel scalar branch special values")
    y = _nan(32, dtype=torch.bfloat16)
    _call("tribe_cast_bf16_fwd", vd.data_ptr(), 32, y.data_ptr())
    assert_bf16_bits(y, v, "cast_bf16 special values")


@pytest.mark.parametrize("n", [4, 2112, 4100 * 4096])
def test_cast_bf16(n):
    x = _wide(n, seed=n % 1009)
    xd = x.cuda()
    y = _nan(n + 8, dtype=torch.bfloat16)
    _call("tribe_cast_bf16_fwd", xd.data_ptr(), n, y.data_ptr())
    assert_bf16_bits(y[:n], x, f"cast_bf16 n={n}")
    assert torch.isnan(y[n:]).all(), "cast_bf16 wrote past n"


# ------------------------------------------------------------------------------------------------
# pack_subject_weights: transpose_cast_kernel<float>, [S, C, V] -> [S, V_pad, C_pad]
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,V", [(3, 70, 45), (1, 64, 128), (2, 65, 129)])
def test_pack_subject_weights(ops, S, C, V):
    w = _wide(S, C, V, seed=S + C + V)
    V_pad, C_pad = ops.round_up(V, 128), ops.round_up(C, 64)
    out = _nan(S, V_pad, C_pad, dtype=torch.bfloat16)
    wd = w.cuda()
    _call("tribe_pack_subject_weights", wd.data_ptr(), S, C, V, out.data_ptr(), V_pad, C_pad)
    assert_bf16_bits(out[:, :V, :C], w.transpose(1, 2).contiguous(), f"pack_subject_weights {(S, C, V)}")
    assert_zero_bits(out[:, V:], "pad rows")
    assert_zero_bits(out[:, :, C:], "pad columns")
    assert torch.equal(ops.pack_subject_weights(wd), out)                  # the wrapper picks the same pads


# ------------------------------------------------------------------------------------------------
# pack_features: 'cat' of f32 / bf16 -> tribe_transpose_bf16; f64, or a layer mean of any dtype -> transpose_cast_kernel
# ------------------------------------------------------------------------------------------------
FEATURE_SHAPES = [(3, 2, 37, 70), (1, 3, 64, 64), (2, 1, 65, 129)]


def _pack_features(feat, layer_mean, K_pad):
    B, L, D, T = feat.shape
    out = _nan(B * T, K_pad, dtype=torch.bfloat16)
    fd = feat.cuda()
    _call("tribe_pack_features", fd.data_ptr(), _dt(feat.dtype), B, L, D, T, int(layer_mean), out.data_ptr(), K_pad)
    return out


@pytest.mark.parametrize("wide_pad", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_pack_features_cat(ops, shape, dtype, wide_pad):
    """out[b T + t, l D + d] = bf16(feat[b, l, d, t]), bit for bit (a float64 state goes through f32, as the kernel's load does)."""
    B, L, D, T = shape
    feat = ref.layer_features(B, L, D, T, seed=B * 1000 + D, dtype=dtype)
    K = L * D
    K_pad = ops.round_up(K, 8) + 16 if wide_pad else ops.round_up(K, 64)
    out = _pack_features(feat, False, K_pad)
    want = feat.float().reshape(B, K, T).transpose(1, 2).reshape(B * T, K)
    assert_bf16_bits(out[:, :K], want, f"pack_features cat {shape} {dtype}")
    assert_zero_bits(out[:, K:], "pad columns")
    if not wide_pad:
        assert torch.equal(ops.pack_features(feat.cuda(), False), out)


@pytest.mark.parametrize("wide_pad", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_pack_features_layer_mean(ops, shape, dtype, wide_pad):
    B, L, D, T = shape
    feat = ref.layer_features(B, L, D, T, seed=B * 1000 + D, dtype=dtype)
    K_pad = ops.round_up(D, 8) + 16 if wide_pad else ops.round_up(D, 64)
    out = _pack_features(feat, True, K_pad)
    want = feat.double().mean(1).transpose(1, 2).reshape(B * T, D)
    assert_bf16(out[:, :D].float(), want, what=f"pack_features mean {shape} {dtype}")
    assert_zero_bits(out[:, D:], "pad columns")


# ------------------------------------------------------------------------------------------------
# rotary
# ------------------------------------------------------------------------------------------------
def _rotary_case(B, T, heads, heads_kv, d, rot, mode, seed):
    g = _gen(seed)
    width = (heads + 2 * heads_kv) * d
    x = torch.randn(B * T, width, generator=g).to(torch.bfloat16)
    cols = rot if mode == 2 else rot // 2
    if mode == 2:                        # any angle per element: the two elements of a pair see different ones
        ang = (torch.rand(T, cols, generator=g) * 2 - 1) * np.pi
        ang[0] = 0
    else:
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, rot, 2).float() / rot))
        ang = torch.arange(T).float()[:, None] * inv_freq[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    xd, cd, sd = x.cuda(), cos.cuda(), sin.cuda()
    _call("tribe_rotary_fwd", xd.data_ptr(), B * T, T, width, heads + heads_kv, d, rot, cd.data_ptr(), sd.data_ptr(), mode)
    n = heads + heads_kv
    want = ref.rotary(x, T, n, d, rot, cos, sin, mode)
    rotated = torch.zeros(B * T, width, dtype=torch.bool)
    rotated[:, : n * d].view(B * T, n, d)[:, :, :rot] = True
    # floor: 3 u (|a c| + |b s|) <= 3 u (|a| + |b|), a and b the two elements of the pair
    r = x.double()[:, : n * d].view(B * T, n, d)[:, :, :rot].abs()
    partner = torch.cat((r[..., rot // 2:], r[..., : rot // 2]), -1) if mode == 0 else r.unflatten(-1, (rot // 2, 2)).flip(-1).flatten(-2)
    floor = torch.zeros(B * T, width, dtype=torch.float64)
    floor[:, : n * d].view(B * T, n, d)[:, :, :rot] = 3 * U * (r + partner)
    got = xd.cpu()
    what = f"rotary mode {mode} d={d} rot={rot} rows={B * T}"
    assert_bf16(got.float()[rotated], want[rotated], floor[rotated], what=what)
    same = _bits16(got) == _bits16(x)
    assert same[~rotated.numpy()].all(), f"{what}: elements outside the rotated span changed (tail of a head or the V section)"
    assert not same[rotated.numpy()].all(), f"{what}: nothing was rotated"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d,rot", [(64, 64), (64, 32), (64, 8), (192, 192), (192, 96), (192, 8)])
def test_rotary_modes(d, rot, mode):
    _rotary_case(2, 19, 3, 2, d, rot, mode, seed=d + rot + mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rotary_beyond_grid_cap(mode):
    """2048 rows x 16 heads x 48 items = 1 572 864 work items: three trips of the grid-stride loop."""
    _rotary_case(2, 1024, 8, 8, 384, 384, mode, seed=40 + mode)


def test_rotary_wrapper_keeps_its_table_check(ops):
    x = torch.zeros(19, 3 * 64, dtype=torch.bfloat16, device="cuda")
    tab = torch.zeros(19, 32, device="cuda")
    with pytest.raises(ValueError):
        ops.rotary_(x, 19, 1, 64, 32, tab, tab, True)                         # [T, rot_dim] where [T, rot_dim / 2] is due


# ------------------------------------------------------------------------------------------------
# embedding and the nearest-neighbour row gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", [64, 100, 3])
def test_embedding(ops, dim, dtype):
    vocab = 11
    table = _wide(vocab, dim, seed=dim).to(dtype)
    ids = torch.randint(0, vocab, (3, 7), generator=_gen(dim + 1))
    ids[0, 0], ids[1, 3], ids[2, 6], ids[0, 5] = -1, vocab, vocab - 1, 0          # -1 and vocab are clamped to rows 0 and vocab - 1
    n = ids.numel()
    assert n % 4 != 0
    x = _nan(n + 1, dim)
    td, idd = table.cuda(), ids.cuda()
    _call("tribe_embedding_fwd", td.data_ptr(), _dt(dtype), idd.data_ptr(), n, dim, vocab, x.data_ptr())
    want = ref.embedding(table, ids)
    assert torch.equal(want, table[ids.flatten().clamp(0, vocab - 1)].float())
    assert_f32_bits(x[:n], want, f"embedding dim={dim} {dtype}")
    assert torch.isnan(x[n]).all(), "embedding wrote past its rows"
    assert_f32_bits(ops.embedding(td, idd), want, "ops.embedding with 2-D ids")


def _gather(x, idx, dim=None):
    B, T, D = x.shape
    n = idx.numel()
    out = _nan(B, n, D)
    xd, idd = x.cuda(), idx.cuda()
    _call("tribe_gather_rows_fwd", xd.data_ptr(), B, T, D if dim is None else dim, idd.data_ptr(), n, out.data_ptr())
    return out


@pytest.mark.parametrize("B,T,dim,n", [(2, 333, 128, 13), (1, 7, 4, 20), (3, 50, 1408, 1)])
def test_gather_rows(B, T, dim, n):
    from data_utils.features.audio import nearest_index

    x = _wide(B, T, dim, seed=T + n)
    idx = nearest_index(T, n)
    assert_f32_bits(_gather(x, idx), ref.gather_rows(x, idx), f"gather_rows {(B, T, dim, n)}")
    edge = torch.tensor([-1, T, 0, T - 1, -5, T + 100])
    assert_f32_bits(_gather(x, edge), x[:, [0, T - 1, 0, T - 1, 0, T - 1]], f"gather_rows clamped indices {(B, T, dim)}")


def test_gather_rows_refuses_odd_width():
    x, idx = torch.zeros(1, 5, 6, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    out = _nan(1, 3, 6)
    with pytest.raises(ValueError):
        _call("tribe_gather_rows_fwd", x.data_ptr(), 1, 5, 6, idx.data_ptr(), 3, out.data_ptr())
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------
# im2col3d
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Fr,C,H,W,tub,p,K_pad", [(2, 4, 3, 32, 48, 2, 16, 1536), (1, 2, 1, 16, 16, 1, 4, 24), (1, 6, 3, 28, 28, 3, 14, 1768),
                                                    (4, 8, 3, 224, 224, 2, 16, 1536)])
def test_im2col3d(B, Fr, C, H, W, tub, p, K_pad):
    pix = torch.randn(B, Fr, C, H, W, generator=_gen(H + W + tub))
    K = C * tub * p * p
    rows = B * (Fr // tub) * (H // p) * (W // p)
    out = _nan(rows, K_pad, dtype=torch.bfloat16)
    pd = pix.cuda()
    _call("tribe_im2col3d_fwd", pd.data_ptr(), B, Fr, C, H, W, tub, p, out.data_ptr(), K_pad)
    assert_bf16_bits(out[:, :K], ref.im2col3d(pix, tub, p).float(), f"im2col3d {(B, Fr, C, H, W, tub, p)}")
    assert_zero_bits(out[:, K:], "pad columns")


# ------------------------------------------------------------------------------------------------
# causal depthwise conv + LayerNorm + swish
# ------------------------------------------------------------------------------------------------
def _conv_run(x, w_dev, ln_w, ln_b, B, T, C, K):
    y = _nan(B * T, C, dtype=torch.bfloat16)
    xd, gd, bd = x.reshape(B * T, C).to(torch.bfloat16).cuda(), ln_w.cuda(), ln_b.cuda()
    _call("tribe_dwconv_ln_swish_fwd", xd.data_ptr(), B, T, C, K, w_dev.data_ptr(), gd.data_ptr(), bd.data_ptr(), float(np.float32(1e-5)),
          y.data_ptr())
    return y.float().cpu().view(B, T, C)


def _conv_reference(x, w, ln_w, ln_b, C, K):
    y, conv, mag, rstd = ref.dwconv_ln_swish(x, w, ln_w, ln_b, float(np.float32(1e-5)))
    k = K + C // 64 + 10
    d = conv - conv.mean(-1, keepdim=True)
    dd = k * U * (mag + mag.mean(-1, keepdim=True))
    v = d * rstd * ln_w.double() + ln_b.double()
    dv = rstd * ln_w.double().abs() * (dd + d.abs() * rstd * dd.amax(-1, keepdim=True)) + 4 * U * v.abs()
    return y, 1.1 * dv + (2 * v.abs() + 8) * U * y.abs()


@pytest.mark.parametrize("B,T,C,K", ref.CONV_SHAPES)
def test_dwconv_ln_swish(B, T, C, K):
    x, w, ln_w, ln_b = ref.conv_case(B, T, C, K, seed=C + K)
    want, floor = _conv_reference(x, w, ln_w, ln_b, C, K)
    wd = w.cuda()
    assert wd.data_ptr() % 16 == 0
    assert_bf16(_conv_run(x, wd, ln_w, ln_b, B, T, C, K), want, floor, what=f"dwconv_ln_swish {(B, T, C, K)}", share=CONV_SHARE)


def test_dwconv_tile_and_one_row_kernels_agree():
    """(2, 19, 128, 31) on the 8-step tile kernel, and again with the taps one float past a 16-byte boundary, which sends the same
    problem to the one-row kernel: both meet the float64 bound, so they differ by at most two bf16 ulps and agree on at least
    2 CONV_SHARE - 1 of the outputs."""
    B, T, C, K = 2, 19, 128, 31
    x, w, ln_w, ln_b = ref.conv_case(B, T, C, K, seed=C + K)
    want, floor = _conv_reference(x, w, ln_w, ln_b, C, K)
    tile = _conv_run(x, w.cuda(), ln_w, ln_b, B, T, C, K)
    shifted = torch.cat([torch.zeros(1), w.flatten()]).cuda()[1:].view(K, C)
    assert shifted.data_ptr() % 16 == 4
    one_row = _conv_run(x, shifted, ln_w, ln_b, B, T, C, K)
    assert_bf16(one_row, want, floor, what="dwconv_ln_swish one-row kernel, unaligned taps", share=CONV_SHARE)
    assert_bf16(tile, want, floor, what="dwconv_ln_swish tile kernel", share=CONV_SHARE)
    agree = float((tile == one_row).double().mean())
    assert agree >= 2 * CONV_SHARE - 1, f"the two kernels agree on {agree:.4f} of the outputs only"


# ------------------------------------------------------------------------------------------------
# segment_mean
# ------------------------------------------------------------------------------------------------
def _windows(T: int):
    """(start, length): full, interior, running past T, zero length, start >= T, start -2 with length 5 (rows 0..2 remain)."""
    return [(0, T), (T // 3, max(T // 4, 1)), (T - 3, 10), (2, 0), (T + 2, 4), (-2, 5)]


@pytest.mark.parametrize("B,T,dim", [(3, 7, 64), (2, 333, 1408), (2, 50, 30)])
def test_segment_mean(ops, B, T, dim):
    g = _gen(T + dim)
    x = torch.randn(B, T, dim, generator=g)        # one scale per output row, so that the row-wise bound means the same in every column
    x[0] += 1e3                                     # sequence 0: a mean of nearly equal large numbers
    xd = x.reshape(B * T, dim).cuda()
    wins = _windows(T)
    for i in range(0, len(wins), B):
        chunk = (wins[i:i + B] + wins[:B])[:B]
        start, length = (torch.tensor([w[j] for w in chunk], dtype=torch.int64) for j in (0, 1))
        got = ops.segment_mean(xd, B, T, start.cuda(), length.cuda())
        want = ref.segment_mean(x, start.tolist(), length.tolist())
        mags = ref.segment_mean(x.abs(), start.tolist(), length.tolist())
        assert_f32_rows(got, want, 80 * U * mags, what=f"segment_mean {(B, T, dim)} windows {chunk}")
        for b, (s, n) in enumerate(chunk):
            if n <= 0 or s >= T:
                assert_zero_bits(got[b], f"segment_mean empty window {(s, n)}")
            else:
                assert got[b].abs().max() > 0
    got = ops.segment_mean(xd, B, T, None, None)
    assert_f32_rows(got, x.double().mean(1), 80 * U * x.double().abs().mean(1), what=f"segment_mean {(B, T, dim)} whole sequences")


# ------------------------------------------------------------------------------------------------
# adaptive average pool, forward and backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [ROWS, 5000])
@pytest.mark.parametrize("T_in,T_out", [(298, 100), (14, 5), (64, 64), (100, 7), (5, 14)])
def test_adaptive_pool_fwd_bwd(ops, T_in, T_out, rows):
    _pool_case(ops, T_in, T_out, rows)


def test_adaptive_pool_beyond_grid_cap(ops):
    _pool_case(ops, 64, 64, 9000)


def _pool_case(ops, T_in, T_out, rows):
    g = _gen(T_in + T_out)
    x = torch.randn(rows, T_in, generator=g) * torch.logspace(-2, 2, rows)[:, None]
    x[1] = 1e3 + torch.randn(T_in, generator=g)
    x[0] = 0
    P = ref.adaptive_pool_matrix(T_in, T_out)
    got = ops.adaptive_avg_pool(x.cuda(), T_out)
    # a window holds <= ceil(T_in / T_out) + 1 terms: 20 roundings cover the longest here (16 adds and the divide)
    assert_f32_rows(got, ref.adaptive_avg_pool(x, T_out), 20 * U * (x.double().abs() @ P.t()), what=f"adaptive_avg_pool {(rows, T_in, T_out)}")
    dy = torch.randn(rows, T_out, generator=g) * torch.logspace(-2, 2, rows)[:, None]
    dx = _nan(rows, T_in)
    dyd = dy.cuda()
    _call("tribe_adaptive_avg_pool_bwd", dyd.data_ptr(), rows, T_in, T_out, dx.data_ptr())
    # an input sits in <= ceil(T_out / T_in) + 1 windows: a quotient and an add for each
    k = 2 * (-(-T_out // T_in) + 1)
    assert_f32_rows(dx, ref.adaptive_avg_pool_adjoint(dy, T_in), k * U * (dy.double().abs() @ P), what=f"adaptive_avg_pool_bwd {(rows, T_in, T_out)}")


# ------------------------------------------------------------------------------------------------
# projector_zero_fwd (fill_embed_kernel) and scale_cols
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(3, 7), (20, 700)])
@pytest.mark.parametrize("with_pos,with_subj", [(True, False), (False, True), (True, True), (False, False)])
def test_projector_zero(B, T, with_pos, with_subj):
    hidden, col0, N_out, S = 96, 32, 40, 4
    g = _gen(B + T)
    pos = torch.randn(T + 3, hidden, generator=g) if with_pos else None
    subj = torch.randn(S, hidden, generator=g) if with_subj else None
    sid = torch.randint(0, S, (B,), generator=g)
    x = _nan(B * T, hidden)
    sentinel = _bits32(x).copy()
    posd, subjd, sidd = (None if t is None else t.cuda() for t in (pos, subj, sid if with_subj else None))
    _call("tribe_projector_zero_fwd", B * T, T, N_out, x.data_ptr(), hidden, col0, _p(posd), _p(subjd), _p(sidd))
    want = torch.zeros(B, T, hidden)
    if with_pos:
        want = want + pos[None, :T]
    if with_subj:
        want = want + subj[sid][:, None]
    inside = slice(col0, col0 + N_out)
    assert_f32_bits(x[:, inside], want.reshape(B * T, hidden)[:, inside], f"projector_zero pos={with_pos} subj={with_subj}")
    got = _bits32(x)
    assert np.array_equal(got[:, :col0], sentinel[:, :col0]) and np.array_equal(got[:, col0 + N_out:], sentinel[:, col0 + N_out:]), \
        "projector_zero wrote outside [col0, col0 + N_out)"


@pytest.mark.parametrize("M,N", [(37, 100), (6000, 100)])
@pytest.mark.parametrize("with_scale", [True, False])
def test_scale_cols(M, N, with_scale):
    g = _gen(M)
    x = _wide(M, N, seed=M + 1)
    rs = (0.5 + torch.rand(N, generator=g)) if with_scale else None
    y = _nan(M + 1, N)
    xd, rsd = x.cuda(), None if rs is None else rs.cuda()
    _call("tribe_scale_cols_fwd", xd.data_ptr(), _p(rsd), M, N, y.data_ptr())
    assert_f32_bits(y[:M], x * rs[None] if with_scale else x, f"scale_cols {(M, N)}")
    assert torch.isnan(y[M]).all()


# ------------------------------------------------------------------------------------------------
# features.hip: piece sums, word bags, the f32 transpose
# ------------------------------------------------------------------------------------------------
def _piece_case():
    """B = 3 segments of C = 70 channels and T = 130 steps from three cached arrays [C, n]."""
    g = _gen(21)
    C = 70
    srcs = [torch.randn(C, n, generator=g) * torch.logspace(-2, 2, C)[:, None] for n in (40, 200, 25)]
    #         segment, source, src_first, src_count, dst_first, dst_count
    layout = [(0, 0, 5, 10, 60, 10),       # steps 60..69: across the edge of the first 64-step tile
              (0, 1, 30, 35, 65, 35),      # overlaps it on 65..69 and runs to 99
              (0, 2, 7, 1, 0, 50),         # one column broadcast over steps 0..49; steps 100..129 stay uncovered
              (0, 0, 0, 3, 62, 3),         # a third layer on 62..64: three terms in one cell, in list order
              # segment 1 has no piece
              (2, 1, 0, 130, 0, 130),      # the whole segment
              (2, 0, 10, 20, 120, 20),     # overlapping, and running 10 steps past T
              (2, 2, 24, 1, 127, 2)]       # a broadcast at the end
    return C, 130, srcs, layout


@pytest.mark.parametrize("C_pad", [128, 72])
def test_segment_gather(ops, C_pad):
    from tribe_hip._lib import BF16, F32, FEATURE_PIECE_DTYPE

    C, T, srcs, layout = _piece_case()
    B = 3
    dev = [s.cuda() for s in srcs]
    rec = np.zeros(len(layout), dtype=FEATURE_PIECE_DTYPE)
    for i, (seg, si, sf, sc, df, dc) in enumerate(layout):
        rec[i] = (dev[si].data_ptr(), srcs[si].shape[1], sf, sc, df, dc)
    seg_ptr = np.searchsorted([l[0] for l in layout], np.arange(B + 1)).astype(np.int32)
    assert seg_ptr.tolist() == [0, 4, 4, 7]
    pieces = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    ptr = torch.from_numpy(seg_ptr).cuda()
    want = torch.from_numpy(ref.piece_sum([(seg, srcs[si].numpy(), sf, sc, df, dc) for seg, si, sf, sc, df, dc in layout], B, C, T))
    assert not want[1].any() and not want[0, :, 100:].any() and want[0, :, 62].abs().min() > 0
    rows = _nan(B, C, T)
    _call("tribe_segment_gather_fwd", pieces.data_ptr(), ptr.data_ptr(), B, C, T, rows.data_ptr(), F32, C)
    assert_f32_bits(rows, want, "segment_gather rows layout")
    packed = _nan(B * T, C_pad, dtype=torch.bfloat16)
    _call("tribe_segment_gather_fwd", pieces.data_ptr(), ptr.data_ptr(), B, C, T, packed.data_ptr(), BF16, C_pad)
    assert_bf16_bits(packed[:, :C], want.transpose(1, 2).reshape(B * T, C), f"segment_gather packed C_pad={C_pad}")
    assert_zero_bits(packed[:, C:], "pad columns")
    assert torch.equal(ops.segment_gather(pieces, ptr, B, C, T, True, C_pad), packed)


@pytest.mark.parametrize("f32_out", [False, True])
@pytest.mark.parametrize("C,C_pad", [(64, 72), (30, 32), (1100, 1104)])
def test_word_bag(ops, C, C_pad, f32_out):
    n_words, rows = 9, 5
    table = _wide(n_words, C, seed=C)
    row_ptr = torch.tensor([0, 3, 3, 4, 8, 9], dtype=torch.int32)              # row 1 is empty
    word_idx = torch.tensor([2, 5, 2, 7, 0, 1, 1, 8, 4], dtype=torch.int32)    # word 2 twice in row 0, word 1 twice in row 3
    want = torch.from_numpy(ref.csr_row_sums(table, row_ptr.tolist(), word_idx.tolist()))
    td, rd, wd = table.cuda(), row_ptr.cuda(), word_idx.cuda()
    if f32_out:
        out = _nan(rows + 1, C)
        _call("tribe_word_bag_f32_fwd", td.data_ptr(), n_words, C, rd.data_ptr(), wd.data_ptr(), rows, out.data_ptr())
        assert_f32_bits(out[:rows], want, f"word_bag f32 C={C}")
        assert torch.isnan(out[rows]).all()
        assert_zero_bits(out[1], "empty row")
        return
    out = _nan(rows + 1, C_pad, dtype=torch.bfloat16)
    _call("tribe_word_bag_fwd", td.data_ptr(), n_words, C, rd.data_ptr(), wd.data_ptr(), rows, out.data_ptr(), C_pad)
    assert_bf16_bits(out[:rows, :C], want, f"word_bag bf16 C={C}")
    assert_zero_bits(out[:rows, C:], "pad columns")
    assert_zero_bits(out[1], "empty row")
    assert torch.isnan(out[rows]).all()
    assert torch.equal(ops.word_bag(td, rd, wd, rows, C_pad), out[:rows])


@pytest.mark.parametrize("Z,R,C", [(2, 65, 129), (1, 1, 300)])
def test_transpose_f32(ops, Z, R, C):
    x = _wide(Z, R, C, seed=R + C)
    out = _nan(Z, C, R)
    xd = x.cuda()
    _call("tribe_transpose_f32_fwd", xd.data_ptr(), Z, R, C, out.data_ptr())
    assert_f32_bits(out, x.transpose(1, 2).contiguous(), f"transpose_f32 {(Z, R, C)}")
    assert torch.equal(ops.transpose_f32(xd), out)
