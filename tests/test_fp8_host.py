"""CPU: oracle/fp8_ref.py pinned to an independent implementation (torch.float8_e4m3fn on the CPU), and the exactness argument that
tests/test_gpu_fp8_bounds.py rests on.

The ONE intended difference between encode_e4m3 and torch's cast: torch turns everything that would round past 448 (+-inf included)
into NaN; the quantiser kernels clamp to +-448 first and so SATURATE.  464 is the midpoint between 448 and the 480 that the format
gives up for its NaN code: torch still takes it as a tie to the even mantissa, 448, and its first NaN is the f32 after 464.  Up to
and including 464 the two agree on every input."""

import numpy as np
import torch

from oracle import fp8_ref as ref


def _torch_codes(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _torch_values(codes: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn).double().numpy()


def test_decode_table_matches_torch_on_all_256_codes():
    codes = np.arange(256, dtype=np.uint8)
    want = _torch_values(codes)
    assert np.array_equal(np.isnan(ref.E4M3_VALUES), np.isnan(want))
    assert np.flatnonzero(np.isnan(ref.E4M3_VALUES)).tolist() == [0x7F, 0xFF]
    fin = ~np.isnan(want)
    assert np.array_equal(ref.E4M3_VALUES[fin], want[fin]) and np.array_equal(np.signbit(ref.E4M3_VALUES[fin]), np.signbit(want[fin]))
    assert ref.E4M3_VALUES[0x7E] == 448.0 and ref.E4M3_VALUES[0x01] == 2.0**-9 and ref.E4M3_VALUES[0x08] == 2.0**-6
    assert len(ref.FINITE_CODES) == 254


def test_encode_round_trips_every_finite_code():
    vals = ref.E4M3_VALUES[ref.FINITE_CODES].astype(np.float32)
    assert np.array_equal(ref.encode_e4m3(vals), ref.FINITE_CODES)            # -0 -> 0x80 included
    assert np.array_equal(_torch_codes(vals), ref.FINITE_CODES)


def test_encode_ties_go_to_the_even_code():
    lo, hi, mid = ref.midpoints()
    assert len(mid) == 126
    even = np.where(lo & 1, hi, lo)
    assert np.array_equal(ref.encode_e4m3(mid), even) and np.array_equal(ref.encode_e4m3(-mid), even | 0x80)
    below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    assert np.array_equal(ref.encode_e4m3(below), lo) and np.array_equal(ref.encode_e4m3(above), hi)
    for x in (mid, -mid, below, above, -below, -above):
        assert np.array_equal(ref.encode_e4m3(x), _torch_codes(x))


def test_encode_matches_torch_on_every_interesting_set_below_the_saturation_edge():
    for name, x in ref.interesting_f32().items():
        keep = np.abs(x) <= 464
        assert np.array_equal(ref.encode_e4m3(x[keep]), _torch_codes(x[keep])), name
    z = ref.encode_e4m3(np.array([0.0, -0.0, 2.0**-10, -(2.0**-10), 1e-9, -1e-9], dtype=np.float32))
    assert z.tolist() == [0x00, 0x80, 0x00, 0x80, 0x00, 0x80]                 # flush to zero keeps the sign, as torch does
    assert ref.encode_e4m3(np.nextafter(np.float32(2.0**-10), np.float32(1)))[()] == 0x01


def test_encode_saturates_where_torch_gives_nan():
    x = np.array([448.0, 463.99, 464.0, np.nextafter(np.float32(464), np.float32(np.inf)), 1e30, np.inf], dtype=np.float32)
    assert ref.encode_e4m3(x).tolist() == [0x7E] * 6 and ref.encode_e4m3(-x).tolist() == [0xFE] * 6
    t = _torch_codes(x)
    assert t[:3].tolist() == [0x7E] * 3                                        # 463.99 rounds down to 448, 464 ties to the even 448
    assert (t[3:] & 0x7F).tolist() == [0x7F] * 3                               # the one intended difference: past 464 torch gives NaN
    # after the clamp the two agree again
    assert np.array_equal(ref.encode_e4m3(x), _torch_codes(np.clip(x, -448, 448)))


def test_encode_nan_keeps_its_sign():
    pos = np.array([0x7FC00000, 0x7F800001], dtype=np.uint32).view(np.float32)
    neg = np.array([0xFFC00000, 0xFF800001], dtype=np.uint32).view(np.float32)
    assert ref.encode_e4m3(pos).tolist() == [0x7F, 0x7F] and ref.encode_e4m3(neg).tolist() == [0xFF, 0xFF]
    assert _torch_codes(pos).tolist() == [0x7F, 0x7F] and _torch_codes(neg).tolist() == [0xFF, 0xFF]
    assert ref.encode_e4m3(pos, inv_scale=np.float32(1 / 0.37)).tolist() == [0x7F, 0x7F]


def test_encode_scales_in_f32_first():
    g = np.random.default_rng(0)
    x = (g.standard_normal(20000) * 10.0 ** g.uniform(-4, 3, 20000)).astype(np.float32)
    inv = np.float32(1.0 / 0.37)
    y = (torch.from_numpy(x) * torch.tensor(inv)).clamp(-448, 448)
    assert np.array_equal(ref.encode_e4m3(x, inv), y.to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    assert np.array_equal(ref.scale_f32(x, inv), (torch.from_numpy(x) * torch.tensor(inv)).numpy())


def test_bf16_exact_subset_is_what_bf16_holds():
    x = np.concatenate(list(ref.interesting_f32().values()))
    sub = ref.bf16_exact(x)
    assert np.array_equal(torch.from_numpy(sub).bfloat16().float().numpy(), sub, equal_nan=True)
    lo, hi, mid = ref.midpoints()
    assert len(ref.bf16_exact(mid)) == len(mid)          # every midpoint (5 significant bits) and every code value is bf16-exact
    assert len(ref.bf16_exact(ref.interesting_f32()["codes"])) == 254


def test_epilogue64_against_torch():
    g = torch.Generator().manual_seed(2)
    M, N = 23, 12
    acc, res = torch.randn(M, N, generator=g, dtype=torch.float64) * 3, torch.randn(M, N, generator=g, dtype=torch.float64)
    cb, rb, rs = (torch.randn(n, generator=g, dtype=torch.float64) for n in (N, M, N))
    rowadd, gadd = torch.randn(7, N, generator=g, dtype=torch.float64), torch.randn(3, N, generator=g, dtype=torch.float64)
    gidx = np.array([2, 0, 2, 1, 2, 0], dtype=np.int64)      # rows 0-3 -> 2, 4-7 -> 0, 8-11 -> 2, ...
    F = torch.nn.functional
    v = acc * 0.5 + cb
    tail = res * rs + rowadd[torch.arange(M) % 7] + gadd[torch.from_numpy(gidx)[torch.arange(M) // 4]]
    for act, fn in ((None, lambda t: t), ("gelu", F.gelu), ("silu", F.silu)):
        got = ref.epilogue64(acc.numpy(), alpha=0.5, col_bias=cb.numpy(), act=act, res=res.numpy(), res_scale=rs.numpy(), rowadd=rowadd.numpy(),
                             rowadd_period=7, gadd=gadd.numpy(), gadd_index=gidx, gadd_div=4)
        np.testing.assert_allclose(got, (fn(v) + tail).numpy(), rtol=1e-13, atol=1e-14)
    got = ref.epilogue64(acc.numpy(), row_bias=rb.numpy(), res=res.numpy())
    np.testing.assert_allclose(got, (acc + rb[:, None] + res).numpy(), rtol=1e-15)
    np.testing.assert_allclose(ref.epilogue64(acc.numpy(), col_bias=cb.numpy(), act="swiglu"),
                               (F.silu((acc + cb)[:, 0::2]) * (acc + cb)[:, 1::2]).numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref.epilogue64(acc.numpy(), col_bias=cb.numpy(), act="glu"), F.glu((acc + cb).reshape(M, N // 2, 2), dim=-1).squeeze(-1).numpy(),
                               rtol=1e-13, atol=1e-15)
    # far tails: no cancellation, no overflow
    t = np.array([[-40.0, -12.0, 12.0, 800.0, -800.0, 0.0]])
    assert np.all(np.isfinite(ref.gelu64(t))) and np.all(np.isfinite(ref.silu64(t)))
    assert ref.gelu64(t)[0, 1] < 0 and abs(ref.gelu64(t)[0, 1] / (-12 * 0.5 * 3.552964224155306e-33) - 1) < 1e-9     # -12 Phi(-12); 1 + erf would give 0
    assert ref.silu64(t)[0, 4] == -800.0 * np.exp(-800.0) and ref.silu64(t)[0, 3] == 800.0


def test_sums_of_eighth_products_are_exact_in_any_order():
    """Operands j / 8, |j| <= 15: a product is an integer multiple of 2^-6 of magnitude <= 225 / 64 < 3.6, a sum of up to K = 1024 of
    them an integer count of 1/64ths below 1024 * 225 < 2^18 -- at most 18 significant bits, which f32 (24) holds exactly.  So every
    partial sum in EVERY order is exact, and forward, reversed and pairwise f32 sums are bit-identical to the integer result."""
    g = np.random.default_rng(1)
    K = 1024
    for trial in range(6):
        ja, jb = g.integers(-15, 16, K), g.integers(-15, 16, K)
        if trial == 0:
            ja[:], jb[:] = 15, 15                                  # the largest sum there is: 1024 * 225 / 64 = 3600
        a, b = ref.decode_e4m3(ref.eighths_codes(ja)).astype(np.float32), ref.decode_e4m3(ref.eighths_codes(jb)).astype(np.float32)
        p = (a * b).astype(np.float32)
        assert np.array_equal(p.astype(np.float64) * 64, (ja * jb).astype(np.float64)) and np.abs(p).max() < 3.6
        exact = int((ja * jb).sum())
        assert abs(exact) < 2**18
        fwd, rev, pair = ref.f32_sum_forward(p), ref.f32_sum_forward(p[::-1]), ref.f32_sum_pairwise(p)
        assert fwd.tobytes() == rev.tobytes() == pair.tobytes() == np.float32(exact / 64).tobytes()
        assert float(fwd) * 64 == exact
