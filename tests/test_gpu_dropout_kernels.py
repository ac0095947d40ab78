"""GPU: tribe_dropout_apply against the numpy restatement of its definition (tests/dropout_restatement.py), bit for bit, on every
launch branch: 16-byte accesses, 8-byte accesses (bf16 whose dim is a multiple of 4 but not of 8) and element accesses (odd dims, odd
pitches, a base pointer one element off 16-byte alignment).  The mask is integer-exact and a kept value is one f32 multiply (plus one
rounding to bf16), so equal bits are demanded: kept elements are `x.float() * scale` rounded by torch's own cast on the CPU, dropped
ones +0.0 with a clear sign bit; pad columns and the guard elements around the tensor keep their fill.

The `idx >> 34` half of the counter (the second counter word) stays 0 at any size a test can afford -- it needs more than 2^34 elements;
it is plain 64-bit C++ in the kernel (`quad >> 32`) and the restatement carries the same split."""

import functools

import pytest
import torch

from tests.dropout_restatement import expected, keep_mask

pytestmark = pytest.mark.gpu

GUARD = 37
ROWS = [1, 3, 257]
DIMS = [1, 2, 63, 64, 65, 200, 1024, 4100]
PS = [0.1, 0.15, 0.5]
KEYS = [(0x0123456789ABCDEF, 7), (0xF00DFACE12345678, (3 << 56) | (2 << 16) | 0xFFFF)]   # the second: bits above 2^32 in seed and site
LAYOUTS = ["tight", "pad64", "off1"]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _ld(dim, layout):
    return (dim + 63) // 64 * 64 if layout == "pad64" else dim


def _buffer(t, layout, fill):
    """(GPU buffer, its [rows, dim] view with contiguous rows of pitch ld holding t): guards and pad columns hold `fill`."""
    rows, dim = t.shape
    ld, off = _ld(dim, layout), int(layout == "off1")
    buf = torch.full((off + rows * ld + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[off:off + rows * ld].view(rows, ld)[:, :dim]
    view.copy_(t)
    if layout == "off1":
        assert view.data_ptr() % 16 == buf.element_size()
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _want_path(dtype, dim, layout):
    ld, q = _ld(dim, layout), (8 if dtype == torch.bfloat16 else 4)
    if layout == "off1":
        return "elem"
    if dim % q == 0 and ld % q == 0:
        return "vec16"
    if dtype == torch.bfloat16 and dim % 4 == 0 and ld % 4 == 0:
        return "vec8"
    return "elem"


@functools.lru_cache(maxsize=None)
def _input(rows, dim, dtype_name):
    g = torch.Generator().manual_seed(rows * 10007 + dim)
    return torch.randn(rows, dim, generator=g).to(DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def _expected(rows, dim, dtype_name, p, seed, site):
    return expected(_input(rows, dim, dtype_name), p, seed, site)


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_bits_equal_the_restatement(dtype_name, layout, inplace):
    from tribe_hip import ops

    dtype = DTYPES[dtype_name]
    for rows in ROWS:
        for dim in DIMS:
            x = _input(rows, dim, dtype_name)
            for p in PS:
                for seed, site in KEYS:
                    want = _expected(rows, dim, dtype_name, p, seed, site)
                    xbuf, xv = _buffer(x, layout, 7.0)
                    what = f"rows={rows} dim={dim} p={p} seed={seed:#x} site={site:#x}"
                    if inplace:
                        assert ops.dropout_path(xv) == _want_path(dtype, dim, layout), what
                        got = ops.dropout_apply(xv, p, seed, site, out=xv)
                        assert got is xv
                        wbuf, _ = _buffer(want, layout, 7.0)
                        assert torch.equal(_bits(xbuf), _bits(wbuf)), what                    # values, pad columns and guards at once
                    else:
                        obuf, ov = _buffer(torch.full_like(x, -3.0), layout, -3.0)
                        assert ops.dropout_path(xv, ov) == _want_path(dtype, dim, layout), what
                        ops.dropout_apply(xv, p, seed, site, out=ov)
                        wbuf, _ = _buffer(want, layout, -3.0)
                        assert torch.equal(_bits(obuf), _bits(wbuf)), what
                        xref, _ = _buffer(x, layout, 7.0)
                        assert torch.equal(_bits(xbuf), _bits(xref)), what                    # the input is untouched


def test_every_branch_is_reached():
    from tribe_hip import ops

    seen = {}
    for dtype_name, dtype in DTYPES.items():
        for layout in LAYOUTS:
            for dim in DIMS:
                _, xv = _buffer(torch.zeros(3, dim, dtype=dtype), layout, 7.0)
                path = ops.dropout_path(xv)
                assert path == _want_path(dtype, dim, layout), (dtype_name, layout, dim)
                seen.setdefault(dtype_name, set()).add(path)
    assert seen == {"f32": {"vec16", "elem"}, "bf16": {"vec16", "vec8", "elem"}}
    # mixed operands: the stricter one decides
    a = torch.zeros(3, 64, device="cuda")
    _, b = _buffer(torch.zeros(3, 64), "off1", 0.0)
    assert ops.dropout_path(a, b) == "elem" and ops.dropout_path(b, a) == "elem" and ops.dropout_path(a, torch.empty_like(a)) == "vec16"


@pytest.mark.parametrize("dtype_name,dim,layout", [("f32", 64, "tight"), ("f32", 65, "pad64"), ("bf16", 64, "pad64"), ("bf16", 4100, "tight"),
                                                   ("bf16", 63, "off1")])
def test_dropped_nan_and_negative_values_are_plus_zero(dtype_name, dim, layout):
    """A select, not a multiply: NaN, -1 and -inf at dropped positions come out as +0.0 (torch.dropout would give NaN / -0.0)."""
    from tribe_hip import ops

    rows, p, (seed, site) = 3, 0.5, KEYS[1]
    keep = torch.from_numpy(keep_mask(rows, dim, p, seed, site))
    x = _input(rows, dim, dtype_name).clone()
    poison = torch.tensor([float("nan"), -1.0, float("-inf")], dtype=x.dtype).repeat(rows * dim // 3 + 1)[:rows * dim].view(rows, dim)
    x = torch.where(keep, x, poison)
    _, xv = _buffer(x, layout, 7.0)
    got = ops.dropout_apply(xv, p, seed, site).cpu()
    assert got.is_contiguous() and got.shape == x.shape
    assert int((~keep).sum()) > rows * dim // 4 and bool((_bits(got)[~keep] == 0).all())          # +0.0: every bit clear
    assert torch.equal(_bits(got), _bits(expected(x, p, seed, site)))


def test_p_zero_launches_nothing_and_wrapper_errors():
    from tribe_hip import ops

    x = torch.randn(5, 12, device="cuda")
    assert ops.dropout_apply(x, 0.0, 1, 2) is x
    out = torch.empty_like(x)
    assert ops.dropout_apply(x, 0.0, 1, 2, out=out) is out and torch.equal(out, x)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            ops.dropout_apply(x, bad, 1, 2)
    with pytest.raises(ValueError):
        ops.dropout_apply(x, 0.5, 1, 2, out=torch.empty(5, 16, device="cuda"))
    with pytest.raises(TypeError):
        ops.dropout_apply(x, 0.5, 1, 2, out=torch.empty(5, 12, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.dropout_apply(x, 0.5, -1, 2)
    with pytest.raises(TypeError):
        ops.dropout_apply(x.double(), 0.5, 1, 2)


def test_result_does_not_depend_on_the_layout():
    """(seed, site, r, c, dim, p) alone: the three layouts -- three different kernels for bf16 dim 4100 / 200 -- give equal values."""
    from tribe_hip import ops

    for dtype_name in DTYPES:
        for dim in (200, 4100):
            x = _input(257, dim, dtype_name)
            outs = [ops.dropout_apply(_buffer(x, layout, 7.0)[1], 0.15, *KEYS[1]).cpu() for layout in LAYOUTS]
            assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
