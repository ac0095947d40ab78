"""CPU (no GPU): the plane values of tribe_gemm_desc.c_dtype (enum tribe_c_planes: the f32 residual stream as bf16 hi + 16-bit lo planes)
are resolved to the out-proj / FF2 role kernels at 256 x 256 tiles and refused, with one error text, on every other path: the generic
epilogue, the one-wave-per-SIMD kernel, 256 x 192 tiles, 128 x 128 tiles, split-K, transposed operands, other roles, the fp8 entry point.
Replayed through tribe_debug_gemm_plan with made-up addresses; nothing is launched."""

import ctypes as C

import pytest

KIND_BIG = 1
REFUSAL = "tribe_gemm_bf16: the plane c_dtype values (16-bit hi / lo residual stream) run on the out-proj / FF2 role kernels at 256 x 256 tiles only"


def _desc(role="out_proj", c_dtype=None, M=1024, N=768, K=256, **over):
    from tribe_hip import _lib

    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = 0x100000, K, 0x200000, K
    d.C, d.ldc = 0x300000, 2 * N     # (a lo row is 2 N 16-bit slots wide; an f32 launch simply gets a wide pitch)
    d.res, d.ldres = 0x300000, 2 * N
    d.c_bf16, d.ld_c_bf16 = 0x400000, N
    d.row_sumsq, d.ld_row_sumsq = 0x500000, N // 32
    d.alpha, d.role, d.tile_hint = 1.0, _lib.ROLE[role], 2
    d.c_dtype = _lib.F32_PLANES_INOUT if c_dtype is None else c_dtype
    if role == "ff2":
        d.bias, d.bias_mode = 0x600000, _lib.BIAS_COL
    for k, v in over.items():
        setattr(d, "role" if k == "role_id" else k, v)
    return d


def _plan(d, fp8=0):
    from tribe_hip import _lib

    out = (C.c_int64 * 19)()
    rc = _lib.lib().tribe_debug_gemm_plan(C.byref(d), fp8, out, 19)
    names = ["rc", "kind", "bm", "bn", "sumsq_cols", "splits", "pair", "epilogue_path"]
    return rc, dict(zip(names, list(out)[:8])), (_lib.lib().tribe_last_error().decode() if rc else "")


@pytest.mark.parametrize("role", ["out_proj", "ff2"])
@pytest.mark.parametrize("variant", ["F32_PLANES_OUT", "F32_PLANES_INOUT", "F32_PLANES_IN"])
@pytest.mark.parametrize("hint", [0, 2])
def test_planes_resolve_to_the_role_kernel(role, variant, hint):
    from tribe_hip import _lib

    # hint 0: the flagship shape, 256 x 256 tiles by the planner's own choice; FF2 takes its role kernel without tile_hint 2
    shape = dict(M=65536, N=3072, K=3072) if hint == 0 else {}
    d = _desc(role, getattr(_lib, variant), tile_hint=hint, **shape)
    rc, p, text = _plan(d)
    assert rc == 0, text
    assert (p["kind"], p["bm"], p["bn"], p["epilogue_path"], p["sumsq_cols"]) == (KIND_BIG, 256, 256, 1, 64)
    f32 = _desc(role, _lib.F32, tile_hint=2, **shape)
    assert _plan(f32)[1]["pair"] == p["pair"], "same kernel family (symbol role) as the f32 launch of the role"
    assert _lib.lib().tribe_gemm_epilogue_path(C.byref(d)) == 1 and _lib.lib().tribe_gemm_sumsq_slots(C.byref(d)) == d.N // 64


def test_f32_descriptors_are_untouched():
    from tribe_hip import _lib

    # FF2 keeps the generic epilogue by default; its role kernel under tile_hint 2 (gemm_plan.cpp, takes_role_epilogue)
    flagship = dict(M=65536, N=3072, K=3072)
    assert _plan(_desc("ff2", _lib.F32, tile_hint=0, **flagship))[1]["epilogue_path"] == 0
    assert _plan(_desc("ff2", _lib.F32, tile_hint=2))[1]["epilogue_path"] == 1
    assert _plan(_desc("out_proj", _lib.F32, tile_hint=0, **flagship))[1]["epilogue_path"] == 1


REFUSED = {
    "generic epilogue (tile_hint 6)": dict(tile_hint=6),
    "one-wave-per-SIMD kernel": dict(tile_hint=5),
    "256 x 192 tiles": dict(tile_hint=4),
    "256 x 192 tiles chosen by the planner": dict(tile_hint=0, M=8192),
    "128 x 128 double-buffered": dict(tile_hint=1),
    "128 x 128 ring": dict(tile_hint=3),
    "128 x 128 by size": dict(tile_hint=0, M=600, N=256),
    "split-K": dict(tile_hint=0, M=128, K=4096, stream_k=1, stream_k_ws=0x700000, stream_k_ws_bytes=1 << 30),
    "transposed operands": dict(trans_ab=1, lda=1024, ldb=768),
    "another role": dict(role_id=0),
    "alpha != 1 (generic epilogue)": dict(alpha=0.5),
    "no hi plane": dict(c_bf16=0, row_sumsq=0),
    "lo rows not 16-byte steps": dict(ldc=2 * 768 + 4, ldres=2 * 768 + 4),
    "lo rows too narrow": dict(ldc=768, ldres=768),
}


@pytest.mark.parametrize("role", ["out_proj", "ff2"])
@pytest.mark.parametrize("what", list(REFUSED))
def test_planes_are_refused_everywhere_else(role, what):
    from tribe_hip import _lib

    for variant in (_lib.F32_PLANES_OUT, _lib.F32_PLANES_INOUT, _lib.F32_PLANES_IN):
        d = _desc(role, variant, **REFUSED[what])
        rc, p, text = _plan(d)
        assert rc != 0 and text == REFUSAL, (what, rc, p, text)
        assert _lib.lib().tribe_gemm_epilogue_path(C.byref(d)) != 1
        # the same descriptor with an f32 C is a launch: the refusal is about the planes alone
        d.c_dtype = _lib.F32
        assert _plan(d)[0] == 0, (what, _plan(d)[2])


def test_fp8_entry_point_refuses_planes():
    from tribe_hip import _lib

    rc, _, text = _plan(_desc("out_proj", _lib.F32_PLANES_INOUT), fp8=1)
    assert rc != 0 and text == "tribe_gemm_fp8: c_dtype must be f32 or bf16"
    rc, _, text = _plan(_desc("out_proj", 19))
    assert rc != 0 and text == "tribe_gemm_bf16: c_dtype must be f32 or bf16"
