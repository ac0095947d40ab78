"""CPU (no GPU): which epilogue a GEMM launch gets, read from the host-side plan (tribe_gemm_epilogue_path; csrc/gemm.hip, role8_ok).
The 8-wave kernels of QKV / FF1 / out-proj / FF2 hold ONLY the epilogue of their role's operator set, so the launcher must keep every
other descriptor away from them.  Pointers are made-up addresses: nothing is launched or dereferenced."""

import ctypes as C

import pytest

P = 0x7F0000000000   # a 16-byte aligned "device address"
M, N, K = 16384, 3072, 3072


def _desc(role, **kw):
    from tribe_hip import _lib

    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
    d.A, d.lda, d.B, d.ldb = P, K, P + (1 << 30), K
    d.C, d.ldc, d.alpha, d.role = P + (2 << 30), N, 1.0, _lib.ROLE[role]
    if role in ("qkv", "ff1"):
        d.c_dtype, d.row_scale = _lib.BF16, P + (3 << 30)
    else:
        d.c_dtype, d.res, d.ldres, d.res_scale = _lib.F32, P + (2 << 30), N, P + (4 << 30)
        d.c_bf16, d.ld_c_bf16, d.row_sumsq, d.ld_row_sumsq = P + (5 << 30), N, P + (6 << 30), N // 64
    if role in ("ff1", "ff2"):
        d.bias, d.bias_mode = P + (7 << 30), _lib.BIAS_COL
    if role == "ff1":
        d.act = _lib.ACT_GELU
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _path(d):
    from tribe_hip import _lib

    return _lib.lib().tribe_gemm_epilogue_path(C.byref(d))


@pytest.mark.parametrize("role", ["qkv", "ff1", "out_proj", "ff2"])
def test_model_descriptors_take_the_role_epilogue(role):
    assert _path(_desc(role)) == (0 if role == "ff2" else 1)   # automatic: FF2 keeps the generic epilogue (no measured gain), the others the role's
    assert _path(_desc(role, tile_hint=2)) == 1
    assert _path(_desc(role, tile_hint=4)) == 1         # 3072 = 16 x 192
    assert _path(_desc(role, tile_hint=6)) == 0         # the A/B switch
    assert _path(_desc(role, tile_hint=1)) == 0 and _path(_desc(role, tile_hint=3)) == 0   # 128 x 128 kernels
    assert _path(_desc(role, tile_hint=5)) == 2         # one-wave-per-SIMD kernel
    # optional operands absent: first-layer QKV, last-layer FF2, no residual scale
    if role in ("qkv", "ff1"):
        assert _path(_desc(role, row_scale=None)) == 1
    else:
        assert _path(_desc(role, tile_hint=2, res_scale=None, c_bf16=None, row_sumsq=None)) == 1


@pytest.mark.parametrize("role", ["qkv", "ff1", "out_proj", "ff2"])
def test_anything_off_the_operator_set_stays_generic(role):
    from tribe_hip import _lib

    bf_role = role in ("qkv", "ff1")
    off = [dict(alpha=0.5), dict(batch1=2), dict(gather1=P), dict(rowadd=P, rowadd_period=8), dict(gadd=P, gadd_index=P, gadd_div=8),
           dict(aux=P, ld_aux=N), dict(c_dtype=_lib.F32 if bf_role else _lib.BF16, c_bf16=None, row_sumsq=None), dict(ldc=N + 2), dict(C=P + 4),
           dict(bias=P, bias_mode=_lib.BIAS_ROW), dict(act=_lib.ACT_NONE if role == "ff1" else _lib.ACT_GELU), dict(trans_ab=1),
           dict(N=N + 64, ldc=N + 64, ld_c_bf16=N + 64)]
    if role in ("ff1", "ff2"):
        off += [dict(bias=None, bias_mode=_lib.BIAS_NONE), dict(bias=P + 4)]
    else:
        off += [dict(bias=P, bias_mode=_lib.BIAS_COL)]
    if bf_role:
        off += [dict(res=P, ldres=N), dict(c_bf16=P, ld_c_bf16=N), dict(row_sumsq=P, ld_row_sumsq=N // 64)]
    else:
        off += [dict(res=None, res_scale=None), dict(row_scale=P), dict(ldres=N + 2), dict(res_scale=P + 4), dict(c_bf16=P + 2), dict(ld_c_bf16=N + 2)]
    for kw in off:
        assert _path(_desc(role, **kw)) == 0, kw
    # another role's operators under this role's name, and roles that have no compiled epilogue
    other = {"qkv": "ff1", "ff1": "qkv", "out_proj": "ff2", "ff2": "out_proj"}[role]
    d = _desc(other)
    d.role = _lib.ROLE[role]
    assert _path(d) == 0
    for name in ("generic", "projector", "voxel_head", "attn_scores"):
        d = _desc(role)
        d.role = _lib.ROLE[name]
        assert _path(d) == 0
