"""GPU: the autograd functions of modeling_utils/autograd.py (the layer that composes the kernels: which GEMM form a gradient takes,
which operand is padded, sliced or transposed, which buffer is zeroed, which summation route a bias gradient uses) per element against
the float64 statements of oracle/autograd_ref.py.  Every function is called through `.apply(...)` and `.backward(...)` as model.py and
models/common.py call it; every element of every output and gradient is compared.  tests/test_autograd_ref_host.py holds the
reference to float64 autograd and the criteria to a list of emulated faults.

Two kinds of case (oracle/autograd_ref.py)
  EXACT    Linear, QKVLinear, ProjectorFuse, VoxelHead + AdaptivePool, PackRows: integer activations, gradients and weights in [-3, 3],
           biases and residuals multiples of 1/64, res_scale in {1/2, 1, 2}.  Every f32 result is compared BIT FOR BIT with float64, every
           bf16 result with its round-to-nearest-even; nothing depends on the summation order, the K split, stream-K parts or slab order.
  BOUNDED  FeedForward, ScaleNorm, ScaleNormFork, InfoNCE, PearsonLossFn, ElemLoss: stage by stage from the intermediates the device
           stored (out.grad_fn.saved_tensors), each under a bound derived next to its check (ff_check, scalenorm_check, infonce_check,
           pearson_check, elem_check); the assertion is worst |err| / bound <= 1.

Every case records the launches of its backward (ag._gemm with its arguments and return value, ag.transpose_bf16, ag.colsum,
ag.cast_bf16, ops.norm_act behind cast_bf16) and asserts the route the table claims.

Branches and the case that reaches each
  wgrad              transposed operands: Linear trans_ab-64x128x128 (the smallest), N136 (ld_dy = Np = 192 behind dense_bwd's pad)
                     explicit transposes: M70 (M pad columns), N100 (N % 8), N120 (N < 128), K64 (K < 128)
                     stream-K engaged: stream-K (M = 21888, N = 264, K = 576: the smallest M the planner cuts for this 6-tile dw);
                     left whole: stream-K-whole-M256
  dense_bwd          Np == N: trans_ab-64x128x128; Np != N: N100, N120 (128), N136 (192), N102-M65; QKV 3N96
  grad_sums_and_cast fused pass, want_sum / res: on / on trans_ab-64x128x128, off / on M70, on / off N100, off / off N120;
                     fallback N % 4 != 0: N102-M65; fallback bf16 dy: bf16-out
  cast_bf16          numel % 4 != 0 through the row kernel: N102-M65; bf16 handed on: bf16-out, QKV
  Linear             out_f32 False: bf16-out; b None: M70, N120; res None: N100; res without res_scale: res-unscaled; raw_res_grad:
                     raw-res-grad (dres has dy's bits); K-padded: K-padded (dw [128, 100]); non-contiguous dy: dy-columns-view,
                     dy-transposed-view
  QKVLinear          3N % 64 == 0: 3N192-M128; 3N = 96: 3N96-M70, 3N96-M64; every case runs a second pass after wk.copy_(...): the repack
                     of _FusedQKVPacks.get into the buffer it holds
  ProjectorFuse      Kp != K with bias: K100-M70-bias, K100-M128-bias; Kp == K without: K128-M128, K128-M70
  VoxelHead + pool   batched + slab scatter: T40-C100in128-V20, T64-C64-V23-nobias, T40-C100in128-V65; per-sample chain:
                     T40-C99in128-V23-chain, T64-C101in128-V65-chain; Cp != Cc: every C..in128 case; bias None: T64-C64-V23-nobias; every
                     case repeats a subject and leaves one unused; every case runs twice
                     (x is bf16, so autograd hands x.grad on as bf16: dx is compared with the rounding of the exact f32 value)
  PackRows           f32-K100, bf16-K128 (the output is the input's storage), bf16-K100
  FeedForward        raw / res_scale: M70-raw-rs, M128-rs, M70-no-rs, M128-raw-no-rs; pre within [-6, 6]: M70-pre-within-6
  ScaleNorm / Fork   register kernel D = 768, walk kernel D = 512; dy bf16 and f32: norm-...-bf16 / -f32; residual only: fork-...-res(-rs);
                     normed branch only (`dxr is None`): fork-D512-bf16-norm-rs.  Residual only (`dy is None`) launches nothing: the gain
                     gets no gradient, which the cases assert.  FOUND HERE: autograd materialised the gradient of an unused output as zeros,
                     so neither branch was ever taken through .apply; ScaleNormFork.forward now calls ctx.set_materialize_grads(False)
  InfoNCE            N64-H64, N70-H128 (Np = 128), N64-H128, N70-H64; tau = 0.07
  PearsonLossFn      contiguous and the transposed '(b t) v' view (the gradient's strides are the view's), mean and sum, V = 1 and 37,
                     voxel 0 constant in pred
  ElemLoss           each kind x reduction at 231 elements with an upstream gradient of 3

Stale memory: the functions' internal buffers are torch.empty, so a pad that a kernel fails to write may happen to be zero.  Every case
runs a second time after blocks of the sizes it is about to request were filled with NaN patterns and freed on the same stream, and
must give the same bits.  This raises the chance of catching a stale read; it proves nothing when it passes.

MEASURED on an MI355X (worst |err| / bound per family; every test prints its own):
    EXACT      every quantity of every Linear (stream-K included), QKVLinear (both passes), ProjectorFuse, VoxelHead + pool and PackRows
               case, and pre, dres, db2, drs of every FeedForward case: the same bits (ratio 0)
    FeedForward  h 0.983 - 0.996 (the bf16 store: an error of half an ulp is 2^-8 |y| at the foot of a binade), out 0.0051, dw2 0.0125,
               db1 0.261, dx 0.793, dw1 0.492 (the three largest in M70-pre-within-6, where gelu' bends)
    ScaleNorm  y 0.99 (bf16; the store again) and 0.0137 (f32), dx 0.0232, dg 0.00054; residual only dx 0.0058 (with res_scale), 0 (without)
    InfoNCE    qn, kn 0.989 (the bf16 store), S 0.037, lse_r 0.0076, lse_c 0.0042, loss 7.9e-5, dq 0.676, dk 0.646
    Pearson    loss 0.0202, gradient 0.0345
    ElemLoss   loss 0.0071, gradient 0.0011
  No ratio above 1 and no bit mismatch: the kernels and the routes are right at these shapes.  The one finding is the dead pair of
  branches in ScaleNormFork.backward (above).
"""

import collections

import numpy as np
import pytest
import torch

from oracle import autograd_ref as ref
from oracle import tribe_ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from modeling_utils import autograd

    return autograd


def _dev(a, dtype=F32, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    return t.requires_grad_() if grad else t


def _param(a):
    return torch.nn.Parameter(_dev(a))


def _np(t):
    """A device tensor as the criteria take it: f32 array, or uint16 bit patterns of a bf16 tensor."""
    t = t.detach().contiguous().cpu()
    if t.dtype == BF16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.float().numpy() if t.dtype != F32 else t.numpy()


class Recorder:
    """Wraps the launch helpers of autograd.py; the wrappers call the real function with the same arguments."""

    def __init__(self, mp, ag):
        from tribe_hip import ops

        self.gemms, self.n, self.cast_same = [], collections.Counter(), []
        real_gemm = ag._gemm

        def gemm(a, b, out, **kw):
            ret = real_gemm(a, b, out, **kw)
            self.gemms.append(dict(kw, ret=ret))
            return ret

        mp.setattr(ag, "_gemm", gemm)
        for mod, name in ((ag, "transpose_bf16"), (ag, "colsum"), (ag, "cast_bf16"), (ops, "norm_act")):
            mp.setattr(mod, name, self._counted(getattr(mod, name), name))

    def _counted(self, real, name):
        def call(*a, **kw):
            self.n[name] += 1
            out = real(*a, **kw)
            if name == "cast_bf16":
                self.cast_same.append(out.data_ptr() == a[0].data_ptr())
            return out
        return call

    def mark(self):
        return len(self.gemms), collections.Counter(self.n), len(self.cast_same)

    def since(self, mark):
        g0, n0, c0 = mark
        return self.gemms[g0:], {k: self.n[k] - n0[k] for k in ("transpose_bf16", "colsum", "cast_bf16", "norm_act")}, self.cast_same[c0:]


@pytest.fixture
def rec(monkeypatch, ag):
    return Recorder(monkeypatch, ag)


def _poison(dims, mult=(1,)):
    """Best effort: blocks of the sizes a function is about to request (products of two of its dimensions, 2 and 4 bytes per element),
    filled with 0xFF bytes (a NaN as bf16 and as f32) and freed on the current stream: the caching allocator hands them out next."""
    dims = sorted(set(dims))
    sizes = {a * b * e * m for a in dims for b in dims for e in (2, 4) for m in mult} | {a * 4 for a in dims}
    blocks = [torch.empty(s, dtype=torch.uint8, device="cuda").fill_(0xFF) for s in sorted(sizes) for _ in range(2)]
    del blocks


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        x, y = (v.view(np.uint32) if v.dtype == np.float32 else v for v in (x, y))
        assert np.array_equal(x, y), f"{what}: {k} differs between two runs (first at {np.argwhere(x != y)[0].tolist()})"


def _report(family, c, results):
    name, ratio, where = ref.worst(results)
    print(f"\n{family} {c['name']}: worst {name} ratio {ratio:.3g} at {where}; " + ", ".join(f"{n} {r:.3g}" for n, r, _ in results))
    bad = [(n, r, w) for n, r, w in results if not r <= 1.0]
    assert not bad, f"{family} {c['name']}: {bad}"


def _grad(p):
    return None if p is None or p.grad is None else _np(p.grad)


def _put(got, **kw):
    for k, v in kw.items():
        if v is not None:
            got[k] = v
    return got


# ------------------------------------------------------------------------------------------------
# Linear
# ------------------------------------------------------------------------------------------------
def _run_linear(ag, rec, c, t):
    x = _dev(t["x"], BF16, grad=True)
    w = _param(t["w"])
    b, res, rs = (_param(t[k]) if k in t else None for k in ("b", "res", "rs"))
    y = ag.Linear.apply(x, w, b, res, rs, c["out_f32"], c["raw"])
    dy = _dev(t["dy"], y.dtype)
    if c["dy_view"] == "cols":
        wide = torch.zeros(c["M"], 2 * c["N"], dtype=y.dtype, device="cuda")
        wide[:, ::2] = dy
        dy = wide[:, ::2]
    elif c["dy_view"] == "t":
        dy = dy.t().contiguous().t()
    assert dy.is_contiguous() == (c["dy_view"] == "contig")
    mark = rec.mark()
    y.backward(dy)
    torch.cuda.synchronize()
    got = _put({"y": _np(y), "dx": _np(x.grad), "dw": _np(w.grad)}, db=_grad(b), dres=_grad(res), drs=_grad(rs))
    return got, rec.since(mark)


def _check_linear_route(c, launches):
    gemms, n, cast_same = launches
    r = ref.linear_route(c)
    M, Kx = c["M"], c["Kx"]
    assert len(gemms) == 2, gemms
    dgrad, wg = gemms
    assert (dgrad["K"], dgrad["lda"], dgrad.get("trans_ab", False)) == (r["Np"], r["Np"], False)
    if r["trans_ab"]:
        assert (wg["trans_ab"], wg["K"], wg["lda"], wg["ldb"], wg["stream_k"]) == (True, M, r["Np"], Kx, True)
        assert wg["ret"] == r["stream_k"], f"stream-K: the launcher {'cut' if wg['ret'] else 'did not cut'} the launch"
    else:
        Mp = ref.round_up(M, 64)
        assert (wg.get("trans_ab", False), wg["K"], wg["lda"], wg["ldb"]) == (False, Mp, Mp, Mp)
    assert n["transpose_bf16"] == r["transposes"] and n["colsum"] == r["colsums"] and n["cast_bf16"] == r["casts"], (n, r)
    assert n["norm_act"] == int(r["cast_row_kernel"])
    if not c["out_f32"]:
        assert cast_same == [True], "a bf16 gradient goes through cast_bf16 as it is"


@pytest.mark.parametrize("c", ref.LINEAR_CASES, ids=lambda c: c["name"])
def test_linear(ag, rec, c):
    t = ref.linear_inputs(c)
    want = ref.linear_reference(c, t)
    got, launches = _run_linear(ag, rec, c, t)
    _check_linear_route(c, launches)
    assert got["dw"].shape == (c["N"], c["K"])
    _report("linear", c, ref.check_exact(want, ref.linear_kinds(c), got))
    _poison([c["M"], ref.round_up(c["M"], 64), c["N"], ref.round_up(c["N"], 64), c["Kx"]] if c["M"] <= 1024 else [c["N"], c["Kx"], 320])
    again, _ = _run_linear(ag, rec, c, t)
    _same_bits(got, again, c["name"])


# ------------------------------------------------------------------------------------------------
# QKVLinear
# ------------------------------------------------------------------------------------------------
def _run_qkv(ag, rec, c, t, ws):
    x = _dev(t["x"], BF16, grad=True)
    for w in ws:
        w.grad = None
    y = ag.QKVLinear.apply(x, *ws)
    mark = rec.mark()
    y.backward(_dev(t["dy"], BF16))
    torch.cuda.synchronize()
    got = {"y": _np(y), "dx": _np(x.grad), "dwq": _np(ws[0].grad), "dwk": _np(ws[1].grad), "dwv": _np(ws[2].grad)}
    return got, rec.since(mark)


@pytest.mark.parametrize("c", ref.QKV_CASES, ids=lambda c: c["name"])
def test_qkv_linear(ag, rec, c):
    t = ref.qkv_inputs(c)
    ws = [_param(t[k]) for k in ("wq", "wk", "wv")]
    got, (gemms, n, cast_same) = _run_qkv(ag, rec, c, t, ws)
    r = ref.qkv_route(c)
    M, K = c["M"], c["K"]
    assert len(gemms) == 2 and (gemms[0]["K"], gemms[0]["lda"]) == (r["Np"], r["Np"])
    if r["trans_ab"]:
        assert (gemms[1]["trans_ab"], gemms[1]["K"], gemms[1]["lda"]) == (True, M, r["Np"])
    else:
        assert (gemms[1].get("trans_ab", False), gemms[1]["K"]) == (False, ref.round_up(M, 64))
    assert n["transpose_bf16"] == r["transposes"] and cast_same == [True]
    _report("qkv", c, ref.check_exact(ref.qkv_reference(c, t), ref.QKV_KINDS, got))
    dims = [M, ref.round_up(M, 64), 3 * c["N"], r["Np"], K]
    _poison(dims)
    again, _ = _run_qkv(ag, rec, c, t, ws)
    _same_bits(got, again, c["name"])
    # a weight written in place outside any optimiser: the next forward must repack it, into the fused buffer it already holds
    fused = ag.QKV_PACKS.get(tuple(ws))[0]
    with torch.no_grad():
        ws[1].copy_(_dev(t["wk2"]))
    _poison(dims)
    second, _ = _run_qkv(ag, rec, c, t, ws)
    assert ag.QKV_PACKS.get(tuple(ws))[0].data_ptr() == fused.data_ptr(), "the repack did not reuse the fused buffer"
    _report("qkv second pass", c, ref.check_exact(ref.qkv_reference(c, t, second=True), ref.QKV_KINDS, second))


# ------------------------------------------------------------------------------------------------
# ProjectorFuse
# ------------------------------------------------------------------------------------------------
def _run_projector(ag, rec, c, t):
    feat, w = _dev(t["feat"], BF16), _param(t["w"])
    b = _param(t["b"]) if "b" in t else None
    y = ag.ProjectorFuse.apply(feat, w, b)
    mark = rec.mark()
    y.backward(_dev(t["dy"]))
    torch.cuda.synchronize()
    return _put({"y": _np(y), "dw": _np(w.grad)}, db=_grad(b)), rec.since(mark)


@pytest.mark.parametrize("c", ref.PROJECTOR_CASES, ids=lambda c: c["name"])
def test_projector_fuse(ag, rec, c):
    t = ref.projector_inputs(c)
    got, (gemms, n, _) = _run_projector(ag, rec, c, t)
    r = ref.projector_route(c)
    Kp = ref.round_up(c["K"], 64)
    assert len(gemms) == 1 and gemms[0].get("trans_ab", False) == r["trans_ab"] and gemms[0]["N"] == Kp
    assert (n["transpose_bf16"], n["colsum"], n["cast_bf16"]) == (r["transposes"], r["colsums"], r["casts"])
    assert got["dw"].shape == (c["N"], c["K"])
    _report("projector", c, ref.check_exact(ref.projector_reference(c, t), {}, got))
    _poison([c["M"], ref.round_up(c["M"], 64), c["N"], Kp])
    again, _ = _run_projector(ag, rec, c, t)
    _same_bits(got, again, c["name"])


# ------------------------------------------------------------------------------------------------
# VoxelHead followed by AdaptivePool
# ------------------------------------------------------------------------------------------------
def _run_voxel(ag, rec, c, t):
    x, w = _dev(t["x"], BF16, grad=True), _param(t["w"])
    bias = _param(t["bias"]) if "bias" in t else None
    y = ag.VoxelHead.apply(x, w, bias, _dev(t["subjects"], torch.int64))
    pooled = ag.AdaptivePool.apply(y, c["Tout"])
    mark = rec.mark()
    pooled.backward(_dev(t["g"]))
    torch.cuda.synchronize()
    return _put({"y": _np(y), "pooled": _np(pooled), "dx": _np(x.grad), "dw": _np(w.grad)}, db=_grad(bias)), rec.since(mark)


@pytest.mark.parametrize("c", ref.VOXEL_CASES, ids=lambda c: c["name"])
def test_voxel_head_and_pool(ag, rec, c):
    t = ref.voxel_inputs(c)
    want = ref.voxel_reference(c, t)
    got, (gemms, n, _) = _run_voxel(ag, rec, c, t)
    r = ref.voxel_route(c)
    assert len(gemms) == r["gemms"] and n["transpose_bf16"] == r["transposes"]
    assert gemms[0]["batch1"] == c["B"] and gemms[0]["gather_b"]
    if r["batched"]:
        assert gemms[1]["batch1"] == c["B"] and gemms[1].get("res") is None
    else:
        assert all(g.get("batch1", 1) == 1 and g["res"] is not None for g in gemms[1:])
    unused = sorted(set(range(c["S"])) - set(c["subjects"]))
    assert unused and not got["dw"][unused].any() and ("db" not in got or not got["db"][unused].any()), "an unused subject's gradient is exactly zero"
    assert not ref.values(got["dx"])[:, :, c["Cc"]:].any(), "the pad columns of dx are exactly zero"
    _report("voxel", c, ref.check_exact(want, {"dx": "bf16"}, got))
    _poison([c["T"], ref.round_up(c["T"], 64), c["V"], ref.round_up(c["V"], 64), c["Cc"], c["Cp"]], mult=(1, c["B"], c["S"]))
    again, _ = _run_voxel(ag, rec, c, t)
    _same_bits(got, again, c["name"])


# ------------------------------------------------------------------------------------------------
# PackRows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.PACKROWS_CASES, ids=lambda c: c["name"])
def test_pack_rows(ag, c):
    t = ref.packrows_inputs(c)
    dtype = F32 if c["dtype"] == "f32" else BF16

    def run():
        x = _dev(t["x"], dtype, grad=True)
        y = ag.PackRows.apply(x)
        assert y.dtype == BF16 and y.shape == (c["M"], ref.round_up(c["K"], 64))
        if c["name"] == "bf16-K128":
            assert y.data_ptr() == x.data_ptr(), "a bf16 operand with K % 64 == 0 is handed on as it lies"
        y.backward(_dev(t["dy"], BF16))
        torch.cuda.synchronize()
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        return {"y": _np(y), "dx": _np(x.grad)}

    got = run()
    _report("packrows", c, ref.check_exact(ref.packrows_reference(c, t), ref.packrows_kinds(c), got))
    _poison([c["M"], c["K"], ref.round_up(c["K"], 64)])
    _same_bits(got, run(), c["name"])


# ------------------------------------------------------------------------------------------------
# FeedForward
# ------------------------------------------------------------------------------------------------
def _run_ff(ag, rec, c, t):
    x = _dev(t["x"], BF16, grad=True)
    w1, b1, w2, b2, res = (_param(t[k]) for k in ("w1", "b1", "w2", "b2", "res"))
    rs = _param(t["rs"]) if "rs" in t else None
    out = ag.FeedForward.apply(x, w1, b1, w2, b2, res, rs, c["raw"])
    saved = out.grad_fn.saved_tensors            # (x, w1, w2, pre, h, res, res_scale)
    got = {"pre": _np(saved[3]), "h": _np(saved[4]), "out": _np(out)}
    mark = rec.mark()
    out.backward(_dev(t["dout"]))
    torch.cuda.synchronize()
    _put(got, dx=_np(x.grad), dw1=_np(w1.grad), db1=_np(b1.grad), dw2=_np(w2.grad), db2=_np(b2.grad), dres=_grad(res), drs=_grad(rs))
    return got, rec.since(mark)


@pytest.mark.parametrize("c", ref.FF_CASES, ids=lambda c: c["name"])
def test_feed_forward(ag, rec, c):
    t = ref.ff_inputs(c)
    got, (gemms, n, _) = _run_ff(ag, rec, c, t)
    M, D, Fh = c["M"], c["D"], c["Fh"]
    assert len(gemms) == 4     # dpre (GELU_BWD), dw2, dx, dw1
    trans = ref.wgrad_reads_transposed(M, D, Fh, D, Fh)
    assert [g.get("trans_ab", False) for g in gemms] == [False, trans, False, ref.wgrad_reads_transposed(M, Fh, D, Fh, D)]
    assert n["transpose_bf16"] == (0 if trans else 4) and n["colsum"] == 1 and n["cast_bf16"] == 0
    _report("ff", c, ref.ff_check(c, t, got))
    _poison([M, ref.round_up(M, 64), D, Fh])
    again, _ = _run_ff(ag, rec, c, t)
    _same_bits(got, again, c["name"])


# ------------------------------------------------------------------------------------------------
# ScaleNorm, ScaleNormFork
# ------------------------------------------------------------------------------------------------
def _run_scalenorm(ag, c, t):
    x, g = _dev(t["x"], grad=True), _param(t["g"])
    if c["fn"] == "norm":
        y = ag.ScaleNorm.apply(x, g, t["gs"], t["eps"], c["out_f32"])
        y.backward(_dev(t["dy"], y.dtype))
    else:
        rs = _dev(t["rs"]) if "rs" in t else None
        y, xr = ag.ScaleNormFork.apply(x, g, t["gs"], t["eps"], rs)
        dy, dxr = _dev(t["dy"], BF16), _dev(t["dxr"])
        if c["use"] == "both":
            torch.autograd.backward([y, xr], [dy, dxr])
        elif c["use"] == "norm":
            y.backward(dy)
        else:
            xr.backward(dxr)
    torch.cuda.synchronize()
    assert y.dtype == (F32 if c["out_f32"] else BF16)
    return _put({"y": _np(y), "dx": _np(x.grad)}, dg=_grad(g))


@pytest.mark.parametrize("c", ref.SCALENORM_CASES, ids=lambda c: c["name"])
def test_scalenorm_and_fork(ag, c):
    t = ref.scalenorm_inputs(c)
    got = _run_scalenorm(ag, c, t)
    assert ("dg" in got) == (c["use"] != "res"), "residual only: ScaleNormFork.backward launches nothing and the gain gets no gradient"
    _report("scalenorm", c, ref.scalenorm_check(c, t, got))
    _poison([ref.SN_ROWS, c["D"]])
    _same_bits(got, _run_scalenorm(ag, c, t), c["name"])      # dg: a fixed-order sum, the same bits in every run


# ------------------------------------------------------------------------------------------------
# InfoNCE
# ------------------------------------------------------------------------------------------------
def _run_infonce(ag, c, t):
    q, k = _dev(t["q"], grad=True), _dev(t["k"], grad=True)
    loss = ag.InfoNCE.apply(q, k, ref.INFONCE_TAU)
    saved = loss.grad_fn.saved_tensors           # (q, k, qn, kn, S, lse_r, lse_c)
    got = {n: _np(s) for n, s in zip(("qn", "kn", "S", "lse_r", "lse_c"), saved[2:])}
    got["loss"] = _np(loss).reshape(1)
    loss.backward(torch.tensor(ref.INFONCE_G, device="cuda"))
    torch.cuda.synchronize()
    return _put(got, dq=_np(q.grad), dk=_np(k.grad))


@pytest.mark.parametrize("c", ref.INFONCE_CASES, ids=lambda c: c["name"])
def test_infonce(ag, c):
    t = ref.infonce_inputs(c)
    got = _run_infonce(ag, c, t)
    _report("infonce", c, ref.infonce_check(c, t, got))
    _poison([c["N"], ref.round_up(c["N"], 64), c["H"]])
    _same_bits(got, _run_infonce(ag, c, t), c["name"])


# ------------------------------------------------------------------------------------------------
# PearsonLossFn, ElemLoss
# ------------------------------------------------------------------------------------------------
def _strides(t):
    """The strides that address something: those of the dimensions longer than 1."""
    return tuple(s for s, n in zip(t.stride(), t.shape) if n > 1)


def _run_pearson(ag, c, t):
    B, V, T = c["B"], c["V"], c["T"]
    strides = []
    if c["layout"] == "bvt":
        leaf = _dev(t["pred"], grad=True)
        pred, true = leaf, _dev(t["true"])
    else:   # the '(b t) v' matrices of pl_module, seen as [1, V, B T]
        leaf = tribe_ref.flatten_bt(torch.from_numpy(t["pred"])).contiguous().cuda().requires_grad_()
        pred = leaf.t().unsqueeze(0)
        true = tribe_ref.flatten_bt(torch.from_numpy(t["true"])).contiguous().cuda().t().unsqueeze(0)
        assert V == 1 or pred.stride()[1:] == (1, V)
    pred.register_hook(lambda g: strides.append((_strides(g), g.shape)))
    loss = ag.PearsonLossFn.apply(pred, true, c["reduction"])
    loss.backward(torch.tensor(ref.PEARSON_G, device="cuda"))
    torch.cuda.synchronize()
    if c["layout"] == "view":
        assert strides == [(_strides(pred), pred.shape)], f"the gradient must come back in the view's strides: {strides} vs {pred.stride()}"
        grad = leaf.grad.view(B, T, V).permute(0, 2, 1)
    else:
        grad = leaf.grad
    return {"loss": _np(loss).reshape(1), "grad": _np(grad)}


@pytest.mark.parametrize("c", ref.PEARSON_CASES, ids=lambda c: c["name"])
def test_pearson_loss(ag, c):
    t = ref.pearson_inputs(c)
    got = _run_pearson(ag, c, t)
    _report("pearson", c, ref.pearson_check(c, t, got))
    _poison([c["B"] * c["T"], c["V"], 6])
    _same_bits(got, _run_pearson(ag, c, t), c["name"])


@pytest.mark.parametrize("c", ref.ELEM_CASES, ids=lambda c: c["name"])
def test_elem_loss(ag, c):
    t = ref.elem_inputs(c)
    pred = _dev(t["pred"], grad=True)
    loss = ag.ElemLoss.apply(pred, _dev(t["true"]), c["kind"], ref.ELEM_PARAM[c["kind"]], c["reduction"])
    (loss * ref.ELEM_G).backward()
    torch.cuda.synchronize()
    _report("elem", c, ref.elem_check(c, t, {"loss": _np(loss).reshape(1), "grad": _np(pred.grad)}))
