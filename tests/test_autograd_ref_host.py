"""CPU: oracle/autograd_ref.py held to account before tests/test_gpu_autograd_bounds.py relies on it.

  * every hand-written float64 gradient equals torch.autograd on a float64 graph of the same function (1e-12 relative);
  * every EXACT case satisfies is_exact per reduction, and an f32 evaluation of sampled elements in three summation orders gives one
    bit pattern, the reference's;
  * the reference rounded the way the device rounds passes every case's criteria, and each fault of ref.FAULTS fails at least one;
  * the branch predicates restated in the case table agree with the code they mirror, and the table reaches every branch.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import autograd_ref as ref
from oracle import tribe_ref
from oracle.gemm_ref import f32_sums

RTOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= RTOL * scale, f"{what}: differs from float64 autograd"


def _t(a, grad=True):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy()).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------
# the reference is right
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in ref.LINEAR_CASES if c["M"] <= 1024], ids=lambda c: c["name"])
def test_linear_reference_is_autograd(c):
    t = ref.linear_inputs(c)
    r = ref.linear_reference(c, t)
    x, w = _t(t["x"][:, :c["K"]]), _t(t["w"])
    b, res, rs = (_t(t[k]) if k in t else None for k in ("b", "res", "rs"))
    y = x @ w.t()
    if b is not None:
        y = y + b
    if res is not None:
        y = y + (res * rs if rs is not None else res)
    y.backward(torch.from_numpy(t["dy"].astype(np.float64)))
    _close(r["y"], y.detach().numpy(), "y")
    _close(r["dx"][:, :c["K"]], x.grad.numpy(), "dx")
    assert not r["dx"][:, c["K"]:].any()
    _close(r["dw"], w.grad.numpy(), "dw")
    if b is not None:
        _close(r["db"], b.grad.numpy(), "db")
    if rs is not None:
        _close(r["drs"], rs.grad.numpy(), "drs")
    if res is not None and not c["raw"]:
        _close(r["dres"], res.grad.numpy(), "dres")
    if c["raw"]:        # the convention of raw_res_grad: the incoming gradient itself (ScaleNormFork applies res_scale)
        assert np.array_equal(r["dres"], t["dy"].astype(np.float64))


@pytest.mark.parametrize("c", ref.QKV_CASES, ids=lambda c: c["name"])
def test_qkv_reference_is_autograd(c):
    t = ref.qkv_inputs(c)
    for second in (False, True):
        r = ref.qkv_reference(c, t, second)
        x, ws = _t(t["x"]), [_t(t["wq"]), _t(t["wk2"] if second else t["wk"]), _t(t["wv"])]
        y = torch.cat([x @ w.t() for w in ws], dim=1)
        y.backward(torch.from_numpy(t["dy"].astype(np.float64)))
        _close(r["y"], y.detach().numpy(), "y")
        _close(r["dx"], x.grad.numpy(), "dx")
        for k, w in zip(("dwq", "dwk", "dwv"), ws):
            _close(r[k], w.grad.numpy(), k)
    assert not np.array_equal(t["wk"], t["wk2"])


@pytest.mark.parametrize("c", ref.PROJECTOR_CASES, ids=lambda c: c["name"])
def test_projector_reference_is_autograd(c):
    t = ref.projector_inputs(c)
    r = ref.projector_reference(c, t)
    f, w = _t(t["feat"][:, :c["K"]], False), _t(t["w"])
    b = _t(t["b"]) if "b" in t else None
    y = f @ w.t() + (b if b is not None else 0.0)
    y.backward(torch.from_numpy(t["dy"].astype(np.float64)))
    _close(r["y"], y.detach().numpy(), "y")
    _close(r["dw"], w.grad.numpy(), "dw")
    if b is not None:
        _close(r["db"], b.grad.numpy(), "db")


@pytest.mark.parametrize("c", ref.VOXEL_CASES, ids=lambda c: c["name"])
def test_voxel_reference_is_autograd(c):
    t = ref.voxel_inputs(c)
    r = ref.voxel_reference(c, t)
    x, w = _t(t["x"]), _t(t["w"])
    bias = _t(t["bias"]) if "bias" in t else None
    s = torch.from_numpy(t["subjects"])
    y = torch.einsum("btc,bcv->bvt", x[:, :, :c["Cc"]], w[s])
    if bias is not None:
        y = y + bias[s][:, :, None]
    pooled = torch.nn.functional.adaptive_avg_pool1d(y, c["Tout"])
    pooled.backward(torch.from_numpy(t["g"].astype(np.float64)))
    _close(r["y"], y.detach().numpy(), "y")
    _close(r["pooled"], pooled.detach().numpy(), "pooled")
    _close(r["dx"], x.grad.numpy(), "dx")
    _close(r["dw"], w.grad.numpy(), "dw")
    if bias is not None:
        _close(r["db"], bias.grad.numpy(), "db")
    unused = sorted(set(range(c["S"])) - set(c["subjects"]))
    assert unused and not r["dw"][unused].any(), "every case keeps a subject without samples: its gradient is exactly zero"
    assert not r["dx"][:, :, c["Cc"]:].any()


@pytest.mark.parametrize("c", ref.PACKROWS_CASES, ids=lambda c: c["name"])
def test_packrows_reference_is_autograd(c):
    t = ref.packrows_inputs(c)
    r = ref.packrows_reference(c, t)
    x = _t(ref.bf16r(t["x"]))
    y = torch.nn.functional.pad(x, (0, r["y"].shape[1] - c["K"]))
    y.backward(torch.from_numpy(t["dy"].astype(np.float64)))
    _close(r["y"], y.detach().numpy(), "y")
    _close(r["dx"], x.grad.numpy(), "dx")


@pytest.mark.parametrize("c", ref.FF_CASES, ids=lambda c: c["name"])
def test_ff_reference_is_autograd(c):
    t = ref.ff_inputs(c)
    s = ref.ff_stages(c, t)
    x, w1, b1, w2, b2, res = (_t(t[k]) for k in ("x", "w1", "b1", "w2", "b2", "res"))
    rs = _t(t["rs"]) if "rs" in t else None
    h = torch.nn.functional.gelu(x @ w1.t() + b1)
    out = h @ w2.t() + b2 + (res * rs if rs is not None else res)
    out.backward(torch.from_numpy(t["dout"].astype(np.float64)))
    _close(s["out"], out.detach().numpy(), "out")
    for k, p in (("dx", x), ("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2)):
        _close(s[k], p.grad.numpy(), k)
    if rs is not None:
        _close(s["drs"], rs.grad.numpy(), "drs")
    if not c["raw"]:
        _close(s["dres"], res.grad.numpy(), "dres")
    assert is_pre_exact(c, t) and ref.is_exact(c["D"]), "pre is exact in f32, and dout W2 (a reduction over D) an exact integer"
    if c["dense"]:
        assert ref.ff_pre_coverage(c, t) >= 0.9, "the dense case must keep pre within [-6, 6]"
        v = s["v"]
        assert all(((v >= lo) & (v < lo + 1)).sum() >= 50 for lo in range(-6, 6)), "and fill every unit interval of it"


def is_pre_exact(c, t) -> bool:
    """pre = x W1^T + b1: a multiple of 1/64 below 3 D + 2 with W1 in [-1, 1] and D <= 256: 24 bits hold it."""
    return c["D"] <= 256 and float(np.abs(t["w1"]).max()) <= 1 and ref.is_exact(c["D"], addends=True, bmax=1)


@pytest.mark.parametrize("c", ref.SCALENORM_CASES, ids=lambda c: c["name"])
def test_scalenorm_reference_is_autograd(c):
    t = ref.scalenorm_inputs(c)
    r = ref.scalenorm_reference(c, t)
    x, g = _t(t["x"]), _t(t["g"])
    y = x / x.norm(dim=-1, keepdim=True).clamp(min=t["eps"]) * t["gs"] * g
    loss = (y * torch.from_numpy(t["dy"].astype(np.float64))).sum() if c["use"] != "res" else y.sum() * 0
    if c["fn"] == "fork" and c["use"] != "norm":
        xr = x * (torch.from_numpy(t["rs"].astype(np.float64)) if "rs" in t else 1.0)
        loss = loss + (xr * torch.from_numpy(t["dxr"].astype(np.float64))).sum()
    loss.backward()
    _close(r["y"], y.detach().numpy(), "y")
    _close(r["dx"], x.grad.numpy(), "dx")
    _close(r["dg"], g.grad.numpy(), "dg")


@pytest.mark.parametrize("c", ref.INFONCE_CASES, ids=lambda c: c["name"])
def test_infonce_reference_is_autograd(c):
    t = ref.infonce_inputs(c)
    f = ref.infonce_full64(t)
    q, k = _t(t["q"]), _t(t["k"])
    logits = torch.nn.functional.normalize(q, dim=-1) @ torch.nn.functional.normalize(k, dim=-1).t() * t["alpha"]
    target = torch.arange(c["N"])
    loss = 0.5 * (torch.nn.functional.cross_entropy(logits, target) + torch.nn.functional.cross_entropy(logits.t(), target))
    loss.backward(torch.tensor(t["gs"] / t["alpha"], dtype=torch.float64))      # upstream g with g alpha = gs
    _close(f["loss"], loss.detach().numpy(), "loss")
    _close(f["dq"], q.grad.numpy(), "dq")
    _close(f["dk"], k.grad.numpy(), "dk")
    _, e = math.frexp(ref.INFONCE_TAU)
    assert math.ldexp(0.5, e) != ref.INFONCE_TAU, "tau must not be a power of two"


@pytest.mark.parametrize("c", ref.PEARSON_CASES, ids=lambda c: c["name"])
def test_pearson_reference_is_autograd(c):
    t = ref.pearson_inputs(c)
    r = ref.pearson_reference(c, t)
    x = _t(tribe_ref.flatten_bt(torch.from_numpy(t["pred"])).numpy())
    y = tribe_ref.flatten_bt(torch.from_numpy(t["true"])).double()
    live = slice(1, None) if c["V"] > 1 else slice(None)                        # voxel 0 is constant in pred where V > 1
    loss = tribe_ref.pearson_loss(x[:, live], y[:, live], "sum")
    k = ref.PEARSON_G * (1.0 / c["V"] if c["reduction"] == "mean" else 1.0)
    (loss * k).backward()
    got = tribe_ref.flatten_bt(torch.from_numpy(r["grad"])).numpy()
    _close(got[:, live], x.grad.numpy()[:, live], "grad")
    const = 1.0 if c["V"] > 1 else 0.0                                          # a constant voxel: r = 0, loss 1
    _close(r["loss"], np.array([(float(loss.detach()) + const) * k / ref.PEARSON_G]), "loss")   # the forward carries no upstream g
    if c["V"] > 1:      # the convention: the finite term -k / den (y - mean y), den = 1e-8
        yc = y[:, 0] - y[:, 0].mean()
        _close(got[:, 0], (-k / 1e-8 * yc).numpy(), "constant voxel")


@pytest.mark.parametrize("c", ref.ELEM_CASES, ids=lambda c: c["name"])
def test_elem_reference_is_autograd(c):
    t = ref.elem_inputs(c)
    r = ref.elem_reference(c, t)
    F = torch.nn.functional
    p = ref.ELEM_PARAM[c["kind"]]
    fn = {"l1": F.l1_loss, "mse": F.mse_loss, "smooth_l1": lambda a, b, reduction: F.smooth_l1_loss(a, b, reduction=reduction, beta=p),
          "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=p)}[c["kind"]]
    x = _t(t["pred"])
    loss = fn(x, torch.from_numpy(t["true"].astype(np.float64)), reduction=c["reduction"])
    (loss * ref.ELEM_G).backward()
    _close(r["loss"], np.array([float(loss.detach())]), "loss")
    _close(r["grad"], x.grad.numpy(), "grad")
    assert t["pred"].size % 4 != 0


# ------------------------------------------------------------------------------------------------
# the exact cases are exact
# ------------------------------------------------------------------------------------------------
EXACT = [("linear", ref.linear_reductions), ("qkv", ref.qkv_reductions), ("projector", ref.projector_reductions), ("voxel", ref.voxel_reductions)]


@pytest.mark.parametrize("family,reductions", EXACT, ids=[f for f, _ in EXACT])
def test_exact_cases_satisfy_is_exact_per_reduction(family, reductions):
    for c in ref.FAMILIES[family]:
        for what, length, ok in reductions(c):
            assert ok, f"{family} {c['name']}: {what} (length {length}) is not exact in f32"


def _one_pattern(products, want, what):
    sums = f32_sums(products)
    bits = {np.float32(s).view(np.uint32).item() for s in sums}
    assert bits == {np.float32(want).view(np.uint32).item()} and float(np.float32(want)) == float(want), f"{what}: {sums} vs {want}"


@pytest.mark.parametrize("c", [c for c in ref.LINEAR_CASES if c["M"] <= 1024], ids=lambda c: c["name"])
def test_linear_f32_sums_do_not_depend_on_the_order(c):
    t = ref.linear_inputs(c)
    r = ref.linear_reference(c, t)
    x, w, dy = t["x"], t["w"], t["dy"]
    K = c["K"]
    for m, n, k in ((0, 0, 0), (c["M"] - 1, c["N"] - 1, K - 1)):
        addends = [t["b"][n]] if "b" in t else []
        if "res" in t:
            addends.append(t["res"][m, n] * (t["rs"][n] if "rs" in t else np.float32(1)))
        _one_pattern(np.concatenate([x[m, :K] * w[n], np.array(addends, dtype=np.float32)]), r["y"][m, n], "y")
        _one_pattern(dy[m] * w[:, k], r["dx"][m, k], "dx")
        _one_pattern(dy[:, n] * x[:, k], r["dw"][n, k], "dw")
        if "b" in t:
            _one_pattern(dy[:, n], r["db"][n], "db")
        if "rs" in t:
            _one_pattern(dy[:, n] * t["res"][:, n], r["drs"][n], "drs")


@pytest.mark.parametrize("c", ref.VOXEL_CASES, ids=lambda c: c["name"])
def test_voxel_f32_sums_do_not_depend_on_the_order(c):
    t = ref.voxel_inputs(c)
    r = ref.voxel_reference(c, t)
    dy = ref.adaptive_avg_pool_adjoint(torch.from_numpy(t["g"]), c["T"]).numpy().astype(np.float32)
    assert np.array_equal(ref.bf16r(dy), dy.astype(np.float64)), "the pool's adjoint must be a bf16 value: the backward casts it"
    s = c["subjects"]
    sub = s[0]
    samples = [b for b in range(c["B"]) if s[b] == sub]
    cc, v = c["Cc"] - 1, c["V"] - 1
    _one_pattern(np.concatenate([t["x"][b, :, cc] * dy[b, v] for b in samples]), r["dw"][sub, cc, v], "dW")
    _one_pattern(dy[0, :, 3] * t["w"][s[0], cc], r["dx"][0, 3, cc], "dx")
    if "bias" in t:
        _one_pattern(np.concatenate([dy[b, v] for b in samples]), r["db"][sub, v], "db")


# ------------------------------------------------------------------------------------------------
# the criteria pass the clean reference and catch every fault
# ------------------------------------------------------------------------------------------------
def _clean(family, c):
    if family == "linear":
        t = ref.linear_inputs(c)
        r, kinds = ref.linear_reference(c, t), ref.linear_kinds(c)
    elif family == "qkv":
        t = ref.qkv_inputs(c)
        r, kinds = ref.qkv_reference(c, t), ref.QKV_KINDS
    elif family == "projector":
        t = ref.projector_inputs(c)
        r, kinds = ref.projector_reference(c, t), {}
    elif family == "voxel":
        t = ref.voxel_inputs(c)
        r, kinds = ref.voxel_reference(c, t), {}
    elif family == "packrows":
        t = ref.packrows_inputs(c)
        r, kinds = ref.packrows_reference(c, t), ref.packrows_kinds(c)
    else:
        inputs, emulate, check = (getattr(ref, f"{family}_{n}") for n in ("inputs", "emulate", "check"))
        t = inputs(c)
        return check(c, t, emulate(c, t))
    return ref.check_exact(r, kinds, ref.emulate_exact(r, kinds))


SMALL = [(f, c) for f, cases in ref.FAMILIES.items() for c in cases if c.get("M", 0) <= 1024]


@pytest.mark.parametrize("family,c", SMALL, ids=[f"{f}-{c['name']}" for f, c in SMALL])
def test_clean_reference_rounded_like_the_device_passes(family, c):
    results = _clean(family, c)
    name, ratio, where = ref.worst(results)
    assert ratio <= 1.0, f"{family} {c['name']}: {name} ratio {ratio} at {where}"


FAULT_NAMES = ["the last row of dw left from the previous tile", "db summed over M - 1 rows", "drs computed from dy instead of dy * res",
               "dres scaled when raw_res_grad is set", "the q and k slices of dw swapped", "one repeated subject's slab added twice",
               "a pad column of dx equal to its neighbour", "gelu' taken at h instead of pre", "1/tau applied twice", "mean taken for sum"]


def test_fault_list_is_whole():
    assert sorted(ref.FAULTS) == sorted(FAULT_NAMES)


@pytest.mark.parametrize("fault", FAULT_NAMES)
def test_every_fault_fails_a_case(fault):
    family, run = ref.FAULTS[fault]
    caught, applied = [], 0
    for c in ref.FAMILIES[family]:
        results = run(c)
        if results is None:
            continue
        applied += 1
        if ref.worst(results)[1] > 1.0:
            caught.append(c["name"])
    assert applied and caught, f"{fault}: applied to {applied} cases of {family}, caught by none"


# ------------------------------------------------------------------------------------------------
# the tables stay in step with the code
# ------------------------------------------------------------------------------------------------
def test_predicates_agree_with_the_code():
    from modeling_utils import autograd as ag
    from tribe_hip import ops

    for M in (64, 70, 128):
        for N in (96, 100, 120, 128, 136, 264):
            for K in (64, 100, 128, 576):
                for ld in (N, ops.round_up(N, 64), N + 4):
                    assert ref.wgrad_reads_transposed(M, N, K, ld, K) == ag.wgrad_reads_transposed(M, N, K, ld, K)
    for a in (1, 63, 64, 65, 100, 136):
        assert ref.round_up(a, 64) == ops.round_up(a, 64)


def test_stream_k_case_is_the_smallest_the_library_cuts():
    from tribe_hip import _lib

    N, K = ref.STREAM_K_NK

    def cut(M):
        d = _lib.GemmDesc()      # the launch of autograd.wgrad: dw [N, K] = dy^T x over M
        d.M, d.N, d.K, d.batch1, d.batch0, d.alpha, d.stream_k, d.trans_ab = N, K, M, 1, 1, 1.0, 1, 1
        d.lda, d.ldb, d.ldc, d.c_dtype = ref.round_up(N, 64), K, K, _lib.F32
        return _lib.lib().tribe_gemm_stream_k_workspace_bytes(ctypes.byref(d)) > 0

    M = ref.STREAM_K_M
    assert M % 64 == 0 and ref.stream_k_engages(M, N, K) and not ref.stream_k_engages(M - 64, N, K)
    assert cut(M) and not cut(M - 64) and not cut(256)
    assert ref.is_exact(M), "9 M < 2^24 keeps the large case exact"


def test_the_table_reaches_every_branch():
    routes = {c["name"]: ref.linear_route(c) for c in ref.LINEAR_CASES}
    by = lambda **kw: [n for n, r in routes.items() if all(r[k] == v for k, v in kw.items())]      # noqa: E731
    assert by(trans_ab=True, stream_k=True) == ["stream-K"] and "stream-K-whole-M256" in by(trans_ab=True, stream_k=False)
    assert routes["trans_ab-64x128x128"]["trans_ab"] and routes["N136"]["trans_ab"] and routes["N136"]["Np"] == 192
    for name in ("M70", "N100", "N120", "K64"):
        assert not routes[name]["trans_ab"], name
    assert {r["Np"] != ref.LINEAR_CASES[i]["N"] for i, r in enumerate(routes.values())} == {True, False}
    assert not routes["N102-M65"]["fused_sums"] and routes["N102-M65"]["cast_row_kernel"] and routes["N102-M65"]["colsums"] == 2
    assert not routes["bf16-out"]["fused_sums"] and not routes["bf16-out"]["cast_row_kernel"]
    fused = {(c["bias"], c["res"] == "scaled") for c in ref.LINEAR_CASES if ref.linear_route(c)["fused_sums"]}
    assert fused == {(True, True), (True, False), (False, True), (False, False)}, "the fused pass with want_sum and res on and off"
    assert {ref.qkv_route(c)["Np"] == 3 * c["N"] for c in ref.QKV_CASES} == {True, False}
    assert {ref.qkv_route(c)["trans_ab"] for c in ref.QKV_CASES} == {True, False}
    assert {(c["K"] % 64 == 0, c["bias"], c["M"]) for c in ref.PROJECTOR_CASES} >= {(False, True, 70), (True, False, 128)}
    assert {ref.voxel_route(c)["batched"] for c in ref.VOXEL_CASES} == {True, False}
    assert {c["Cp"] != c["Cc"] for c in ref.VOXEL_CASES} == {True, False} and {c["V"] for c in ref.VOXEL_CASES} == {20, 23, 65}
    assert {c["T"] for c in ref.VOXEL_CASES} == {40, 64} and any(not c["bias"] for c in ref.VOXEL_CASES)
    assert all(len(set(c["subjects"])) < len(c["subjects"]) for c in ref.VOXEL_CASES), "every case repeats a subject"
    assert {ref.scalenorm_bwd_register_kernel(c["D"]) for c in ref.SCALENORM_CASES} == {True, False}
    assert {(c["raw"], c["rs"], c["M"]) for c in ref.FF_CASES} >= {(True, True, 70), (False, True, 128), (False, False, 70), (True, False, 128)}
    assert {(c["N"] % 64 == 0, c["H"]) for c in ref.INFONCE_CASES} == {(True, 64), (False, 128), (True, 128), (False, 64)}
