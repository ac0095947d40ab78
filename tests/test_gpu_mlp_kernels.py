"""GPU: tribe_norm_act_fwd / tribe_norm_act_bwd (csrc/mlp.hip) per element against float64 on the CPU, on every launch branch.

Bounds (derived, none fitted; e = 2^-24, one f32 rounding).  The only measured figures are the errors of the device's erff / expf /
expm1f inside the activation and its derivative, which cannot be derived: each was measured once against float64 on these very inputs
(`measure_activation_errors`) and twice the measured maximum is allowed (E_ACT, E_DACT below).

forward, f32 output.  The kernel forms the row statistics as f64 sums of the widened inputs (their error, < 1e-12 relative at these
  sizes, is ignored) and rounds mean and rstd to f32 once each; then per element d = z - mean, zh = d * rstd, u = fma(zh, gamma, beta),
  one rounding each.  The rounding of mean moves d by e |mean|, its own rounding by e |d|; rstd's rounding and the product add 2 e |zh|:
  |zh - zh64| <= e rstd (3 |z - mean| + |mean|), and the fma adds e |u|:
      |du| <= c e (|gamma| rstd (|z - mean| + |mean|) + |u|),   c = 3 by this count, 4 allowed for the second-order products
      |dy| <= L |du| + E_ACT ulp(max(|y|, |u|)),   L = 1 (ReLU, ELU, none: ReLU and none add nothing of their own) or 1.13 (GELU)
  Without a norm u = z exactly, so ReLU and identity are exact.
forward, bf16 output: the bits of y_f32.bfloat16(); pad columns exactly 0 (both dtypes).
stats: mean and rstd within 2^-23 relative of float64.
backward.  The float64 reference starts from the kernel's own f32 inputs -- dy, z, gamma, beta AND the saved f32 mean and rstd -- so
  here zh carries two roundings only, dzh_ = 2 e |zh|, and du_ = |gamma| dzh_ + e |u|.  With act' off by at most
  a = |dy| (L2 du_ + E_DACT e)  (L2 = max |act''|: 0.8 GELU, 1 ELU, 0 otherwise), du = dy act'(u) and dzh = du gamma one rounding each,
  the error of dzh is at most g = |gamma| a + 2 e |dzh|.  m1 = mean_H(dzh), m2 = mean_H(dzh zh) are f64 sums rounded once, then
  dz = rstd * fma(-zh, m2, dzh - m1): three more roundings.  Counting the e-terms on |dzh| (5), |m1| (4) and |zh m2| (5):
      |ddz| <= c' e rstd (|dzh| + |m1| + |zh m2|) + A,   c' = 5 by this count, 6 allowed for the second-order products
      A = rstd (|gamma| a + mean_H(g) + |zh| mean_H(g |zh| + |dzh| dzh_))
  A is the activation-derivative term together with the row means of ABSOLUTE errors, which the signed means m1, m2 do not bound.
  Without a norm dz = du: |ddz| <= |dy| E_DACT e + e |du|.
      |ddgamma| <= c'' e sum_rows |du zh| + sum_rows a |zh|,  |ddbeta| <= c'' e sum_rows |du| + sum_rows a,   c'' = 4
  (du's rounding 1, zh 2, the final f32 rounding of the f64 column sum 1; dbeta needs 2).
ReLU: an element whose float64 |u| is below the forward bound on du may carry the other mask on the device.  Such elements are left
  out of the dz comparison (at most 0.1 % of a case, else the test fails); what a flipped mask does to the rest of its row through the
  two means, (|dy gamma| + |zh| |dy gamma zh|) rstd / H, and to its column's sums, |dy zh| and |dy|, is added to those bounds.
bf16 dy / dz: the bits of the f32 run on the widened dy, rounded to nearest even; dgamma / dbeta bit-equal.
determinism: the backward run twice gives equal bits in dz, dgamma, dbeta.

Measured (MI355X, these inputs), in the units used above: E_ACT gelu 1.527 ulp, elu 0.882 ulp; E_DACT gelu 2.371 e, elu 0.831 e.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E = 2.0 ** -24
EPS = 1e-5
C_FWD, C_BWD, C_COL = 4, 6, 4
LIP = {"gelu": 1.13, "relu": 1.0, "elu": 1.0, None: 1.0}
LIP2 = {"gelu": 0.8, "relu": 0.0, "elu": 1.0, None: 0.0}
# twice the measured maxima (module docstring): ulps of max(|y|, |u|) forward, units of 2^-24 (|act'| <= 1.13) backward
E_ACT = {"gelu": 2 * 1.527, "relu": 0.0, "elu": 2 * 0.882, None: 0.0}
E_DACT = {"gelu": 2 * 2.371, "relu": 0.0, "elu": 2 * 0.831, None: 0.0}

ROWS = [1, 3, 64, 257]
# dim -> launch branch with 16-byte friendly pointers and pitches (tribe_norm_act_path); 2048 and 4096 added for "reg16" and its edge
DIMS = {1: "elem", 2: "elem", 63: "elem", 64: "reg4", 65: "elem", 200: "reg4", 1000: "reg4", 1024: "reg4", 1025: "elem", 2048: "reg16",
        4096: "reg16", 4100: "walk4"}
LAYOUTS = ["tight", "pad64", "off1"]          # ld == dim; ld padded to 64; base pointer one element off 16-byte alignment
ACTS = ["gelu", "relu", "elu", None]
DISTS = ["n01", "shift10"]                    # z ~ N(0, 1); z ~ 10 + N(0, 1): cancellation in z - mean
GUARD = 8


def _ops():
    from tribe_hip import ops

    return ops


@functools.lru_cache(maxsize=4)
def _inputs(rows, dim, dist):
    """CPU f32 inputs of a case; computed once, never modified."""
    g = torch.Generator().manual_seed(1000 * rows + dim + (7 if dist == "shift10" else 0))
    z = torch.randn(rows, dim, generator=g) + (10.0 if dist == "shift10" else 0.0)
    gamma = 1.0 + 0.3 * torch.randn(dim, generator=g)
    beta = 0.3 * torch.randn(dim, generator=g)
    dy = torch.randn(rows, dim, generator=g)
    return z, gamma, beta, dy


def act64(act, u):
    if act == "gelu":
        return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    if act == "relu":
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == "elu":
        return torch.where(u > 0, u, torch.expm1(u))
    return u


def dact64(act, u):
    if act == "gelu":
        return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    if act == "relu":
        return (u > 0).to(u.dtype)
    if act == "elu":
        return torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    return torch.ones_like(u)


def ulp(v):
    """Spacing of f32 at |v| (float64 tensor), 2^(floor(log2 |v|) - 23); the smallest normal's spacing below it."""
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), ex - 24)


def _ld(dim, layout):
    return (dim + 63) // 64 * 64 if layout == "pad64" else dim


def _place(t, layout, dtype=torch.float32):
    """GPU copy of CPU [rows, dim] in the layout: a [rows, dim] view with contiguous rows of pitch ld; pad columns hold 7."""
    rows, dim = t.shape
    ld, off = _ld(dim, layout), int(layout == "off1")
    buf = torch.full((off + rows * ld + GUARD,), 7.0, dtype=dtype, device="cuda")
    view = buf[off:off + rows * ld].view(rows, ld)[:, :dim]
    view.copy_(t)
    if layout == "off1":
        assert view.data_ptr() % 16 == buf.element_size()
    return view


def _out(rows, dim, layout, dtype):
    """(buffer, contiguous [rows, ld] output inside it): the buffer holds -3 around and inside the output."""
    ld, off = _ld(dim, layout), int(layout == "off1")
    buf = torch.full((off + rows * ld + GUARD,), -3.0, dtype=dtype, device="cuda")
    return buf, buf[off:off + rows * ld].view(rows, ld)


def _guards_intact(buf, rows, ld, layout):
    off = int(layout == "off1")
    return bool((buf[:off] == -3).all()) and bool((buf[off + rows * ld:] == -3).all())


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def ref_forward(z, gamma, beta, norm, act):
    """float64 forward from the f32 inputs: dict of u, y, mean, rstd, zh and the forward bound on du."""
    z64, g, b = z.double(), gamma.double(), beta.double()
    if norm:
        mean = z64.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((z64 - mean) ** 2).mean(1, keepdim=True) + float(torch.tensor(EPS, dtype=torch.float32)))
        zh = (z64 - mean) * rstd
        u = zh * g + b
        du = C_FWD * E * (g.abs() * rstd * ((z64 - mean).abs() + mean.abs()) + u.abs())
    else:
        mean = rstd = None
        zh, u, du = torch.zeros_like(z64), z64, torch.zeros_like(z64)
    return {"u": u, "y": act64(act, u), "mean": mean, "rstd": rstd, "zh": zh, "du_bound": du}


def forward_bound(ref, act):
    return LIP[act] * ref["du_bound"] + E_ACT[act] * ulp(torch.maximum(ref["y"].abs(), ref["u"].abs()))


def run_forward(z, gamma, beta, norm, act, layout, dtype, want_stats=True):
    ops = _ops()
    rows, dim = z.shape
    zg = _place(z, layout)
    buf, out = _out(rows, dim, layout, dtype)
    y, mean, rstd = ops.norm_act(zg, gamma.cuda(), beta.cuda(), EPS, act, norm=norm, out=out, want_stats=want_stats)
    torch.cuda.synchronize()
    assert _guards_intact(buf, rows, out.shape[1], layout), "the kernel wrote outside its output"
    return y, mean, rstd, ops.norm_act_path(zg, gamma.cuda() if norm else None, beta.cuda() if norm else None, out)


def _expected_path(dim, layout):
    return "elem" if layout == "off1" else DIMS[dim]


@pytest.mark.parametrize("dim", list(DIMS))
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dist", DISTS)
def test_forward(dist, rows, dim):
    z, gamma, beta, _ = _inputs(rows, dim, dist)
    for norm in (True, False):
        for act in ACTS:
            ref = ref_forward(z, gamma, beta, norm, act)
            bound = forward_bound(ref, act)
            for layout in LAYOUTS:
                tag = f"rows={rows} dim={dim} {dist} norm={norm} act={act} {layout}"
                y32, mean, rstd, path = run_forward(z, gamma, beta, norm, act, layout, torch.float32)
                assert path == _expected_path(dim, layout), f"{tag}: branch {path}"
                got = y32[:, :dim].double().cpu()
                err = (got - ref["y"]).abs()
                assert bool((err <= bound).all()), f"{tag}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
                assert bool((y32[:, dim:] == 0).all()), f"{tag}: f32 pad columns are not zero"
                if norm:
                    for name, dev, want in (("mean", mean, ref["mean"]), ("rstd", rstd, ref["rstd"])):
                        rel = (dev.double().cpu() - want[:, 0]).abs() / want[:, 0].abs().clamp_min(1e-300)
                        assert float(rel.max()) <= 2.0 ** -23, f"{tag}: {name} off by {float(rel.max()):.3e} relative"
                else:
                    assert mean is None and rstd is None
                y16, _, _, path16 = run_forward(z, gamma, beta, norm, act, layout, torch.bfloat16, want_stats=False)
                assert path16 == path
                assert _same_bits(y16[:, :dim], y32[:, :dim].bfloat16()), f"{tag}: bf16 output is not the rounded f32 output"
                assert bool((y16[:, dim:] == 0).all()), f"{tag}: bf16 pad columns are not zero"


@pytest.mark.parametrize("act", ACTS)
def test_dim_one_is_act_of_beta(act):
    """dim == 1: zh == 0 exactly (the f64 mean of one value is that value), hence y == act(beta) up to E_ACT."""
    z, gamma, beta, _ = _inputs(64, 1, "shift10")
    y, mean, rstd, _ = run_forward(z, gamma, beta, True, act, "tight", torch.float32)
    want = act64(act, beta.double()).expand(64, 1)
    tol = E_ACT[act] * ulp(torch.maximum(want.abs(), beta.double().abs().expand(64, 1)))
    assert bool(((y.double().cpu() - want).abs() <= tol).all())
    assert torch.equal(mean.cpu(), z[:, 0])
    assert bool(((rstd.double().cpu() - 1.0 / math.sqrt(float(torch.tensor(EPS, dtype=torch.float32)))).abs() <= 2.0 ** -23 / math.sqrt(EPS)).all())


def ref_backward(dy, z, mean, rstd, gamma, beta, norm, act):
    """float64 backward from the kernel's f32 inputs and the bounds of the module docstring."""
    dy64, z64, g, b = dy.double(), z.double(), gamma.double(), beta.double()
    if not norm:
        u = z64
        du = dy64 * dact64(act, u)
        return {"dz": du, "dz_bound": dy64.abs() * E_DACT[act] * E + E * du.abs(), "skip": torch.zeros_like(u, dtype=torch.bool)}
    m, r = mean.double()[:, None], rstd.double()[:, None]
    zh = (z64 - m) * r
    u = zh * g + b
    du = dy64 * dact64(act, u)
    dzh = du * g
    m1, m2 = dzh.mean(1, keepdim=True), (dzh * zh).mean(1, keepdim=True)
    dz = r * (dzh - m1 - zh * m2)
    zh_e = 2 * E * zh.abs()
    a = dy64.abs() * (LIP2[act] * (g.abs() * zh_e + E * u.abs()) + E_DACT[act] * E)
    ge = g.abs() * a + 2 * E * dzh.abs()
    dz_bound = C_BWD * E * r * (dzh.abs() + m1.abs() + (zh * m2).abs()) + \
        r * (g.abs() * a + ge.mean(1, keepdim=True) + zh.abs() * (ge * zh.abs() + dzh.abs() * zh_e).mean(1, keepdim=True))
    dg_bound = C_COL * E * (du * zh).abs().sum(0) + (a * zh.abs()).sum(0)
    db_bound = C_COL * E * du.abs().sum(0) + a.sum(0)
    skip = torch.zeros_like(u, dtype=torch.bool)
    if act == "relu":   # elements whose mask the device may have decided the other way
        skip = u.abs() < C_FWD * E * (g.abs() * r * ((z64 - m).abs() + m.abs()) + u.abs())
        flip = skip * (dy64 * g).abs()
        dz_bound = dz_bound + r * (flip.sum(1, keepdim=True) + zh.abs() * (flip * zh.abs()).sum(1, keepdim=True)) / z.shape[1]
        dg_bound = dg_bound + (skip * (dy64 * zh).abs()).sum(0)
        db_bound = db_bound + (skip * dy64.abs()).sum(0)
    return {"dz": dz, "dz_bound": dz_bound, "dgamma": (du * zh).sum(0), "dbeta": du.sum(0), "dg_bound": dg_bound, "db_bound": db_bound,
            "skip": skip}


def run_backward(dy, z, mean, rstd, gamma, beta, norm, act, layout, dy_dtype, dz_dtype):
    ops = _ops()
    rows, dim = z.shape
    zg, dyg = _place(z, layout), _place(dy, layout, dy_dtype)
    buf, out = _out(rows, dim, layout, dz_dtype)
    dz, dgamma, dbeta = ops.norm_act_bwd(dyg, zg, mean, rstd, gamma.cuda(), beta.cuda(), act, norm=norm, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf, rows, out.shape[1], layout), "the kernel wrote outside its output"
    return dz, dgamma, dbeta, ops.norm_act_path(zg, gamma.cuda() if norm else None, beta.cuda() if norm else None, out, dy=dyg)


@pytest.mark.parametrize("dim", list(DIMS))
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dist", DISTS)
def test_backward(dist, rows, dim):
    z, gamma, beta, dy = _inputs(rows, dim, dist)
    dy_r = dy.bfloat16().float()               # a gradient that bf16 holds exactly, for the bf16 dy / dz runs
    for norm in (True, False):
        mean = rstd = None
        if norm:                               # the statistics the forward kernel saves (checked in test_forward)
            _, mean, rstd = _ops().norm_act(z.cuda(), gamma.cuda(), beta.cuda(), EPS, None, norm=True, want_stats=True)
        for act in ACTS:
            ref = ref_backward(dy, z, None if mean is None else mean.cpu(), None if rstd is None else rstd.cpu(), gamma, beta, norm, act)
            n_skip = int(ref["skip"].sum())
            assert n_skip <= 1e-3 * rows * dim, f"{n_skip} of {rows * dim} elements left out"
            for layout in LAYOUTS:
                tag = f"rows={rows} dim={dim} {dist} norm={norm} act={act} {layout}"
                dz, dgamma, dbeta, path = run_backward(dy, z, mean, rstd, gamma, beta, norm, act, layout, torch.float32, torch.float32)
                assert path == _expected_path(dim, layout), f"{tag}: branch {path}"
                err = (dz[:, :dim].double().cpu() - ref["dz"]).abs()
                ok = (err <= ref["dz_bound"]) | ref["skip"]
                assert bool(ok.all()), f"{tag}: dz max err / bound {float((err / ref['dz_bound'].clamp_min(1e-300))[~ref['skip']].max()):.3f}"
                assert bool((dz[:, dim:] == 0).all()), f"{tag}: dz pad columns are not zero"
                if norm:
                    for name, dev, want, bound in (("dgamma", dgamma, ref["dgamma"], ref["dg_bound"]), ("dbeta", dbeta, ref["dbeta"], ref["db_bound"])):
                        cerr = (dev.double().cpu() - want).abs()
                        assert bool((cerr <= bound).all()), f"{tag}: {name} max err / bound {float((cerr / bound.clamp_min(1e-300)).max()):.3f}"
                else:
                    assert dgamma is None and dbeta is None
                again = run_backward(dy, z, mean, rstd, gamma, beta, norm, act, layout, torch.float32, torch.float32)
                assert _same_bits(dz, again[0]) and (not norm or (_same_bits(dgamma, again[1]) and _same_bits(dbeta, again[2]))), \
                    f"{tag}: two runs differ"
                # bf16 in and out: the f32 run on the same (widened) gradient, rounded once
                w32 = run_backward(dy_r, z, mean, rstd, gamma, beta, norm, act, layout, torch.float32, torch.float32)
                b16 = run_backward(dy_r, z, mean, rstd, gamma, beta, norm, act, layout, torch.bfloat16, torch.bfloat16)
                assert _same_bits(b16[0][:, :dim], w32[0][:, :dim].bfloat16()), f"{tag}: bf16 dz is not the rounded f32 dz"
                assert bool((b16[0][:, dim:] == 0).all())
                assert not norm or (_same_bits(b16[1], w32[1]) and _same_bits(b16[2], w32[2])), f"{tag}: bf16 dy changes dgamma / dbeta"


def test_more_than_one_column_partial_and_large_pitch():
    """130 rows = three partials of the column sums (64 rows each) summed in order; pitch far above dim."""
    ops = _ops()
    z, gamma, beta, dy = _inputs(130, 200, "n01")
    wide = torch.full((130, 1024), 7.0, device="cuda")
    wide[:, :200] = z.cuda()
    zg = wide[:, :200]
    y, mean, rstd = ops.norm_act(zg, gamma.cuda(), beta.cuda(), EPS, "gelu", want_stats=True, out_dtype=torch.float32, ld_out=256)
    ref = ref_forward(z, gamma, beta, True, "gelu")
    assert bool(((y[:, :200].double().cpu() - ref["y"]).abs() <= forward_bound(ref, "gelu")).all()) and bool((y[:, 200:] == 0).all())
    dz, dgamma, dbeta = ops.norm_act_bwd(dy.cuda(), zg, mean, rstd, gamma.cuda(), beta.cuda(), "gelu")
    rb = ref_backward(dy, z, mean.cpu(), rstd.cpu(), gamma, beta, True, "gelu")
    assert bool(((dz.double().cpu() - rb["dz"]).abs() <= rb["dz_bound"]).all())
    assert bool(((dgamma.double().cpu() - rb["dgamma"]).abs() <= rb["dg_bound"]).all())
    assert bool(((dbeta.double().cpu() - rb["dbeta"]).abs() <= rb["db_bound"]).all())


def test_argument_errors():
    ops = _ops()
    z = torch.zeros(4, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.norm_act(z, None, None, EPS, "prelu")
    with pytest.raises(ValueError):
        ops.norm_act(z, torch.ones(7, device="cuda"), None, EPS, "gelu")
    with pytest.raises(ValueError):
        ops.norm_act(z.t(), None, None, EPS, "gelu")


def measure_activation_errors():
    """The measured figures of the module docstring: max error of the device's activation in ulps of max(|y|, |u|) and of its derivative
    in units of 2^-24, over every input set of this module (norm off, so that u = z exactly) and over u = gamma * zh + beta."""
    ops = _ops()
    out = {}
    for act in ("gelu", "elu"):
        worst_f = worst_b = 0.0
        for rows, dim in ((257, 4100), (257, 1024), (64, 1000)):
            for dist in DISTS:
                z, gamma, beta, _ = _inputs(rows, dim, dist)
                u_norm = ref_forward(z, gamma, beta, True, None)["u"].float()
                for u in (z, u_norm):
                    y, _, _ = ops.norm_act(u.cuda(), None, None, EPS, act, norm=False, out_dtype=torch.float32, ld_out=dim)
                    y64 = act64(act, u.double())
                    worst_f = max(worst_f, float(((y.double().cpu() - y64).abs() / ulp(torch.maximum(y64.abs(), u.double().abs()))).max()))
                    dz, _, _ = ops.norm_act_bwd(torch.ones(rows, dim, device="cuda"), u.cuda(), None, None, None, None, act, norm=False)
                    worst_b = max(worst_b, float((dz.double().cpu() - dact64(act, u.double())).abs().max()) / E)
        out[act] = (worst_f, worst_b)
    return out
