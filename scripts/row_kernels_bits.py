#!/usr/bin/env python3
"""Bits and speed of the one-wave-per-row norm kernels (csrc/row_wave.h), straight through the C entry points.

    TRIBE_HIP_LIB=/path/to/libtribe_hip.so python scripts/row_kernels_bits.py
        one line `case buffer sha256` per output buffer: ScaleNorm forward and backward (tribe_scalenorm_bwd_ordered: dx, dg_rows, dg),
        RMSNorm / LayerNorm / norm + e4m3 quantise, tribe_norm_act_fwd / _bwd once per launch path.  Seeded inputs built like
        tests/test_gpu_reductions.py's (_norm_rows; 37 rows, so the last workgroup has three idle waves), with aligned pointers: every
        kernel template at every NV it is compiled for, and its walk at widths no NV fits.  (A misaligned pointer at a register width
        takes the same walk kernels; that host branch is not run here.)  Two builds compute the same bits on these cases if and only if
        their outputs are equal line for line.

    python scripts/row_kernels_bits.py --bench PARENT.so CHANGE.so
        both libraries in one process, timed in turns on the shapes the project runs: 7 timings each (device events around enough
        launches to fill ~0.2 s) after a warm-up; min / median / max in microseconds per launch.
"""
import ctypes
import hashlib
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "algonauts-2025_amd"))
from tribe_hip import _lib  # noqa: E402  (signatures and dtype codes only; the library under test is opened below)

ROWS = 37
NAMES = ["tribe_scalenorm_fwd", "tribe_rmsnorm_fwd", "tribe_layernorm_fwd", "tribe_norm_quantize_fp8_fwd", "tribe_scalenorm_bwd_ordered",
         "tribe_norm_act_fwd", "tribe_norm_act_bwd", "tribe_norm_act_bwd_workspace_bytes", "tribe_norm_act_path", "tribe_last_error"]


def open_lib(path):
    h = ctypes.CDLL(str(path))
    for name in NAMES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def call(h, name, *args):
    rc = getattr(h, name)(*args, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"{name}: {rc}: {h.tribe_last_error().decode()}")


def p(t):
    return None if t is None else t.data_ptr()


def dt(t):
    return _lib.BF16 if t == torch.bfloat16 else _lib.F32


def norm_rows(dim, seed, rows=ROWS):
    """tests/test_gpu_reductions.py::_norm_rows: row 0 zero, row 3 far below the eps clamps, rows 1-2 at 1e3 + N(0, 1), the rest N(0, 1)
    at scales from 1e-3 to 1e2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g) * torch.logspace(-3, 2, rows)[:, None]
    x[0] = 0
    x[1:3] = 1e3 + torch.randn(2, dim, generator=g)
    x[3] = 1e-9 * torch.randn(dim, generator=g)
    return x


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def nan_like(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=dtype, device="cuda")
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def bits(h):
    out = []
    eps = 1e-5
    for dim in (768, 1024, 3072, 4, 260, 1408, 4096):
        x, g = norm_rows(dim, dim).cuda(), torch.tensor([1.3]).cuda()
        for od in (torch.float32, torch.bfloat16):
            y = nan_like((ROWS, dim), od)
            call(h, "tribe_scalenorm_fwd", x.data_ptr(), ROWS, dim, g.data_ptr(), dim**0.5, eps, y.data_ptr(), dt(od))
            out.append((f"scalenorm_fwd dim={dim} out={od}", "y", sha(y)))
    for dim in (16, 512, 1024, 1028, 1408, 2048, 3072, 3088, 4096):
        x = norm_rows(dim, dim + 1).cuda()
        gen = torch.Generator().manual_seed(dim + 2)
        w = (1.0 + 0.2 * torch.randn(dim, generator=gen)).cuda()
        b = (0.1 * torch.randn(dim, generator=gen)).cuda()
        for kind in ("rms", "ln", "ln_bias"):
            bias = b if kind == "ln_bias" else None
            for od in (torch.float32, torch.bfloat16, torch.uint8):
                if od == torch.uint8 and dim % 16:
                    continue
                y = nan_like((ROWS, dim), od)
                if od == torch.uint8:
                    call(h, "tribe_norm_quantize_fp8_fwd", x.data_ptr(), ROWS, dim, w.data_ptr(), p(bias), int(kind != "rms"), eps, 448 / 2.0,
                         y.data_ptr())
                elif kind == "rms":
                    call(h, "tribe_rmsnorm_fwd", x.data_ptr(), ROWS, dim, w.data_ptr(), eps, y.data_ptr(), dt(od))
                else:
                    call(h, "tribe_layernorm_fwd", x.data_ptr(), ROWS, dim, w.data_ptr(), p(bias), eps, y.data_ptr(), dt(od))
                out.append((f"rowstat {kind} dim={dim} out={od}", "y", sha(y)))
    for dim in (768, 3072, 256, 1000, 1024):
        x, g = norm_rows(dim, dim + 3).cuda(), torch.tensor([1.3]).cuda()
        gen = torch.Generator().manual_seed(dim + 4)
        dy32 = torch.randn(ROWS, dim, generator=gen)
        dres = (2 * torch.randn(ROWS, dim, generator=gen)).cuda()
        rs = (0.5 + torch.rand(dim, generator=gen)).cuda()
        for dyd in (torch.float32, torch.bfloat16):
            dy = dy32.to(dyd).cuda()
            for residual in ("none", "dres", "dres_rs"):
                dx, dg, dg_rows = nan_like((ROWS, dim), torch.float32), nan_like((1,), torch.float32), nan_like((ROWS,), torch.float32)
                call(h, "tribe_scalenorm_bwd_ordered", x.data_ptr(), dy.data_ptr(), dt(dyd), g.data_ptr(), dim**0.5, eps, ROWS, dim,
                     p(dres if residual != "none" else None), p(rs if residual == "dres_rs" else None), dx.data_ptr(), dg.data_ptr(),
                     dg_rows.data_ptr())
                for name, t in (("dx", dx), ("dg_rows", dg_rows), ("dg", dg)):
                    out.append((f"scalenorm_bwd dim={dim} dy={dyd} {residual}", name, sha(t)))
    paths = ("reg4", "reg16", "walk4", "elem")
    for dim, want in ((1000, "reg4"), (2048, "reg16"), (4100, "walk4"), (65, "elem")):
        gen = torch.Generator().manual_seed(1000 * ROWS + dim)
        z = torch.randn(ROWS, dim, generator=gen).cuda()
        gamma, beta = (1.0 + 0.3 * torch.randn(dim, generator=gen)).cuda(), (0.3 * torch.randn(dim, generator=gen)).cuda()
        dy = torch.randn(ROWS, dim, generator=gen).cuda()
        ld = (dim + 63) // 64 * 64
        y, mean, rstd = nan_like((ROWS, ld), torch.bfloat16), nan_like((ROWS,), torch.float32), nan_like((ROWS,), torch.float32)
        got = paths[h.tribe_norm_act_path(z.data_ptr(), dim, dim, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _lib.BF16, ld, None, 0, 0)]
        assert got == want, f"norm_act dim={dim}: path {got}, expected {want}"
        call(h, "tribe_norm_act_fwd", z.data_ptr(), ROWS, dim, dim, gamma.data_ptr(), beta.data_ptr(), eps, 1, _lib.ACT_GELU, y.data_ptr(),
             _lib.BF16, ld, mean.data_ptr(), rstd.data_ptr())
        for name, t in (("y", y), ("mean", mean), ("rstd", rstd)):
            out.append((f"norm_act_fwd {want} dim={dim}", name, sha(t)))
        dz, dgamma, dbeta = nan_like((ROWS, dim), torch.float32), nan_like((dim,), torch.float32), nan_like((dim,), torch.float32)
        nbytes = h.tribe_norm_act_bwd_workspace_bytes(ROWS, dim)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        got = paths[h.tribe_norm_act_path(z.data_ptr(), dim, dim, gamma.data_ptr(), beta.data_ptr(), dz.data_ptr(), _lib.F32, dim, dy.data_ptr(),
                                          _lib.F32, dim)]
        assert got == want, f"norm_act bwd dim={dim}: path {got}, expected {want}"
        call(h, "tribe_norm_act_bwd", dy.data_ptr(), _lib.F32, dim, z.data_ptr(), ROWS, dim, dim, mean.data_ptr(), rstd.data_ptr(),
             gamma.data_ptr(), beta.data_ptr(), 1, _lib.ACT_GELU, dz.data_ptr(), _lib.F32, dim, dgamma.data_ptr(), dbeta.data_ptr(),
             ws.data_ptr(), nbytes)
        for name, t in (("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta)):
            out.append((f"norm_act_bwd {want} dim={dim}", name, sha(t)))
    return out


def bench_cases():
    """name -> launch(h): the shapes the project runs (the bench step's B = 64, T = 1024 residual stream; the extractors' widths)."""
    eps = 1e-5
    cases = {}
    g = torch.tensor([1.3]).cuda()

    def randn(rows, dim, dtype=torch.float32):
        return torch.randn(rows, dim, device="cuda").to(dtype)

    x = randn(65536, 3072)
    for od in (torch.bfloat16, torch.float32):
        y = torch.empty(65536, 3072, dtype=od, device="cuda")
        cases[f"scalenorm_fwd 65536x3072 -> {od}"] = lambda h, y=y, od=od: call(h, "tribe_scalenorm_fwd", x.data_ptr(), 65536, 3072, g.data_ptr(),
                                                                                 3072**0.5, eps, y.data_ptr(), dt(od))
    xb, dres, rs = x[:16384], randn(16384, 3072), torch.rand(3072, device="cuda") + 0.5
    dx, dg, dg_rows = torch.empty(16384, 3072, device="cuda"), torch.zeros(1, device="cuda"), torch.empty(16384, device="cuda")
    for dyd in (torch.bfloat16, torch.float32):
        dy = randn(16384, 3072, dyd)
        cases[f"scalenorm_bwd 16384x3072 dres+rs dy={dyd}"] = lambda h, dy=dy, dyd=dyd: call(
            h, "tribe_scalenorm_bwd_ordered", xb.data_ptr(), dy.data_ptr(), dt(dyd), g.data_ptr(), 3072**0.5, eps, 16384, 3072, dres.data_ptr(),
            rs.data_ptr(), dx.data_ptr(), dg.data_ptr(), dg_rows.data_ptr())
    # the extractors' widths, then LayerNorm's other register forms (NV = 8 and 12, f32 out), then one walk
    for kind, dim in (("ln", 1024), ("ln", 1408), ("rms", 3072), ("e4m3", 3072), ("ln", 2048), ("ln", 3072), ("ln_f32", 1408), ("ln_f32", 3072),
                      ("ln", 4096)):
        xs, w, b = randn(16384, dim), torch.rand(dim, device="cuda") + 0.5, randn(1, dim).view(dim)
        od = torch.uint8 if kind == "e4m3" else (torch.float32 if kind == "ln_f32" else torch.bfloat16)
        y = torch.empty(16384, dim, dtype=od, device="cuda")
        if kind in ("ln", "ln_f32"):
            fn = lambda h, xs=xs, w=w, b=b, y=y, dim=dim, od=od: call(h, "tribe_layernorm_fwd", xs.data_ptr(), 16384, dim, w.data_ptr(), b.data_ptr(),
                                                                      eps, y.data_ptr(), dt(od))
        elif kind == "rms":
            fn = lambda h, xs=xs, w=w, y=y, dim=dim: call(h, "tribe_rmsnorm_fwd", xs.data_ptr(), 16384, dim, w.data_ptr(), eps, y.data_ptr(), _lib.BF16)
        else:
            fn = lambda h, xs=xs, w=w, y=y, dim=dim: call(h, "tribe_norm_quantize_fp8_fwd", xs.data_ptr(), 16384, dim, w.data_ptr(), None, 0, eps,
                                                          64.0, y.data_ptr())
        cases[f"{kind} 16384x{dim}" + (" (walk)" if dim == 4096 else "")] = fn
    return cases


def timed(fn, h, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn(h)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n      # microseconds per launch


def bench(parent_path, change_path):
    libs = {"parent": open_lib(parent_path), "change": open_lib(change_path)}
    torch.manual_seed(0)
    cases = bench_cases()
    for fn in cases.values():                # warm-up of every shape, both libraries
        for h in libs.values():
            timed(fn, h, 3)
    print("# microseconds per launch: min / median / max of 7 timings per library, the libraries timed in turns; ok = the change's median is "
          "at or below the parent's max")
    for name, fn in cases.items():
        n = max(3, int(0.2e6 / timed(fn, libs["parent"], 5)))
        t = {k: [] for k in libs}
        for _ in range(7):
            for k, h in libs.items():
                t[k].append(timed(fn, h, n))
        s = {k: sorted(v) for k, v in t.items()}
        ok = s["change"][3] <= s["parent"][6]
        print(f"{name}: n={n}  parent {s['parent'][0]:.1f} / {s['parent'][3]:.1f} / {s['parent'][6]:.1f}  change {s['change'][0]:.1f} / "
              f"{s['change'][3]:.1f} / {s['change'][6]:.1f}  {'ok' if ok else 'SLOWER'}", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs an MI355X"
    if len(sys.argv) == 4 and sys.argv[1] == "--bench":
        bench(sys.argv[2], sys.argv[3])
    else:
        for case, buf, digest in bits(open_lib(os.environ.get("TRIBE_HIP_LIB", _lib.LIB_PATH))):
            print(f"{case} {buf} {digest}", flush=True)
