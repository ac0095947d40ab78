"""Diagnostic: libtribe_hip_stamps.so = the library with -DTRIBE_GEMM_STAMPS in the 8-wave 256 x 256 GEMM (gemm_8wave_nb4.hip; every
other object as `make` left it in csrc/).  Prints, for the four encoder GEMMs at their B = 64 shapes and with their model operators,
where a wave's time goes: the K loop by slot (shares), and per tile the cycles from kernel entry to the first K-loop iteration, from
the loop's end to the last store issued, and to the last store retired (wave end) -- once through the role-compiled epilogue and once
through the generic one (tile_hint 6).  `--build-only` builds the library (no GPU needed); without it an existing ab_tmp/ library that is
newer than the sources is used as it is.  Never a timing run: the stamps serialise the schedule; read the SHARES and the per-tile cycles."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CS = ROOT / "algonauts-2025_amd" / "csrc"
out = ROOT / "ab_tmp" / "libtribe_hip_stamps.so"
out.parent.mkdir(exist_ok=True)
srcs = [CS / "gemm_8wave_nb4.hip", CS / "gemm_8wave.h", CS / "gemm_launch.h", CS / "gemm_common.h", CS / "common.h", ROOT / "include" / "tribe_hip.h"]
if not out.exists() or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
    others = sorted(o for o in CS.glob("*.o") if o.name != "gemm_8wave_nb4.o")
    assert any(o.name == "gemm_8wave_nb3.o" for o in others), "run `make` in csrc/ first: the other objects are linked as they are"
    obj = out.parent / "gemm_stamps.o"
    hipcc = ["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950"]
    subprocess.run([*hipcc, "-DTRIBE_GEMM_STAMPS", "-c", str(CS / "gemm_8wave_nb4.hip"), "-o", str(obj)], check=True)
    subprocess.run([*hipcc[:1], "-shared", "-fPIC", "--offload-arch=gfx950", str(obj), *map(str, others), "-o", str(out)], check=True)
if "--build-only" in sys.argv:
    sys.exit(0)
os.environ["TRIBE_HIP_LIB"] = str(out)
sys.path[:0] = [str(ROOT), str(ROOT / "algonauts-2025_amd")]
import torch  # noqa: E402
from tribe_hip import _lib  # noqa: E402

dev = torch.device("cuda")
M, DIM, FF = 16384, 3072, 12288
SHAPES = {"qkv": (3 * DIM, DIM), "ff1": (FF, DIM), "out_proj": (DIM, DIM), "ff2": (DIM, FF)}
names = ["lds_reads", "stage+vmcnt", "barrier1", "mfma", "barrier2"]
torch.manual_seed(0)
for role, (N, K) in SHAPES.items():
    a = torch.randn(M, K, device=dev).bfloat16()
    b = (torch.randn(N, K, device=dev) / K**0.5).bfloat16()
    bias, rs, scale = torch.randn(N, device=dev), torch.rand(N, device=dev) + 0.5, torch.rand(M, device=dev) + 0.5
    ntiles = (M // 256) * (N // 256)
    for hint, label in ((2, "role epilogue"), (6, "generic epilogue")):
        dbg = torch.zeros(ntiles * 8 * 8, dtype=torch.int64, device=dev)
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.batch1, d.batch0 = M, N, K, 1, 1
        d.A, d.lda, d.B, d.ldb = a.data_ptr(), K, b.data_ptr(), K
        d.alpha, d.tile_hint, d.role = 1.0, hint, _lib.ROLE[role]
        if role in ("qkv", "ff1"):
            o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            d.C, d.ldc, d.c_dtype, d.row_scale = o.data_ptr(), N, _lib.BF16, scale.data_ptr()
            if role == "ff1":
                d.bias, d.bias_mode, d.act = bias.data_ptr(), _lib.BIAS_COL, _lib.ACT_GELU
        else:
            o = torch.randn(M, N, device=dev)
            xb, ssq = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N // 64, device=dev)
            d.C, d.ldc, d.c_dtype, d.res, d.ldres, d.res_scale = o.data_ptr(), N, _lib.F32, o.data_ptr(), N, rs.data_ptr()
            d.c_bf16, d.ld_c_bf16, d.row_sumsq, d.ld_row_sumsq = xb.data_ptr(), N, ssq.data_ptr(), N // 64
            if role == "ff2":
                d.bias, d.bias_mode = bias.data_ptr(), _lib.BIAS_COL
        d.gadd_index = dbg.data_ptr()   # the side buffer (desc.gadd stays NULL)
        assert _lib.lib().tribe_gemm_epilogue_path(C.byref(d)) == (1 if hint == 2 else 0)
        for _ in range(3):
            _lib.check(_lib.lib().tribe_gemm_bf16(C.byref(d), torch.cuda.current_stream().cuda_stream), "gemm")
        torch.cuda.synchronize()
        t = dbg.view(ntiles, 8, 8).double().cpu()
        nk = K // 64
        for grp, sl in (("wr=0", slice(0, 4)), ("wr=1", slice(4, 8))):
            m = t[:, sl, :5].mean(dim=(0, 1))
            tot = m.sum()
            e = t[:, sl, 5:].mean(dim=(0, 1))
            p90 = t[:, sl, 5:].flatten(0, 1).quantile(0.9, dim=0)
            print(f"{role:8s} {label:16s} {grp}: K loop {tot:9.0f} cycles/tile ({tot / nk:7.1f} per K-tile: "
                  + "  ".join(f"{n} {v / tot * 100:4.1f}%" for n, v in zip(names, m))
                  + f")  entry->loop {e[0]:7.0f}  loop end->last store issued {e[1]:7.0f} (p90 {p90[1]:7.0f})  ->wave end {e[2]:7.0f} (p90 {p90[2]:7.0f})")
