"""Build-time audit (csrc/Makefile): no kernel of the given object files may use scratch (private_segment_fixed_size > 0 = the register
allocator spilled).  A fused-epilogue experiment of round 3 silently cost the bf16 GEMM kernels 84 bytes per lane this way.
Usage: python3 scripts/check_no_scratch.py [--arch gfx950] gemm.o gemm_8wave_nb4.o ...
The architecture comes from --arch, else from ARCH in the environment, else gfx950; the LLVM tools from the ROCm root of HIPCC (default
/opt/rocm/bin/hipcc).  Each object is copied into a temporary directory and unbundled there (llvm-objdump --offloading writes next to
its input), so nothing is written beside the objects."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

args = sys.argv[1:]
arch = os.environ.get("ARCH", "gfx950")
if "--arch" in args:
    i = args.index("--arch")
    arch = args[i + 1]
    del args[i:i + 2]
hipcc = shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) or "/opt/rocm/bin/hipcc"
LLVM = Path(hipcc).resolve().parent.parent / "lib" / "llvm" / "bin"
bad = []
total = 0
for obj in args:
    with tempfile.TemporaryDirectory() as tmp:
        copy = Path(shutil.copy(obj, tmp))
        subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", copy.name], cwd=tmp, check=True, capture_output=True)
        # the bundles are named <input>.<n>.<target>
        cos = list(Path(tmp).glob(f"{copy.name}.*.hipv4-amdgcn-amd-amdhsa--{arch}"))
        if not cos:
            sys.exit(f"check_no_scratch: no {arch} code object in {obj}")
        for co in cos:
            notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
            name = None
            for line in notes.splitlines():
                m = re.search(r"\.name:\s+(\S+)", line)
                if m:
                    name = m.group(1)
                m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
                if m:
                    total += 1
                    if int(m.group(1)) > 0:
                        bad.append((obj, name, int(m.group(1))))
if bad:
    for obj, name, size in bad:
        print(f"SCRATCH: {obj}: {name}: {size} bytes per lane", file=sys.stderr)
    sys.exit(1)
print(f"OK: {total} kernels in {len(args)} object(s), none uses scratch")
