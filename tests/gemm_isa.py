"""What the narrow-tile ISA tests (test_narrow_gemm_isa.py, test_narrow_lo6_isa.py, test_narrow_qkv_isa.py) read: csrc/gemm.hip compiled for gfx950 -- hipcc
cross-compiles without a GPU -- and the resource metadata of every kernel in it.  One compile per process, shared by the three modules."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blim_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def metadata():
    """{mangled kernel name: {field: int}} of gemm.hip compiled for gfx950."""
    with tempfile.TemporaryDirectory(prefix="gemm_isa") as tmp:
        out = os.path.join(tmp, "gemm.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(CSRC, "gemm.hip"), "-o", out],
                       check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|max_flat_workgroup_size|vgpr_count):\s+(\d+)", blk)}
    return meta
