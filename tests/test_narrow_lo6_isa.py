"""CPU (needs hipcc, which cross-compiles gfx950 without a GPU): the resources of the narrow-tile residual GEMM with the e2m3 second pass (csrc/gemm.hip:
gemm_narrow_lo6_kernel), read from the compiled code object's metadata as tests/test_narrow_gemm_isa.py reads its kernel's: exactly two instantiations, no spilled
VGPR, no scratch, at most 64 KiB of LDS (two workgroups per CU), 256 threads -- and the plain narrow kernel's two names and every gemm_kernel instantiation are
still there.  Register, scratch and LDS figures only."""
import os
import re

import pytest

import gemm_isa
from test_narrow_gemm_isa import WIDE

pytestmark = pytest.mark.skipif(not os.path.exists(gemm_isa.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def metadata():
    return gemm_isa.metadata()


def test_narrow_lo6_kernel_resources(metadata):
    names = [n for n in metadata if re.fullmatch(r"_Z22gemm_narrow_lo6_kernelILi[01]EEv10GemmParams", n)]
    assert len(names) == 2, sorted(metadata)                            # bf16 and fp16
    assert len([n for n in metadata if "gemm_narrow_lo6_kernel" in n]) == 2
    for n in names:
        m = metadata[n]
        print("NARROW_LO6_ISA", n, m)
        assert m["vgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)             # no scratch
        assert 0 < m["group_segment_fixed_size"] <= 65536, (n, m)       # LDS: at least two workgroups share a CU's 160 KiB
        assert m["max_flat_workgroup_size"] == 256, (n, m)


def test_the_older_kernels_are_all_still_there(metadata):
    assert len([n for n in metadata if re.fullmatch(r"_Z18gemm_narrow_kernelILi[01]EEv10GemmParams", n)]) == 2, sorted(metadata)
    have = set()
    for n in metadata:
        m = re.fullmatch(r"_Z11gemm_kernelILi(\d)ELi(\d)ELb([01])ELb([01])EEv10GemmParams", n)
        if m:
            have.add(tuple(int(x) for x in m.groups()))
    assert WIDE <= have, sorted(WIDE - have)
