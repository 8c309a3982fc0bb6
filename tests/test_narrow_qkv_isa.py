"""CPU (needs hipcc, which cross-compiles gfx950 without a GPU): the resources of the narrow-tile QKV GEMM (csrc/gemm.hip: gemm_nqkv_kernel), read from the compiled
code object's metadata as tests/test_narrow_gemm_isa.py and tests/test_narrow_lo6_isa.py read their kernels': exactly six instantiations -- <DT, SPLIT, LO6> for fp16
and bf16 without (LO6 and not SPLIT) --, no spilled VGPR, no scratch, at most 64 KiB of LDS (two workgroups per CU), 256 threads -- and both older narrow kernels'
names and every gemm_kernel instantiation are still there.  Register, scratch and LDS figures only."""
import os
import re

import pytest

import gemm_isa
from test_narrow_gemm_isa import WIDE

pytestmark = pytest.mark.skipif(not os.path.exists(gemm_isa.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def metadata():
    return gemm_isa.metadata()


def test_narrow_qkv_kernel_resources(metadata):
    names = {}
    for n in metadata:
        m = re.fullmatch(r"_Z16gemm_nqkv_kernelILi([01])ELb([01])ELb([01])EEv10GemmParams", n)
        if m:
            names[tuple(int(x) for x in m.groups())] = n
    want = {(dt, split, lo6) for dt in (0, 1) for split, lo6 in ((0, 0), (1, 0), (1, 1))}
    assert set(names) == want, sorted(metadata)
    assert len([n for n in metadata if "gemm_nqkv_kernel" in n]) == 6
    for key, n in sorted(names.items()):
        m = metadata[n]
        print("NARROW_QKV_ISA", n, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)             # no scratch
        assert 0 < m["group_segment_fixed_size"] <= 65536, (n, m)       # LDS: at least two workgroups share a CU's 160 KiB
        assert m["max_flat_workgroup_size"] == 256, (n, m)


def test_the_older_kernels_are_all_still_there(metadata):
    assert len([n for n in metadata if re.fullmatch(r"_Z18gemm_narrow_kernelILi[01]EEv10GemmParams", n)]) == 2, sorted(metadata)
    assert len([n for n in metadata if re.fullmatch(r"_Z22gemm_narrow_lo6_kernelILi[01]EEv10GemmParams", n)]) == 2, sorted(metadata)
    assert len([n for n in metadata if "gemm_narrow_lo6_kernel" in n]) == 2 and len([n for n in metadata if "gemm_narrow_kernel" in n]) == 2
    have = set()
    for n in metadata:
        m = re.fullmatch(r"_Z11gemm_kernelILi(\d)ELi(\d)ELb([01])ELb([01])EEv10GemmParams", n)
        if m:
            have.add(tuple(int(x) for x in m.groups()))
    assert WIDE <= have, sorted(WIDE - have)
