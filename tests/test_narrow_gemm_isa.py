"""CPU (needs hipcc, which cross-compiles gfx950 without a GPU): the resources of the narrow-tile residual GEMM (csrc/gemm.hip: gemm_narrow_kernel), read from the
compiled code object's metadata as tests/test_isa_guards.py reads its kernels': no spilled VGPR, no scratch, at most 64 KiB of LDS (two workgroups per CU), 256
threads -- and every gemm_kernel instantiation that existed before the narrow kernel is still there.  Register, scratch and LDS figures only."""
import os
import re

import pytest

import gemm_isa

pytestmark = pytest.mark.skipif(not os.path.exists(gemm_isa.HIPCC), reason="hipcc not installed")

# gemm_kernel<EPI, DT, SPLIT, MXA> as launch_t instantiates them (gemm.hip): the plain kernels of six epilogues x three dtypes, the split (hi | lo) outputs of the
# three 16-bit epilogues, the e2m3 second pass (plain outputs: RESID, SWIGLU, LSE; split outputs: QKV, SWIGLU) and the fp8 down projection with an MX-scaled A
WIDE = ({(e, d, 0, 0) for e in range(6) for d in range(3)} | {(e, d, 1, 0) for e in (0, 3, 4) for d in (0, 1)}
        | {(e, d, 0, 1) for e in (2, 4, 5) for d in (0, 1)} | {(e, d, 1, 1) for e in (3, 4) for d in (0, 1)} | {(2, 2, 0, 1)})


@pytest.fixture(scope="module")
def metadata():
    return gemm_isa.metadata()


def test_narrow_kernel_resources(metadata):
    names = [n for n in metadata if re.fullmatch(r"_Z18gemm_narrow_kernelILi[01]EEv10GemmParams", n)]
    assert len(names) == 2, sorted(metadata)                            # bf16 and fp16
    for n in names:
        m = metadata[n]
        print("NARROW_ISA", n, m)
        assert m["vgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)             # no scratch
        assert 0 < m["group_segment_fixed_size"] <= 65536, (n, m)       # LDS: at least two workgroups share a CU's 160 KiB
        assert m["max_flat_workgroup_size"] == 256, (n, m)


def test_the_wide_kernels_are_all_still_there(metadata):
    have = set()
    for n in metadata:
        m = re.fullmatch(r"_Z11gemm_kernelILi(\d)ELi(\d)ELb([01])ELb([01])EEv10GemmParams", n)
        if m:
            have.add(tuple(int(x) for x in m.groups()))
    assert WIDE <= have, sorted(WIDE - have)
