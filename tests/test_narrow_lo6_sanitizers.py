"""CPU (-m "not gpu"): the host code of the switches of the narrow-tile residual GEMM with the e2m3 second pass (csrc/engine.hip: option "narrow_lo6", blim_gemm's
`tile_lo6`) under AddressSanitizer + UBSan.

tests/hostmock_narrow_lo6/ holds a stand-alone driver and a Makefile of its own; the engine's host sources and the mock HIP runtime of tests/hostmock/ are compiled
where they are.  The driver walks the option's values (a compensated decode under each on an engine with "precise_lo6" on, whole batch and pruned rows) and every
refusal of blim_gemm's tile_lo6.  It is a program with its own main: it is run directly, must end with exit code 0, no sanitizer report and no leak."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ (x86 ASan / UBSan runtimes)")
def test_narrow_lo6_switches_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "hostmock_narrow_lo6"), "-j4", f"OUT={out}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    d = subprocess.run([os.path.join(out, "narrow_lo6_driver")], capture_output=True, text=True, timeout=600, env=env)
    log = d.stdout + d.stderr
    assert d.returncode == 0 and "narrow lo6 sanitizer drive: ok" in d.stdout, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
    shutil.rmtree(out, ignore_errors=True)
