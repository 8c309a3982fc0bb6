"""CPU (-m "not gpu"): the host code of blim_score_tvg_first_within and blim_tvg_rank_within (csrc/engine.hip) under AddressSanitizer + UBSan.

tests/hostmock_within/ holds a stand-alone driver and a Makefile of its own; the engine's host sources and the mock HIP runtime of tests/hostmock/ are compiled where
they are.  The driver runs the calls from one query to more rows and queries than a 256-row round of the workspaces, with and without prior rows, plain and compensated, and walks
every refusal of the two entry points.  It is a program with its own main: it is run directly, must end with exit code 0, no sanitizer report and no leak."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ (x86 ASan / UBSan runtimes)")
def test_within_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "hostmock_within"), "-j4", f"OUT={out}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    d = subprocess.run([os.path.join(out, "within_driver")], capture_output=True, text=True, timeout=600, env=env)
    log = d.stdout + d.stderr
    assert d.returncode == 0 and "within sanitizer drive: ok" in d.stdout, log[-4000:]
    assert "AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
    shutil.rmtree(out, ignore_errors=True)
