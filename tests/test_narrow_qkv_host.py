"""CPU: the host side of the narrow-tile QKV GEMM's switches -- blim_gemm_args ends on `tile_qkv` in the header and in the ctypes mirror, the library exports the
counter and the threshold (which is gemm.hpp's constant), the engine module offers both, and both command lines parse --narrow_qkv and refuse it with --dtype f8."""
import ctypes as C
import os
import re

import pytest

from blim_amd import engine as eng
from blim_amd import main as blim_main
from blim_amd import search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_args_end_on_tile_qkv():
    names = [f[0] for f in eng.GemmArgs._fields_]
    assert names[-3:] == ["tile", "tile_lo6", "tile_qkv"]
    assert eng.GemmArgs.tile_qkv.size == 4 and eng.GemmArgs.tile_qkv.offset == eng.GemmArgs.tile_lo6.offset + 4
    header = open(os.path.join(ROOT, "include", "blim.h")).read()
    body = re.search(r"typedef struct blim_gemm_args \{(.*?)\} blim_gemm_args;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?[\w ]+?[\s\*]+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert fields[-3:] == ["tile", "tile_lo6", "tile_qkv"], fields[-4:]
    assert re.search(r"#define\s+BLIM_ABI_VERSION\s+9\b", header)
    assert "tile_qkv" in eng._GEMM_INTS


def test_the_library_exports_the_counter_and_the_threshold():
    assert os.path.exists(eng.LIB_PATH), f"{eng.LIB_PATH} is missing: build() has not run"
    lib = C.CDLL(eng.LIB_PATH)
    for sym in ("blim_gemm_narrow_qkv_launches", "blim_gemm_narrow_qkv_threshold", "blim_gemm_narrow_launches", "blim_gemm_narrow_lo6_launches"):
        assert hasattr(lib, sym), sym
    lib.blim_gemm_narrow_qkv_launches.restype = C.c_int64
    lib.blim_gemm_narrow_qkv_threshold.restype = C.c_int32
    assert lib.blim_gemm_narrow_qkv_launches() >= 0                     # (a process-wide counter: GPU tests of the same session may have moved it)
    hpp = open(os.path.join(ROOT, "blim_amd", "csrc", "gemm.hpp")).read()
    assert lib.blim_gemm_narrow_qkv_threshold() == int(re.search(r"#define\s+GEMM_NARROW_QKV_TILES\s+(\d+)", hpp).group(1))
    assert callable(eng.gemm_narrow_qkv_launches) and callable(eng.gemm_narrow_qkv_threshold)


def test_params_struct_ends_on_narrow_qkv():
    hpp = open(os.path.join(ROOT, "blim_amd", "csrc", "gemm.hpp")).read()
    body = re.search(r"struct GemmParams \{(.*?)\n\};", hpp, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?[\w ]+?[\s\*]+(\w+);", re.sub(r"//[^\n]*", "", body), re.M)
    assert fields[-3:] == ["narrow", "narrow_lo6", "narrow_qkv"], fields[-4:]


@pytest.mark.parametrize("parser", [search.get_args_parser, blim_main.get_args_parser], ids=["search", "main"])
def test_both_command_lines_parse_the_flag(parser):
    p = parser()
    assert p.parse_args([]).narrow_qkv == "off"
    assert p.parse_args(["--narrow_qkv", "auto"]).narrow_qkv == "auto"
    with pytest.raises(SystemExit):
        p.parse_args(["--narrow_qkv", "on"])


@pytest.mark.parametrize("mod", [search, blim_main], ids=["search", "main"])
def test_both_command_lines_refuse_the_flag_with_f8(mod):
    args = mod.get_args_parser().parse_args(["--narrow_qkv", "auto", "--dtype", "f8"])
    with pytest.raises(SystemExit, match="--narrow_qkv auto needs a 16-bit engine"):
        mod.check_args(args)
    extra = ["--query_ids", "0"] if mod is search else []
    mod.check_args(mod.get_args_parser().parse_args(["--narrow_qkv", "auto", "--dtype", "f16"] + extra))          # a 16-bit engine: accepted
