"""CPU (-m "not gpu"): the launches of the engine's host code (csrc/engine.hip: run_layers, the heads, the projector), compared with a recorded trace.

tests/hostmock_trace/ holds a stand-alone driver and a Makefile of its own; the engine's host sources and the mock HIP runtime of tests/hostmock/ are compiled where
they are.  The driver defines the launchers the decoder and the heads call and writes one line per launch -- every argument, GemmParams field by field, pointers as
alloc<rank>+<offset> or the name of a driver buffer -- through every numeric mode of the engine (plain, the compensated modes with the 16-bit and the e2m3 second
pass, per-layer masks, adapters apart, fp8, the narrow-tile options, pruned and unpruned last layers, the gallery's fill / cached / admit calls).
tests/golden/launch_trace.txt is that output, recorded BEFORE run_layers got its single post-attention path and the GEMM parameters their one builder: a change
to the host code that moves, drops or alters any launch shows up here as a differing line.  The golden file's own coverage is asserted too, so that it cannot pass
while saying nothing.

File format: "engine" lines as they are; "state <label> : state <k>" opens a state and "state <label> == state <k>" stands for one whose calls and lines are those
of state k; "call <name> : block <k>" opens the lines of one call, "call <name> == block <k>" stands for a call whose lines
are those of block k.  Inside a block a line seen for the first time is "<n>| <text>"; repeated lines are named by number, a run of them on one line as
"= <n> <a>-<b> ..." (a-b: lines a to b in order).  Fields that hold a launcher's default are left out (the file's first line lists them), a pointer at offset 0 has
no "+0", and "dtype=c" is the compute dtype the engine line gives.  The comparison is made on the expanded text."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GOLDEN = os.path.join(HERE, "golden", "launch_trace.txt")


def expand(text):
    table, blocks, states, out, body, state = {}, {}, {}, [], None, None

    def add(lines, to_body=True):
        out.extend(lines)
        if state is not None:
            state.extend(lines)
        if to_body and body is not None:
            body.extend(lines)

    for raw in text.splitlines():
        if raw.startswith("state "):
            m = re.fullmatch(r"(state .*) (:|==) state (\d+)", raw)
            body = state = None
            add([m.group(1)])
            if m.group(2) == "==":
                add(states[int(m.group(3))])
            else:
                state = states.setdefault(int(m.group(3)), [])
        elif raw.startswith("call "):
            m = re.fullmatch(r"call (.*) (:|==) block (\d+)", raw)
            body = None
            add(["call " + m.group(1)])
            if m.group(2) == "==":
                add(blocks[int(m.group(3))])
            else:
                body = blocks.setdefault(int(m.group(3)), [])
        elif raw.startswith(("#", "engine ")):
            body = state = None
            add([raw])
        elif raw.startswith("="):
            for ref in raw[1:].split():
                a, _, b = ref.partition("-")
                add([table[k] for k in range(int(a), int(b or a) + 1)])
        else:
            n, line = raw.split("| ", 1)
            table[int(n)] = line
            add([line])
    return out


def kind(line):
    w = line.split(" ", 2)
    return " ".join(w[:2]) if w[0] == "launch_gemm" else w[0]


def fields(line):
    return dict(m.groups() for m in re.finditer(r"(\w+)=(\S+)", line))


def alloc(ptr):
    return ptr.split("+")[0]


@pytest.fixture(scope="module")
def golden():
    return expand(open(GOLDEN).read())


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ (x86 ASan / UBSan runtimes)")
def test_every_launch_of_the_host_code_matches_the_recorded_trace(tmp_path, golden):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "hostmock_trace"), "-j4", f"OUT={out}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("BLIM_LO6_FUSED_MASK", None)
    d = subprocess.run([os.path.join(out, "trace_driver")], capture_output=True, text=True, timeout=600, env=env)
    assert d.returncode == 0 and "launch trace drive: ok" in d.stderr, (d.stdout[-2000:] + d.stderr[-4000:])
    assert "AddressSanitizer" not in d.stderr and "runtime error" not in d.stderr and "LeakSanitizer" not in d.stderr, d.stderr[-4000:]
    got = expand(d.stdout)
    shutil.rmtree(out, ignore_errors=True)
    first = {}                                                       # the first differing line of each kind
    where = {}
    for i, (g, w) in enumerate(zip(got, golden)):
        if w.startswith(("engine ", "state ", "call ")):
            where[w.split(" ", 1)[0]] = w
        if g != w:
            first.setdefault(kind(w), f"line {i + 1} ({' / '.join(where.values())}):\n  recorded: {w}\n  now:      {g}")
    report = "\n".join(first.values())
    assert not first and len(got) == len(golden), f"{len(got)} lines now, {len(golden)} recorded; first difference of each kind:\n{report}"


def test_the_recorded_trace_covers_every_form(golden):
    """What the golden file must contain, read from the file itself: every operand form of the hi | lo GEMMs, who wrote the e2m3 tiles a GEMM reads, the fp8
    additions, the narrow options, the pruned last layer, augmented weights, the e2m3 LM head and the gallery's launches."""
    seen = set()
    last_writer = {}                                                 # allocation -> the launch that last wrote e2m3 tiles into it
    base_w = {}                                                      # epilogue -> W operands seen without adapters
    adapters = False
    for line in golden:
        if line.startswith("engine "):
            last_writer.clear()
        if line.startswith("state "):
            adapters = " adapters " in line
        name = line.split(" ", 1)[0]
        f = fields(line)
        if name == "launch_f6_tiles":
            last_writer[alloc(f["out"])] = "f6_tiles"
        elif name == "launch_rmsnorm" and "out6" in f:
            last_writer[alloc(f["out6"])] = "rmsnorm"
        elif name in ("launch_attention_cached", "launch_kv_capture"):
            seen.add(name)
        elif name == "launch_gemm":
            epi = line.split(" ")[1]
            if int(f.get("w_wrap_k", 0)) > 0:
                seen.add("w_wrap_k")
            if "A6" in f:
                w = last_writer.get(alloc(f["A6"]))
                assert w is not None, line
                seen.add(f"A6 of {epi} written by {w}")
            if "out6" in f:
                seen.add("out6")
                last_writer[alloc(f["out6"])] = "out6 epilogue"
            for k in ("a_mx", "out_mx"):
                if k in f:
                    seen.add(k)
            for k in ("narrow", "narrow_lo6", "narrow_qkv"):
                if f.get(k) == "2":
                    seen.add(f"{k}=2")
            if epi == "resid" and f["M"] == "38":
                seen.add("38 live rows" + (" with A6" if "A6" in f else ""))
            if epi in ("qkv", "resid") and f["W"] != "0":
                if not adapters:
                    base_w.setdefault(epi, set()).add(alloc(f["W"]))
                elif alloc(f["W"]) not in base_w.get(epi, set()):
                    seen.add("augmented weight")
    want = {"w_wrap_k", "out6", "a_mx", "out_mx", "narrow=2", "narrow_lo6=2", "narrow_qkv=2", "38 live rows", "38 live rows with A6", "augmented weight",
            "launch_attention_cached", "launch_kv_capture", "A6 of lse written by f6_tiles",
            "A6 of qkv written by f6_tiles", "A6 of resid written by f6_tiles", "A6 of swiglu written by f6_tiles",     # tiles quantised on the spot
            "A6 of qkv written by rmsnorm", "A6 of swiglu written by rmsnorm", "A6 of resid written by out6 epilogue"}   # tiles a producer wrote: norm 1, norm 2, gate | up
    assert want <= seen, sorted(want - seen)
