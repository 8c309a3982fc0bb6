"""Compare the attn_kernel instantiations of two device-assembly files of csrc/attention.hip (hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950
--cuda-device-only -S attention.hip), e.g. the parent commit's against this tree's.  Every kernel of the first file is matched with the kernel of the second
whose template arguments start with its own (a template parameter added with a default value -- the gallery's PC = false -- is appended to the mangled name)
and whose parameter type is AttnParams; bodies are compared with comments, label numbers and the kernel's own name normalised.  Prints one line per
kernel that differs and a summary; exit status 1 when any differs.

    python tools/attn_isa_diff.py before.s after.s"""
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); out[cur] = []; continue
        if cur is None:
            continue
        if line.startswith("\t.section") or re.match(r"^\s*\.size\s", line) or line.startswith(".Lfunc_end"):
            cur = None; continue
        out[cur].append(line)
    return out


def normalised(lines, name):
    res = []
    for line in lines:
        line = line.replace(name, "KERNEL").split(";")[0].rstrip()
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        if line:
            res.append(line)
    return res


def main(before, after):
    a, b = kernels(before), kernels(after)
    same, diff = 0, []
    for k, body in a.items():
        if "attn_kernel" not in k:
            continue
        args = k.split("attn_kernelI")[1].split("EEv")[0]
        m = [k2 for k2 in b if k2.startswith("_Z11attn_kernelI" + args + "E") and k2.endswith("10AttnParamsE4typeE") or k2 == k]
        m = [k2 for k2 in m if "Lb1EEvNSt11conditional" not in k2 or k2 == k]
        if len(m) != 1 or normalised(body, k) != normalised(b[m[0]], m[0]):
            diff.append(k)
        else:
            same += 1
    for k in diff:
        print("DIFFERS:", k)
    print(f"attn_kernel instantiations: {sum('attn_kernel' in k for k in a)} before, {sum('attn_kernel' in k for k in b)} after; "
          f"{same} of the earlier ones identical, {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
