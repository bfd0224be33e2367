#!/usr/bin/env python3
"""
Per-kernel diff of two device assembly files of the same HIP source (no GPU needed): the check behind "this refactor
compiles to the same instructions".

    hipcc -O3 -std=c++20 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -S --cuda-device-only \\
          learn-nerf_amd/csrc/ngp_mlp.hip -o new.s          # the flags of csrc/Makefile; likewise old.s from the parent
    python3 tools/asm_kernel_diff.py old.s new.s [--full]

Kernels are matched by demangled name without the argument list, so a kernel whose signature changed is still compared.
Only instructions and local labels are compared (comments, directives and the numbering of .LBB labels are dropped).
A kernel with the same instruction sequence in which some s_load / s_add_u32 / s_cselect_b32 / s_mov_b64 differ in an
immediate only is reported as such: that is what removing a kernel argument or a field of an argument struct leaves.
"""
import difflib
import re
import subprocess
import sys

IMM = re.compile(r"^(0x[0-9a-f]+|-?\d+)$")
ARG_OPS = ("s_load_dword", "s_load_dwordx2", "s_load_dwordx4", "s_add_u32", "s_cselect_b32", "s_mov_b64")


def kernels(path):
    """-> {short demangled kernel name: [instruction lines]}"""
    asm = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = m.group(1)
            out[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    dem = subprocess.run(["c++filt"], input="\n".join(out) + "\n", stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {re.sub(r"\(.*", "", d.replace("void ", "").replace("lnrf::", "")): out[k] for k, d in zip(out, dem)}


def without_immediates(instr):
    return [o for o in re.split(r"[ ,]+", instr) if not IMM.match(o)]


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    full = "--full" in sys.argv
    for k in a:
        if k not in b:
            print(f"{k}: missing in the second file")
            continue
        diff = list(difflib.unified_diff(a[k], b[k], lineterm="", n=0))
        verdict = "identical"
        if diff:
            pairs = [(x, y) for x, y in zip(a[k], b[k]) if x != y]
            if len(a[k]) == len(b[k]) and all(x.split()[0] in ARG_OPS and without_immediates(x) == without_immediates(y)
                                               for x, y in pairs):
                verdict = (f"{len(pairs)} instructions differ, each an s_load / s_add_u32 / s_cselect_b32 / s_mov_b64 with "
                           f"another immediate (kernel-argument offsets); everything else identical")
            else:
                n = sum(1 for l in diff if l[0] in "+-" and not l.startswith(("+++", "---")))
                verdict = f"{n} differing lines"
        print(f"{k}: {len(a[k])} -> {len(b[k])} instructions, {verdict}")
        if full and diff:
            print("\n".join("    " + l for l in diff[2:]))
    for k in b:
        if k not in a:
            print(f"{k}: only in the second file")


if __name__ == "__main__":
    main()
