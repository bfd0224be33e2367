#!/usr/bin/env python3
"""
Static instruction mix of the kernels of one HIP source, from the compiler's assembly (no GPU needed).

    python3 tools/isa_mix.py                                  # learn-nerf_amd/csrc/nerf_mlp.hip, every kernel
    python3 tools/isa_mix.py --kernel 'nerf_fwd_kernel<true, true, false>' --kernel nerf_bwd_chain
    python3 tools/isa_mix.py --src learn-nerf_amd/csrc/refnerf_fused.hip --json

Runs `hipcc -O3 -std=c++20 --offload-arch=gfx950 --cuda-device-only -S <src> -o -` as a child process (the flags of
csrc/Makefile) and counts, per kernel: MFMA, VALU (every other v_* instruction), the VALU classes the fused chains'
epilogues are made of (v_max_f32, v_cvt_pk_bf16_f32, v_pk_max_i16, v_perm_b32, 64-bit address arithmetic), LDS and
global memory instructions (and how many of the latter take their base from SGPRs), the s_waitcnt operands, and the
registers / scratch / occupancy the compiler reports.  The counts are static: for the fused forward and chain kernels,
which are fully unrolled and handle one 32-evaluation tile per wave, they are the instructions per wave and tile.
"""
import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join("learn-nerf_amd", "csrc", "nerf_mlp.hip")
FLAGS = ["-O3", "-std=c++20", "--cuda-device-only", "-S"]

ADDR_OPS = ("v_add_co_u32", "v_addc_co_u32", "v_lshl_add_u64", "v_add_u64")
CLASSES = ("v_max_f32", "v_cvt_pk_bf16_f32", "v_pk_max_i16", "v_perm_b32", "v_mov_b32", "v_accvgpr")

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
INFO = re.compile(r"^;\s*(TotalNumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)"
                  r"\s*[:=]\s*(\d+)")
ENCODING = re.compile(r"_(e32|e64|sdwa|dpp|e64_dpp)$")  # encoding suffixes of VALU mnemonics
WAIT = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")


def compile_to_asm(src, arch, hipcc):
    cmd = [hipcc, *FLAGS, f"--offload-arch={arch}", src, "-o", "-"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed:\n{r.stderr}")
    return r.stdout


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool is None:
        cand = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "")), "..", "llvm", "bin",
                            "llvm-cxxfilt")
        tool = cand if os.path.exists(cand) else None
    if tool is None or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True)
    out = r.stdout.splitlines()
    if r.returncode != 0 or len(out) != len(names):
        return {n: n for n in names}
    # "void lnrf::nerf_fwd_kernel<true, true, false>(char const*, ...)" -> "nerf_fwd_kernel<true, true, false>"
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void\s+", "", d)
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        short[n] = re.sub(r"^(\w+::)+", "", d[:cut])
    return short


def parse(asm):
    """-> {mangled kernel name: stats dict}"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    stats, cur, last = {}, None, None
    for line in asm.splitlines():
        m = LABEL.match(line)
        if m and m.group(1) in kernels:
            cur = last = m.group(1)
            stats[cur] = {"ops": collections.Counter(), "vmcnt": collections.Counter(),
                          "lgkmcnt": collections.Counter(), "global_saddr": 0, "info": {}}
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            m = INFO.match(line)
            if m and last is not None and m.group(1) not in stats[last]["info"]:
                stats[last]["info"][m.group(1)] = int(m.group(2))
            continue
        m = INSTR.match(line)
        if not m:
            continue
        op, rest = ENCODING.sub("", m.group(1)), m.group(2).split(";")[0]
        s = stats[cur]
        s["ops"][op] += 1
        if op == "s_waitcnt":
            for what, n in WAIT.findall(rest):
                if what in s:
                    s[what][int(n)] += 1
        elif op.startswith("global_") and re.search(r",\s*s\[\d+:\d+\]", rest):
            s["global_saddr"] += 1
    return stats


def summarise(s):
    ops = s["ops"]
    total = lambda pred: sum(n for o, n in ops.items() if pred(o))
    mfma = total(lambda o: o.startswith("v_mfma") or o.startswith("v_smfmac"))
    out = {
        "mfma": mfma,
        "valu": total(lambda o: o.startswith("v_")) - mfma,
        "salu": total(lambda o: o.startswith("s_") and o not in ("s_waitcnt", "s_barrier", "s_nop", "s_endpgm")),
        "addr_adds": sum(ops[o] for o in ADDR_OPS),
        "lds_read": total(lambda o: o.startswith("ds_read") or o.startswith("ds_load")),
        "lds_write": total(lambda o: o.startswith("ds_write") or o.startswith("ds_store")),
        "global_load": total(lambda o: o.startswith("global_load")),
        "global_store": total(lambda o: o.startswith("global_store")),
        "global_saddr": s["global_saddr"],
        "flat_scratch": total(lambda o: o.startswith("flat_") or o.startswith("scratch_") or o.startswith("buffer_")),
        "s_waitcnt": ops["s_waitcnt"],
        "s_barrier": ops["s_barrier"],
        "s_nop": ops["s_nop"],
        "vmcnt": dict(sorted(s["vmcnt"].items())),
        "lgkmcnt": dict(sorted(s["lgkmcnt"].items())),
    }
    for c in CLASSES:
        out[c] = total(lambda o, c=c: o.startswith(c))
    for o in ADDR_OPS:
        out[o] = ops[o]
    info = s["info"]
    out["vgprs"] = info.get("NumVgprs")
    out["agprs"] = info.get("NumAgprs")
    out["sgprs"] = info.get("TotalNumSgprs")
    out["scratch_bytes"] = info.get("ScratchSize")
    out["occupancy"] = info.get("Occupancy")
    out["code_bytes"] = info.get("codeLenInByte")
    return out


def hist(d):
    return " ".join(f"({k})x{v}" for k, v in d.items()) or "-"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=DEFAULT_SRC, help="HIP source, relative to the repository root")
    ap.add_argument("--asm", help="read this assembly file instead of compiling --src")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "hipcc"))
    ap.add_argument("--kernel", action="append", default=[], help="only kernels whose demangled name contains this")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    args = ap.parse_args()

    if args.asm:
        with open(args.asm) as f:
            asm = f.read()
    else:
        asm = compile_to_asm(args.src, args.arch, args.hipcc)
    stats = parse(asm)
    names = demangle(list(stats))
    rows = {}
    for mangled, s in stats.items():
        name = names[mangled]
        if args.kernel and not any(k in name for k in args.kernel):
            continue
        rows[name] = summarise(s)
    if args.json:
        print(json.dumps(rows, indent=1))
        return
    for name, r in rows.items():
        print(name)
        print(f"  MFMA {r['mfma']}  VALU {r['valu']}  SALU {r['salu']}  | v_max_f32 {r['v_max_f32']}  "
              f"v_cvt_pk_bf16_f32 {r['v_cvt_pk_bf16_f32']}  v_pk_max_i16 {r['v_pk_max_i16']}  "
              f"v_perm_b32 {r['v_perm_b32']}  v_mov_b32 {r['v_mov_b32']}")
        print(f"  address adds {r['addr_adds']} (" + ", ".join(f"{o} {r[o]}" for o in ADDR_OPS) + ")")
        print(f"  LDS read {r['lds_read']} write {r['lds_write']}  global load {r['global_load']} "
              f"store {r['global_store']} (SGPR base: {r['global_saddr']})  flat/scratch/buffer {r['flat_scratch']}")
        print(f"  s_waitcnt {r['s_waitcnt']}  s_barrier {r['s_barrier']}  s_nop {r['s_nop']}")
        print(f"    vmcnt   {hist(r['vmcnt'])}")
        print(f"    lgkmcnt {hist(r['lgkmcnt'])}")
        print(f"  VGPRs {r['vgprs']}  AGPRs {r['agprs']}  SGPRs {r['sgprs']}  scratch {r['scratch_bytes']} B  "
              f"occupancy {r['occupancy']}  code {r['code_bytes']} B")


if __name__ == "__main__":
    main()
