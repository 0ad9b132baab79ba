#!/usr/bin/env python3
"""Static census of a map kernel instantiation in a gfx950 code object: registers and spills from the notes, instruction counts by
class from the disassembly -- for the whole kernel and, in a -DMQ_CODE_MARKS build, per stage between the stage stamps' symbols (the
split of tools/code_sizes.sh).  No GPU needed.

    hipcc --offload-arch=gfx950 --offload-device-only -c <the library's flags> [-DMQ_CODE_MARKS] -o x.o mapquik_amd/csrc/mq_capi.hip
    clang-offload-bundler --unbundle --type=o --input=x.o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=x.hsaco
    tools/spec_census.py x.hsaco [substring of the demangled kernel name, default "map_kernel<64, false, false, mq::SpecNone>"]

Classes (one instruction is counted in one class only, in this order):
    lane    v_readlane / v_writelane / v_readfirstlane        (what an SGPR spill costs on the vector pipe)
    v_mov   v_mov_b32 / v_mov_b64 / v_accvgpr moves
    valu_s  any other v_ instruction with an SGPR, vcc or exec SOURCE operand (2.46 cycles against 1.03, tools/valu_enc.hip)
    valu    every other v_ instruction
    lds, vmem, smem, salu, branch, wait/other
"""
import re
import subprocess
import sys

LLVM = "/opt/rocm/lib/llvm/bin/"
CLASSES = ("lane", "v_mov", "valu_s", "valu", "lds", "vmem", "smem", "salu", "branch", "other")
SREG = re.compile(r"^(s\d+|s\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?|ttmp\d+|m0)$")


def classify(mn, ops):
    if mn.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if mn.startswith(("v_mov_b", "v_accvgpr")):
        return "v_mov"
    if mn.startswith("v_"):
        return "valu_s" if any(SREG.match(o) for o in ops[1:]) else "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if mn.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep", "s_setprio", "s_sethalt", "s_code_end", "s_icache_inv")):
        return "other"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def symbols(path):
    out = subprocess.run([LLVM + "llvm-readelf", "-sW", "--demangle", path], capture_output=True, text=True, check=True).stdout
    syms = []
    for ln in out.splitlines():
        p = ln.split(None, 7)
        if len(p) >= 8 and re.match(r"^[0-9a-f]+$", p[1]) and p[2].isdigit():
            syms.append((int(p[1], 16), int(p[2]), p[3], p[7]))
    return syms


def notes(path, mangled):
    """the scalar fields of the kernel's entry in the AMDGPU metadata note (YAML; an entry of amdhsa.kernels opens with .agpr_count)"""
    out = subprocess.run([LLVM + "llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    for blk in out.split("\n  - .agpr_count:"):
        if re.search(r"\.name:\s+" + re.escape(mangled) + r"\s*\n", blk):
            return {m.group(1): m.group(2) for m in re.finditer(r"^\s+\.(\w+):\s+(\S+)\s*$", "    .agpr_count:" + blk, re.M)}
    return {}


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "map_kernel<64, false, false, mq::SpecNone>"
    syms = symbols(path)
    k = [s for s in syms if s[2] == "FUNC" and want in s[3] and "void" in s[3]] or [s for s in syms if s[2] == "FUNC" and want in s[3]]
    if not k:
        sys.exit("no kernel matching %r" % want)
    a0, size, _, name = k[0]
    mangled = subprocess.run([LLVM + "llvm-readelf", "-sW", path], capture_output=True, text=True).stdout
    mangled = [ln.split()[7] for ln in mangled.splitlines() if len(ln.split()) >= 8 and ln.split()[3] == "FUNC" and int(ln.split()[1], 16) == a0][0]
    print("kernel: %s\n  symbol %s, %d bytes" % (name, mangled, size))
    md = notes(path, mangled)
    print("  notes: " + "  ".join("%s=%s" % (f, md.get(f, "?")) for f in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                                                        "private_segment_fixed_size", "group_segment_fixed_size")))
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--start-address=%d" % a0, "--stop-address=%d" % (a0 + size), path],
                         capture_output=True, text=True, check=True).stdout  # (by address: the stage stamps are symbols inside the kernel)
    insts = []
    for ln in dis.splitlines():
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
        if m:
            ops = [o.strip() for o in m.group(2).split(",")] if m.group(2) else []
            ops = [o.split(" ")[0] for o in ops]
            insts.append((int(m.group(3), 16), m.group(1), ops))
    marks = sorted((a, n) for a, _, _, n in syms if n.startswith("mq_mark_") and a0 <= a < a0 + size)
    bounds = [(a0, "entry")] + marks + [(a0 + size, "end")]

    def census(lo, hi):
        c = dict.fromkeys(CLASSES, 0)
        for a, mn, ops in insts:
            if lo <= a < hi:
                c[classify(mn, ops)] += 1
        return c

    hdr = "%-26s %8s " % ("segment", "bytes") + " ".join("%7s" % c for c in CLASSES)
    print(hdr)
    whole = census(a0, a0 + size)
    print("%-26s %8d " % ("whole kernel", size) + " ".join("%7d" % whole[c] for c in CLASSES))
    if marks:
        tot = {}
        for (lo, n0), (hi, n1) in zip(bounds, bounds[1:]):
            stage = n1.split("_")[2] if n1.startswith("mq_mark_") else n1
            c = census(lo, hi)
            t = tot.setdefault(stage, dict.fromkeys(("bytes",) + CLASSES, 0))
            t["bytes"] += hi - lo
            for x in CLASSES:
                t[x] += c[x]
        for stage in sorted(tot, key=lambda s: (len(s), s)):
            t = tot[stage]
            print("%-26s %8d " % ("in front of stamp " + stage, t["bytes"]) + " ".join("%7d" % t[c] for c in CLASSES))


if __name__ == "__main__":
    main()
