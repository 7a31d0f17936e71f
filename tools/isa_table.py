#!/usr/bin/env python3
"""Static ISA figures of the kernels in a gfx950 assembly file (hipcc --cuda-device-only -S):
per kernel, instructions, VALU / SALU / MFMA counts, integer-division sequences (v_rcp_iflag_f32),
the position of the first global loads, and the register counts of the compiler's metadata.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S \
        headposeestimation-whenet_amd/csrc/front2.hip -o front2.s
    python tools/isa_table.py front2.s [substring of the demangled kernel name]

The project GEMMs and front.hip (generic against static form, docs/experiments.md section 26): the same on csrc/pw.hip and
csrc/front.hip without the -mllvm flag; the static form of a kernel is the instantiation whose last template argument is a row
of the kernel's shape table instead of -1.  Where no demangler is installed the names stay mangled (_Float16 is DF16_, -1 is Lin1E).
"""
import os
import re
import subprocess
import sys


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:\s+\d+\s+(?:\.args:.*?)?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?"
                         r"\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+)\s+\.sgpr_spill_count:\s+(\d+).*?"
                         r"\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
        meta[m.group(2)] = tuple(int(m.group(i)) for i in (4, 5, 6, 7, 1, 3))
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        if m.group(1) in meta:
            bodies[m.group(1)] = m.group(2)
    names = demangle(list(bodies))
    print("| kernel | instr | VALU | SALU | MFMA | idiv | 1st global load | 3rd | SGPR / spill | VGPR / spill | LDS B | scratch B |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for sym, body in bodies.items():
        name = re.sub(r"\(whenet::.*", "", names[sym]).replace("void whenet::(anonymous namespace)::", "")
        if want not in name:
            continue
        ins = [l.split()[0] for l in body.split("\n") if re.match(r"^\s+[a-z_0-9]+(\s|$)", l) and not l.strip().startswith(".")]
        loads = [i for i, x in enumerate(ins) if x.startswith("global_load")]
        sg, ss, vg, vs, lds, scratch = meta[sym]
        print(f"| `{name}` | {len(ins)} | {sum(x.startswith('v_') and 'mfma' not in x for x in ins)} | "
              f"{sum(x.startswith('s_') for x in ins)} | {sum('mfma' in x for x in ins)} | {ins.count('v_rcp_iflag_f32_e32')} | "
              f"{loads[0] if loads else '-'} | {loads[2] if len(loads) > 2 else '-'} | {sg} / {ss} | {vg} / {vs} | {lds} | {scratch} |")


if __name__ == "__main__":
    main()
