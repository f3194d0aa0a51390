#!/usr/bin/env python3
"""The wait structure of a kernel from hipcc's assembly listing: its scalar and vector LOADS, its waits and its branches in program order, everything else
counted but left out.  Each line is prefixed by the number of instructions in front of it, so "the first vmcnt(0) is N instructions in" can be read off.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only -o k_contacts.s avian_amd/csrc/k_contacts.hip
       python tools/wait_structure.py k_contacts.s 'k_color_pass<float, 1>' ['k_color_pass<float, 2>' ...]
Kernels of namespace avn, named as a demangler prints them without the argument list."""
import re
import sys

KEEP = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load|s_load|s_buffer_load|s_waitcnt|s_cbranch|s_branch|s_endpgm|s_setpc|s_barrier)")
LABEL = re.compile(r"^([.\w$]+):")
SUMMARY = re.compile(r"^; (NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|codeLenInByte): ")


def mangled_prefix(want):
    """'k_color_pass<float, 1>' -> '_ZN3avn12k_color_passIfLi1EE' (kernels of namespace avn whose template arguments are float / double / bool and integers)"""
    m = re.fullmatch(r"(\w+)(?:<(.*)>)?", want.strip())
    name, targs = m.group(1), [t.strip() for t in (m.group(2) or "").split(",") if t.strip()]
    enc = "".join({"float": "f", "double": "d"}.get(t) or ("Lb1E" if t == "true" else "Lb0E" if t == "false" else f"Li{t}E") for t in targs)
    return f"_ZN3avn{len(name)}{name}" + (f"I{enc}E" if targs else "")


def kernels(path):
    """{mangled name: [lines from `name:` to the end of the compiler's resource summary behind the kernel]}"""
    lines = open(path).read().splitlines()
    found, cur, name = {}, None, None
    for ln in lines:
        m = re.match(r"^(_Z[\w$]+):\s*(;.*)?$", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            cur.append(ln)
            if SUMMARY.match(ln.strip()) and ln.strip().startswith("; Occupancy"):
                found[name] = cur
                cur = None
    return found


def structure(body):
    out, n = [], 0
    summary = []
    for ln in body:
        s = ln.strip()
        if SUMMARY.match(s):
            summary.append(s[2:])
            continue
        if not s or s.startswith(";") or s.startswith("."):
            m = LABEL.match(s)
            if m and s.startswith(".LBB"):
                out.append(f"      {m.group(1)}:")
            continue
        m = LABEL.match(s)
        if m:
            out.append(f"      {m.group(1)}:")
            continue
        s = s.split(";")[0].rstrip()
        if KEEP.match(s):
            out.append(f"{n:5d} {s}")
        n += 1
    return out, n, summary


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    ks = kernels(path)
    for want in wanted:
        hits = [k for k in ks if k.startswith(mangled_prefix(want))]
        if not hits:
            print(f"== {want}: not found"); continue
        for k in hits:
            out, n, summary = structure(ks[k])
            loads = sum(1 for l in out if re.search(r"\d (global|buffer|flat)_load", l))
            print(f"== {want} ({k[:60]}): {n} instructions, {loads} vector loads; {', '.join(summary)}")
            print("\n".join(out))
            print()


if __name__ == "__main__":
    main()
