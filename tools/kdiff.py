#!/usr/bin/env python3
"""Compare the kernels of two device-assembly builds against each other.

usage: python3 tools/kdiff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] [FILTER-REGEX]
  each side: one or more outputs of
    hipcc <the Makefile's flags> --offload-arch=gfx950 -S --cuda-device-only SRC.hip -o SRC.s
Kernels are matched by demangled name. Per kernel: the instruction count of each build and whether
the instruction sequence is identical as mnemonics, and as whole instructions once register numbers
and local labels are normalised. It diffs two builds only; it knows nothing about any instruction.
"""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} of the .amdhsa_kernel symbols of one .s file."""
    names, bodies, cur = set(), {}, None
    lines = open(path, errors="replace").read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w.$]*):", ln)
        if m and m.group(1) in names:
            cur = bodies.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        t = ln.split(";")[0].strip()
        if t.startswith(".Lfunc_end") or t.startswith(".section") or t.startswith(".rodata"):
            cur = None
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        cur.append(t)
    return bodies


def normalise(ins):
    ins = re.sub(r"\b([svaSVA])\[\d+(:\d+)?\]", lambda m: m.group(1) + ("[r:r]" if m.group(2) else "[r]"), ins)
    ins = re.sub(r"\b([sva])\d+\b", r"\1r", ins)
    return re.sub(r"\.LBB\d+_\d+", ".L", ins)


def load(spec):
    out = {}
    for p in spec.split(","):
        out.update(kernels(p))
    mangled = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
    clean = lambda n: n.replace("icp::(anonymous namespace)::", "").replace("(icp::NNLaunch)", "")
    return {clean(d): out[m] for m, d in zip(mangled, dem)}


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    filt = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    same_m = same_n = moved = 0
    rows = [n for n in old if n in new and filt.search(n)]
    for n in rows:
        a, b = old[n], new[n]
        mn = [x.split()[0] for x in a] == [x.split()[0] for x in b]
        nm = mn and [normalise(x) for x in a] == [normalise(x) for x in b]
        same_m += mn
        same_n += nm
        moved += len(a) != len(b)
        print("%-60s insts %6d -> %6d  mnemonics %-9s operands %s" %
              (n[:60], len(a), len(b), "identical" if mn else "DIFFER", "identical" if nm else "differ"))
    for n in sorted(set(old) ^ set(new)):
        if filt.search(n):
            print("%-60s only in the %s build" % (n[:60], "old" if n in old else "new"))
    print("summary: %d kernels matched, %d with an identical mnemonic sequence, %d identical after "
          "register/label normalisation, %d with a changed instruction count" % (len(rows), same_m, same_n, moved))


if __name__ == "__main__":
    main()
