#!/usr/bin/env python3
"""Two device-assembly listings of one translation unit, kernel by kernel (the static half of a refactor's check).

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -o A.s vittrack.hip      (and B.s from the other tree)
    python tools/isa_compare.py A.s B.s [--resources]

A function is the text from its `_Z...:` label to `.Lfunc_end`; comments are dropped and the function ordinal in `.LBB<n>_` labels is
normalised, so a kernel that merely moved in the file compares equal.  Prints the number of kernels on each side, the symbols only
one side has, and per differing kernel its demangled name and both line counts.  --resources compares, per symbol, the
`.set <sym>.num_vgpr / .numbered_sgpr / .private_seg_size` lines and `.amdhsa_group_segment_fixed_size` instead.  Texts only: no
particular instruction is looked for.  Exit status 1 when anything differs."""
import re, subprocess, sys


def functions(path):
    out, name = {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"(_Z\w+):$", line)
        if m:
            name, out[m.group(1)] = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            name = None
        elif name and line.strip():
            out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.set (_Z\w+)\.(num_vgpr|numbered_sgpr|private_seg_size), (\S+)", line)
        if m:
            out.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
        m = re.match(r"\s*\.amdhsa_kernel (_Z\w+)", line)
        cur = m.group(1) if m else cur
        m = re.match(r"\s*\.amdhsa_group_segment_fixed_size (\d+)", line)
        if m and cur:
            out.setdefault(cur, {})["lds"] = m.group(1)
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def main():
    res = "--resources" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--resources"]
    read, what = (resources, "symbols with resource lines") if res else (functions, "kernels")
    show = (lambda v: v) if res else len
    a, b = read(args[0]), read(args[1])
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    names = demangle(only + differ)
    print(f"{what}: {len(a)} | {len(b)}; on one side only: {len(only)}; differ: {len(differ)}")
    for k in only:
        print("  only in", args[0] if k in a else args[1], names[k])
    for k in differ:
        print("  ", names[k], show(a[k]), "|", show(b[k]))
    sys.exit(1 if only or differ else 0)


if __name__ == "__main__":
    main()
