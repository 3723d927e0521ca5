#!/usr/bin/env python3
"""Kernel resource usage from hipcc's -Rpass-analysis=kernel-resource-usage remarks, and the diff of two
builds (the default path's instantiations are untouched by a new variant).

  hipcc --offload-arch=gfx950 --cuda-device-only <the Makefile's HIPFLAGS> \\
        -Rpass-analysis=kernel-resource-usage -c csrc/pathtrace.hip -o /dev/null 2> branch.log
  tools/resource_usage.py parent.log branch.log     # every kernel of either log, changed ones marked
  tools/resource_usage.py branch.log                # one build's table

Exit status 1 when a kernel both logs hold differs in any column.  No GPU needed.
"""
import re
import subprocess
import sys

COLS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
        ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"), ("LDS Size [bytes/block]", "LDS"),
        ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        r = list(names)
    short = {}
    for n, d in zip(names, r):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\(PathTraceParams\)$", "", d)
    return short


def row(u):
    return " ".join("%7s" % u.get(k, "-") for k, _ in COLS)


def main(argv):
    if len(argv) not in (2, 3):
        print(__doc__)
        return 2
    raw = [parse(p) for p in argv[1:]]
    short = demangle(sorted(set().union(*raw)))
    logs = [{short[n]: u for n, u in r.items()} for r in raw]  # keyed by the demangled name
    if len(logs) == 2:
        # a template parameter added with the default `false` renames an instantiation without changing
        # it: k<a, b> of the first build is k<a, b, false> of the second
        for name in list(logs[0]):
            grown = re.sub(r">$", ", false>", name)
            if name not in logs[1] and grown in logs[1]:
                logs[0][grown] = logs[0].pop(name)
    names = sorted(set().union(*logs))
    short = {n: n for n in names}
    width = max(len(short[n]) for n in names)
    print("%-*s %s" % (width + 8, "kernel", " ".join("%7s" % c for _, c in COLS)))
    changed = 0
    for n in sorted(names, key=lambda k: short[k]):
        if len(logs) == 1:
            print("%-*s %s" % (width + 8, short[n], row(logs[0][n])))
            continue
        a, b = logs[0].get(n), logs[1].get(n)
        if a is None or b is None:
            print("%-*s %s" % (width + 8, short[n] + (" [new]" if a is None else " [gone]"), row(b or a)))
        elif a == b:
            print("%-*s %s" % (width + 8, short[n] + " [same]", row(b)))
        else:
            changed += 1
            print("%-*s %s" % (width + 8, short[n] + " [WAS]", row(a)))
            print("%-*s %s" % (width + 8, short[n] + " [NOW]", row(b)))
    if len(logs) == 2:
        print("%d kernel(s) of both builds differ" % changed)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
