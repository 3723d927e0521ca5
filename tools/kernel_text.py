#!/usr/bin/env python3
"""Per-kernel comparison of two device builds of one source file: a host-only change
leaves every kernel's instructions as they were.  No GPU needed.

  hipcc --offload-arch=gfx950 --cuda-device-only <the Makefile's HIPFLAGS> -c csrc/denoise.hip -o parent.o
  tools/kernel_text.py parent.o branch.o

The gfx950 code objects are disassembled and compared symbol by symbol without addresses and encodings
(whole objects differ in symbol order and padding where no kernel does).  Lines that differ in a number
only, such as a kernel-argument offset that moved with the parameter struct, are counted apart.
Exit status 1 when the kernel sets, a kernel's size or a kernel's instructions differ.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernels(path, tmp):
    """{kernel symbol: (size, [instruction lines])} of an offload bundle or a code object."""
    co = path
    if open(path, "rb").read(4) != b"\x7fELF":
        co = os.path.join(tmp, "%d.co" % len(os.listdir(tmp)))
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + path,
                        "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    dump = lambda *a: subprocess.run([os.path.join(LLVM, "llvm-objdump"), *a, co], capture_output=True, text=True,
                                     check=True).stdout
    sizes, kd = {}, set()
    for line in dump("-t").splitlines():
        m = re.match(r"^[0-9a-f]+ (.{7}) \S+\s+([0-9a-f]+) (?:\.\w+ )?(\S+)$", line)  # flags, size, name
        if m and m.group(3).endswith(".kd"):  # a kernel descriptor
            kd.add(m.group(3)[:-3])
        elif m and "F" in m.group(1):
            sizes[m.group(3)] = int(m.group(2), 16)
    text, cur, pcrel = {}, None, 0
    for line in dump("-d", "--no-show-raw-insn", "--no-leading-addr").splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        line = re.sub(r"\s*//.*$", "", line).strip()  # the comment holds the address
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and line not in ("", "..."):  # "...": zero padding up to the next symbol
            # the two adds after s_getpc_b64 carry a variable's distance from the program counter,
            # which moves with the order of the symbols
            if pcrel and re.match(r"s_addc?_u32 .*, (0x[0-9a-f]+|-?\d+)$", line):
                line = re.sub(r"\S+$", "<pc-relative>", line)
            pcrel = 2 if line.startswith("s_getpc_b64") else max(pcrel - 1, 0)
            cur.append(line)
    return {k: (sizes[k], text.get(k, [])) for k in kd if k in sizes}


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (kernels(p, tmp) for p in argv[1:])
    num = lambda s: re.sub(r"\b(0x[0-9a-f]+|\d+)\b", "#", s)
    bad = same = moved = offsets = 0
    for k in sorted(set(a) | set(b)):
        (sa, ta), (sb, tb) = a.get(k, (None, [])), b.get(k, (None, []))
        diff = [(x, y) for x, y in zip(ta, tb) if x != y]
        other = [d for d in diff if num(d[0]) != num(d[1])]
        if sa != sb or len(ta) != len(tb) or other:
            bad += 1
            print("size %s -> %s, %d -> %d lines, %d differ in more than a number: %s" % (sa, sb, len(ta), len(tb),
                                                                                          len(other), k), *other[:1])
            continue
        same += not diff
        moved += bool(diff)
        offsets += len(diff)
    print("%d kernels in the first build, %d in the second: %d identical, %d with %d line(s) that differ in a number "
          "only, %d that differ otherwise" % (len(a), len(b), same, moved, offsets, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
