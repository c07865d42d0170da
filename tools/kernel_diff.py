#!/usr/bin/env python3
"""Diff of two builds of the device code, kernel by kernel.  Not a test.

Each argument is the disassembly of one device-only object:

    hipcc <the Makefile's CXXFLAGS> [-DAGX_NEQ=7] [-DAGX_TPG=1] --cuda-device-only \
        --no-gpu-bundle-output -c agx_api.hip -o dev.o
    llvm-objdump -d --no-show-raw-insn --no-leading-addr dev.o > dev.dis

    tools/kernel_diff.py before.dis after.dis

The literal of an s_add_u32 that follows s_getpc_b64 is left out of the comparison: it is the
distance to a called function, which moves with the size of the code in between.  The same
pair of instructions also forms the address of a constant or a global, so a change of such an
address alone does not show here.

Prints the symbols only one side has and the symbols whose instructions differ; exit status 1
when there are any.
"""
import re
import sys


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:\s*$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip():
            # the trailing comment holds absolute addresses, which move with the code around
            # a kernel; the instruction and its (relative) operands are in front of it
            ins = line.split("//")[0].strip()
            # the distance to a function that is called, not inlined (s_getpc_b64, then
            # s_add_u32 with the literal): it changes with the size of the code in between
            if out[name] and out[name][-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
            out[name].append(ins)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    for n in only_a:
        print("only before:", n)
    for n in only_b:
        print("only after: ", n)
    for n in differ:
        print("differs:    ", n, len(a[n]), "->", len(b[n]), "instructions")
    print(f"{len(set(a) & set(b)) - len(differ)} of {len(set(a) | set(b))} symbols identical")
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
