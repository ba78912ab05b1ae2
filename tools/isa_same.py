#!/usr/bin/env python3
"""Do two assembly files (hipcc --cuda-device-only -S, before and after a change) hold the same kernels?  The same set of kernel
symbols, and for each the same instructions and the same kernel descriptor once comments are dropped and the function index inside
local labels (.LBB12_3, .LJTI12_0) is taken out; the order of the kernels in the file is free.  CPU only.
    python tools/isa_same.py before.s after.s     exit status 0 = the same, 1 = not (the differences are printed)"""
import re
import sys

_LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")


def kernels(lines):
    """{kernel symbol: normalised lines of its body and its .amdhsa_kernel descriptor}"""
    names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
    out, cur = {}, None
    for l in lines:
        head = l.split(";", 1)[0].strip()
        if head.endswith(":") and head[:-1] in names:  # the entry label: the body, then the descriptor, run to .Lfunc_end
            cur = out.setdefault(head[:-1], [])
        elif head.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and head:
            cur.append(_LOCAL.sub(r".L\1_\2", head))
    return out


def compare(before, after):
    """the differences between two assembly texts (lists of lines), as messages; empty = the same kernels"""
    a, b = kernels(before), kernels(after)
    msgs = [f"only before: {n}" for n in sorted(set(a) - set(b))] + [f"only after: {n}" for n in sorted(set(b) - set(a))]
    for n in sorted(set(a) & set(b)):
        if a[n] != b[n]:
            i = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            msgs.append(f"{n}: differs at instruction {i}: {a[n][i] if i < len(a[n]) else '(end)'!r} / {b[n][i] if i < len(b[n]) else '(end)'!r}")
    return msgs


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    before, after = (open(p).read().splitlines() for p in sys.argv[1:3])
    msgs = compare(before, after)
    print("\n".join(msgs) if msgs else f"same: {len(kernels(before))} kernels")
    sys.exit(1 if msgs else 0)
