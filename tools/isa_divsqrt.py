#!/usr/bin/env python3
"""tools/isa_divsqrt.py [-D...] [--kernel MANGLED-SUBSTRING] [--asm FILE] [--sites] — the IEEE division and square-root expansions of a
render_pool instantiation, per phase.

`a / b` and `sqrtf` are no single instruction on gfx950.  The compiler expands a float division into 2 `v_div_scale_f32`, a `v_rcp_f32`,
six fma / mul, a `v_div_fmas_f32` and a `v_div_fixup_f32` (11 VALU, one serial chain), a root into `v_sqrt_f32` with a scale-up test,
a +-1 ulp residual test, a scale-down and a class select (15 VALU).  A site that is given a shorter exact form (rt_short_forms.h) keeps
its expansion only behind a wave-uniform branch, in a block of its own; this tool shows what is left and where.

Same compile step, kernel cut and phase cut as tools/isa_copies.py (the `; chunky-mark phase-end` comments of pool_kernel.inc).  Per
phase: the static VALU count and the counts of `v_div_scale_f32`, `v_div_fmas_f32`, `v_div_fixup_f32` (one per division), `v_sqrt_f32`
(one per root, short or expanded), `v_rcp_f32` and `v_rsq_f32`.  With --sites every `v_div_fixup_f32` and `v_sqrt_f32` with its line, its
phase, its basic block and that block's loop depth — a slow path sits in a block that holds little besides the expansion.

CPU only (hipcc cross-compiles); `scan`, `summary` and `report` need no compiler."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_copies  # noqa: E402

OPS = ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_sqrt_f32", "v_rcp_f32", "v_rsq_f32")
SITES = ("v_div_fixup_f32", "v_sqrt_f32")


def opcode(line):
    """the mnemonic of an instruction line without its encoding suffix (`v_sqrt_f32_e32` -> `v_sqrt_f32`), or None"""
    if not isa_copies.is_instruction(line):
        return None
    op = line.split(";")[0].split()[0]
    for suffix in ("_e32", "_e64", "_dpp", "_sdwa"):
        if op.endswith(suffix):
            op = op[:-len(suffix)]
    return op


def scan(body, phase_of=None):
    """(per-phase counts {phase: {"valu": n, op: n, ...}}, sites [{line, phase, op, block, depth, block_valu}]) of a kernel's assembly"""
    blocks = isa_copies.parse(body)
    block_of = {}
    for b in blocks:
        for i, _ in b.lines:
            block_of[i] = b
    per, sites = {}, []
    for i, ln in enumerate(body):
        op = opcode(ln)
        if op is None:
            continue
        ph = phase_of(i) if phase_of else "KERNEL"
        row = per.setdefault(ph, dict({"valu": 0}, **{o: 0 for o in OPS}))
        row["valu"] += op.startswith("v_")
        if op in OPS:
            row[op] += 1
        if op in SITES:
            b = block_of.get(i)
            sites.append({"line": i, "phase": ph, "op": op, "block": b.label if b else "?", "depth": b.depth if b else 0,
                          "block_valu": b.count(lambda x: x.strip().startswith("v_")) if b else 0})
    return per, sites


def summary(per):
    """the whole kernel's row"""
    tot = dict({"valu": 0}, **{o: 0 for o in OPS})
    for row in per.values():
        for k, v in row.items():
            tot[k] += v
    return tot


def report(per, sites=None):
    lines = ["phase        VALU  div_scale  div_fmas  div_fixup   sqrt    rcp    rsq"]
    rows = [(p, per[p]) for p in isa_copies.PHASES + ("KERNEL",) if p in per] + [("(whole)", summary(per))]
    for p, r in rows:
        lines.append(f"{p:10s} {r['valu']:6d} {r['v_div_scale_f32']:10d} {r['v_div_fmas_f32']:9d} {r['v_div_fixup_f32']:10d} "
                     f"{r['v_sqrt_f32']:6d} {r['v_rcp_f32']:6d} {r['v_rsq_f32']:6d}")
    if sites is not None:
        lines.append("line    phase      instruction       block        depth  VALU in the block")
        for s in sites:
            lines.append(f"{s['line']:6d}  {s['phase']:10s} {s['op']:17s} {s['block']:12s} {s['depth']:5d} {s['block_valu']:6d}")
    return lines


def main(args):
    kernel = "render_poolILi17ELi64ELb0ELb0ELb0ELb0EE"  # (render_pool<17, 64, false, false, false, false>)
    asm, show_sites = None, False
    for opt in ("--kernel", "--asm"):
        if opt in args:
            i = args.index(opt)
            val = args[i + 1]
            del args[i:i + 2]
            if opt == "--kernel":
                kernel = val
            else:
                asm = val
    if "--sites" in args:
        args.remove("--sites")
        show_sites = True
    name, body, meta = isa_copies.cut_kernel(open(asm).read().splitlines(), kernel) if asm else isa_copies.compile_kernel(kernel, args)
    header = next((i for i, ln in enumerate(body) if "This Loop Header: Depth=1" in ln), None)
    per, sites = scan(body, isa_copies.phase_function(body, header_line=header))
    print(f"# {name}")
    print(f"# NumVgprs {meta['; NumVgprs:']}  ScratchSize {meta['; ScratchSize:']}  Occupancy {meta['; Occupancy:']}  flags: {' '.join(args) or '(library defaults)'}")
    for ln in report(per, sites if show_sites else None):
        print(ln)


if __name__ == "__main__":
    main(sys.argv[1:])
