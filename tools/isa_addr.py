#!/usr/bin/env python3
"""tools/isa_addr.py [-D...] [--kernel MANGLED-SUBSTRING] [--asm FILE] [--sites] [--weights PHASE-STATS.json] — the address arithmetic of a
render_pool instantiation, per phase and per basic block.

A scene array indexed with a sign-extended `int` or a `size_t` product off a per-lane 64-bit pointer costs a sign extension
(`v_ashrrev_i32 …, 31`), a 64-bit shift-add (`v_lshl_add_u64`) and, where the index is a product, integer multiplies
(`v_mul_lo_u32`, `v_mad_u64_u32`, `v_mad_i64_i32`), and the load then takes its address from a VGPR pair (`v[a:a+1], off`).  The
same read as a 32-bit byte offset off a kernel-argument pointer is `global_load_* v, v_off, s[base:base+1]`: no pair, no extension.

Same compile step, kernel cut and phase cut as tools/isa_copies.py.  Listed per phase:

  integer multiplies   v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32, v_mad_i64_i32, each attributed to its use:
                         address        the result reaches, through adds, left shifts, sign extensions and copies inside its basic
                                        block, the address operand of a global load / store or a 64-bit shift-add
                         fast_quotient  v_mul_hi_u32 (the division by an invariant, pool_walk.hpp) and the v_mul_lo_u32 that takes the
                                        remainder from it
                         pcg/other      everything else (the PCG steps multiply and then xor / shift right: no address)
  64-bit address pieces v_lshl_add_u64; `v_ashrrev_i32 vN, 31, vM` whose result only feeds one (or a 64-bit multiply-add);
                        v_add_co_u32 / v_addc_co_u32 pairs
  memory instructions  every global_load_* / global_store_* / global_atomic_* with its form: `saddr` (SGPR base + 32-bit VGPR offset)
                        or `vaddr64` (a VGPR pair, `off`)

With --sites every multiply and every 64-bit-address load with its line, phase, block and attribution.  With --weights an upper-bound
estimate of the address instructions issued per 64 samples, as isa_copies.py's: each depth-1 block once per execution of its phase.

CPU only (hipcc cross-compiles); `scan`, `summary` and `report` need no compiler."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_copies  # noqa: E402
from isa_divsqrt import opcode  # noqa: E402

MULS = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mad_i64_i32")
COLS = MULS + ("mul_address", "mul_fast_quotient", "mul_other", "v_lshl_add_u64", "sext_for_address", "add_co_pairs", "mem_saddr", "mem_vaddr64")
# instructions that carry an index on towards an address (a value that passes an xor or a right shift is no index any more)
_CARRY = ("v_add_u32", "v_add3_u32", "v_add_lshl_u32", "v_lshl_add_u32", "v_lshl_add_u64", "v_lshlrev_b32", "v_lshlrev_b64", "v_ashrrev_i32",
          "v_mad_u64_u32", "v_mad_i64_i32", "v_mad_u32_u24", "v_mul_u32_u24", "v_mul_lo_u32", "v_mov_b32", "v_add_co_u32", "v_addc_co_u32",
          "v_lshl_or_b32", "v_or_b32", "v_sub_u32", "v_subrev_u32", "v_mad_i32_i24", "v_lshl_add_u32")
_MEM = re.compile(r"^(global_load|global_store|global_atomic)")
_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def vregs(text):
    """the VGPR numbers an operand string names (v3 -> {3}, v[4:5] -> {4, 5})"""
    out = set()
    for m in _REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def operands(line):
    """(destination operand, [source operands]) of an instruction line, as text; a store has no destination"""
    s = line.split(";")[0].strip()
    parts = s.split(None, 1)
    ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    # (v[4:5] holds no comma; s[0:1] neither)
    op = opcode(line) or ""
    if op.startswith(("global_store", "global_atomic")) and "_rtn" not in op:
        return None, ops
    return (ops[0] if ops else None), ops[1:]


def mem_form(line):
    """'saddr' or 'vaddr64' of a global_* instruction"""
    dst, src = operands(line)
    ops = ([dst] if dst is not None else []) + src
    return "vaddr64" if any(o.split()[0] == "off" for o in ops) else "saddr"


def mem_address(line):
    """the VGPRs that hold the address (pair) or the offset of a global_* instruction"""
    _, src = operands(line)   # (a store or an atomic without return has no destination: its address is the first operand too)
    return vregs(src[0]) if src else set()


def reaches_address(block_lines, k):
    """does the result of instruction k of a block reach an address operand inside the block (see the module's text)?"""
    dst, _ = operands(block_lines[k][1])
    live = vregs(dst or "")
    for _, ln in block_lines[k + 1:]:
        if not live:
            return False
        op = opcode(ln)
        d, src = operands(ln)
        used = set().union(*[vregs(s) for s in src]) if src else set()
        if _MEM.match(op):
            if mem_address(ln) & live:
                return True
            if d is not None:
                live -= vregs(d)
            continue
        if op == "v_lshl_add_u64" and used & live:
            return True
        if used & live and op in _CARRY:
            live |= vregs(d or "")
        elif d is not None and op.startswith("v_"):
            live -= vregs(d)
    return False


def is_sext(line):
    return opcode(line) == "v_ashrrev_i32" and re.search(r"v_ashrrev_i32\S*\s+v\d+,\s*31,\s*v\d+", line) is not None


def sext_only_feeds_address(block_lines, k):
    """a `v_ashrrev_i32 vN, 31, vM` whose result is read only by 64-bit address instructions of its block"""
    dst, _ = operands(block_lines[k][1])
    reg = vregs(dst)
    fed = False
    for _, ln in block_lines[k + 1:]:
        op = opcode(ln)
        d, src = operands(ln)
        used = set().union(*[vregs(s) for s in src]) if src else set()
        if used & reg:
            if op in ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_lshlrev_b64", "v_mul_lo_u32", "v_add3_u32", "v_addc_co_u32") or (_MEM.match(op) and mem_form(ln) == "vaddr64"):
                fed = True
            else:
                return False
        if d is not None and vregs(d) & reg:  # overwritten
            break
    return fed


def scan(body, phase_of=None):
    """(per-phase counts {phase: {column: n}}, sites [{line, phase, op, use, block, depth}]) of a kernel's assembly"""
    blocks = isa_copies.parse(body)
    per, sites = {}, []
    for b in blocks:
        for k, (i, ln) in enumerate(b.lines):
            op = opcode(ln)
            ph = phase_of(i) if phase_of else "KERNEL"
            row = per.setdefault(ph, dict({"valu": 0}, **{c: 0 for c in COLS}))
            row["valu"] += op.startswith("v_")
            use = None
            if op in MULS:
                row[op] += 1
                if reaches_address(b.lines, k):
                    use = "address"
                elif op == "v_mul_hi_u32" or (op == "v_mul_lo_u32" and any(opcode(x) == "v_mul_hi_u32" for _, x in b.lines[max(0, k - 6):k])):
                    use = "fast_quotient"
                else:
                    use = "pcg/other"
                row["mul_" + use.replace("pcg/", "")] += 1
            elif op == "v_lshl_add_u64":
                row[op] += 1
                use = "address"
            elif is_sext(ln) and sext_only_feeds_address(b.lines, k):
                row["sext_for_address"] += 1
                use = "address"
            elif op == "v_addc_co_u32":
                row["add_co_pairs"] += 1
                use = "address"
            elif _MEM.match(op):
                form = mem_form(ln)
                row["mem_" + form] += 1
                use = form
            if use is not None:
                sites.append({"line": i, "phase": ph, "op": op, "use": use, "block": b.label, "depth": b.depth})
    return per, sites


def summary(per):
    tot = dict({"valu": 0}, **{c: 0 for c in COLS})
    for row in per.values():
        for k, v in row.items():
            tot[k] += v
    return tot


def address_instructions(row):
    """the instructions of a row that exist only to form a 64-bit address"""
    return row["mul_address"] + row["v_lshl_add_u64"] + row["sext_for_address"] + 2 * row["add_co_pairs"]


def report(per, sites=None):
    lines = ["phase        VALU  mul_lo mul_hi mad_u64 mad_i64 | address quotient  other | lshl_add_u64  sext  add_co | loads/stores: saddr vaddr64"]
    rows = [(p, per[p]) for p in isa_copies.PHASES + ("KERNEL",) if p in per] + [("(whole)", summary(per))]
    for p, r in rows:
        lines.append(f"{p:10s} {r['valu']:6d} {r['v_mul_lo_u32']:7d} {r['v_mul_hi_u32']:6d} {r['v_mad_u64_u32']:7d} {r['v_mad_i64_i32']:7d} | "
                     f"{r['mul_address']:7d} {r['mul_fast_quotient']:8d} {r['mul_other']:6d} | {r['v_lshl_add_u64']:12d} {r['sext_for_address']:5d} "
                     f"{r['add_co_pairs']:7d} | {r['mem_saddr']:19d} {r['mem_vaddr64']:7d}")
    if sites is not None:
        lines.append("line    phase      instruction              use            block        depth")
        for s in sites:
            if s["use"] == "saddr":
                continue
            lines.append(f"{s['line']:6d}  {s['phase']:10s} {s['op']:24s} {s['use']:14s} {s['block']:12s} {s['depth']:5d}")
    return lines


def weighted_estimate(body, phase_of, stats):
    """address instructions issued per 64 samples, as an upper bound: the address instructions of every depth-1 block once per execution
    of its phase (tools/isa_copies.py weighted_estimate has the weights' meaning); blocks of inner loops are left out.  Multiplies count
    once here: their issue cost is tools/ubench_imul.hip's business."""
    loop = stats["loop"]
    weight = {"MARCH": float(loop["march_entries_per_64_samples"]), "BLOCK": float(stats["block"]["execs_per_sample"]),
              "MODELS": float(stats.get("model", {}).get("execs_per_sample", 0.0)), "SHADE": float(stats["shade"]["execs_per_sample"]),
              "SWAP": float(stats.get("swaps", {}).get("rounds_per_sample", loop["iterations_per_64_samples"]))}
    blocks = isa_copies.parse(body)
    rows = {}
    for b in blocks:
        if b.depth != 1 or not b.lines:
            continue
        sub = [body[i] for i, _ in b.lines]
        per, _ = scan(sub)
        n = address_instructions(per.get("KERNEL", dict({"valu": 0}, **{c: 0 for c in COLS})))
        ph = phase_of(b.lines[0][0])
        rows[ph] = rows.get(ph, 0) + n
    out = [(p, n, weight.get(p, 0.0)) for p, n in rows.items() if p in weight]
    return out, sum(n * w for _, n, w in out)


def main(args):
    kernel = "render_poolILi17ELi64ELb0ELb0ELb0ELb0EE"  # (render_pool<17, 64, false, false, false, false>)
    asm, weights, show_sites = None, None, False
    for opt in ("--kernel", "--asm", "--weights"):
        if opt in args:
            i = args.index(opt)
            val = args[i + 1]
            del args[i:i + 2]
            if opt == "--kernel":
                kernel = val
            elif opt == "--asm":
                asm = val
            else:
                weights = val
    if "--sites" in args:
        args.remove("--sites")
        show_sites = True
    name, body, meta = isa_copies.cut_kernel(open(asm).read().splitlines(), kernel) if asm else isa_copies.compile_kernel(kernel, args)
    header = next((i for i, ln in enumerate(body) if "This Loop Header: Depth=1" in ln), None)
    phase_of = isa_copies.phase_function(body, header_line=header)
    per, sites = scan(body, phase_of)
    print(f"# {name}")
    print(f"# NumVgprs {meta['; NumVgprs:']}  ScratchSize {meta['; ScratchSize:']}  Occupancy {meta['; Occupancy:']}  flags: {' '.join(args) or '(library defaults)'}")
    for ln in report(per, sites if show_sites else None):
        print(ln)
    if weights:
        rows, total = weighted_estimate(body, phase_of, json.load(open(weights)))
        print(f"# estimate per 64 samples ({weights}):")
        for p, n, w in rows:
            print(f"  {p:10s} {n:4d} address instructions x {w:6.2f} = {n * w:8.1f}")
        print(f"  total   {total:8.1f} per 64 samples (an upper bound: each depth-1 block once per execution of its phase)")


if __name__ == "__main__":
    main(sys.argv[1:])
