#!/usr/bin/env python3
"""tools/isa_waits.py [-D...] [--kernel MANGLED-SUBSTRING] [--asm FILE] [--phase NAME] — the round trips to memory a wave of a render_pool
instantiation sits out: every `s_waitcnt` of the compiled kernel with the loads it waits for.

A wave that asks for a word and waits for it in the next instruction pays the whole latency of the memory behind it; a wave that asks
for twenty words and waits once pays it once.  The compiler requests a kernel-argument word (`s_load_`) in the basic block that first
uses it, so code that reads the launch arguments field by field becomes a string of single scalar round trips, each fully exposed.
This tool lists them.

Same compile step, kernel cut and phase cut as tools/isa_copies.py (the `; chunky-mark phase-end` comments of pool_kernel.inc).  The
kernel's text is read in program order, one list of outstanding loads per counter:

  lgkmcnt   `s_load_` (scalar: the argument segment) and `ds_` (LDS)
  vmcnt     `global_load_` and `global_atomic_`

Instructions are recognised by these prefixes and nothing else.  For every `s_waitcnt` the report names, per counter it mentions, the
loads of that counter issued since the counter's last full wait (`cnt(0)`); a partial `vmcnt(n)` leaves the n youngest outstanding, a partial
`lgkmcnt(n)` the n youngest LDS operations and every scalar load (those return out of order: only `lgkmcnt(0)` waits for one).  A
wait whose counter has had no load since its last full wait is listed as "nothing new" (it stands at a join of flows, or waits for a
store).  Per phase: the waits, and the count of SCALAR waits that each expose a fresh load — `lgkmcnt(0)` with at least one `s_load_`
outstanding — which is the number of scalar round trips a wave that passes all of the phase's text sits out one after the other.
Program order is not control flow: a branch may skip a wait, so the count is an upper bound for one execution.

CPU only (hipcc cross-compiles); `scan` and `report` need no compiler."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_copies  # noqa: E402

_WAIT = re.compile(r"^\s*s_waitcnt\s+(.*?)\s*(?:;.*)?$")
_CNT = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")
_LGKM = ("s_load_", "ds_")
_VM = ("global_load_", "global_atomic_")


def classify(line):
    """'lgkm' / 'vm' for a load the counters track, 'wait' for s_waitcnt, else None — by prefix alone"""
    s = line.strip()
    if s.startswith("s_waitcnt"):
        return "wait"
    if s.startswith(_LGKM):
        return "lgkm"
    if s.startswith(_VM):
        return "vm"
    return None


def short(line):
    """an instruction without its trailing comment, blanks squeezed"""
    return " ".join(line.split(";")[0].split())


def scan(body, phase_of=None):
    """The waits of a kernel's assembly (a list of lines), in program order: dicts {line, phase, text, waits: {counter: (n, [loads waited
    for], [loads left outstanding])}, scalar_fresh}.  `phase_of`: line index -> phase name (default: one phase, "KERNEL")."""
    pending = {"lgkm": [], "vm": []}
    out = []
    for i, ln in enumerate(body):
        kind = classify(ln)
        if kind in ("lgkm", "vm"):
            pending[kind].append((i, short(ln)))
        elif kind == "wait":
            m = _WAIT.match(ln)
            waits = {}
            for name, n in _CNT.findall(m.group(1) if m else ""):
                n = int(n)
                key = {"vmcnt": "vm", "lgkmcnt": "lgkm"}.get(name)
                if key is None:
                    continue
                q = pending[key]
                if n == 0:
                    keep = []
                elif key == "lgkm":
                    # LDS operations return in order, scalar loads do not: a partial lgkmcnt(n) says nothing about an s_load_ (only
                    # lgkmcnt(0) does), so those stay outstanding; of the ds_ entries the n youngest stay
                    ds = [x for x in q if not x[1].startswith("s_load_")]
                    gone = set(i for i, _ in (ds[:len(ds) - n] if n <= len(ds) else []))
                    keep = [x for x in q if x[0] not in gone]
                else:
                    keep = q[len(q) - n:] if n <= len(q) else list(q)
                done = [x for x in q if x not in keep]
                pending[key] = list(keep)
                waits[name] = (n, done, keep)
            lg = waits.get("lgkmcnt")
            fresh = bool(lg and lg[0] == 0 and any(t.startswith("s_load_") for _, t in lg[1]))
            out.append({"line": i, "phase": phase_of(i) if phase_of else "KERNEL", "text": short(ln), "waits": waits, "scalar_fresh": fresh})
    return out


def summary(waits):
    """per phase: [waits, scalar waits that expose a fresh load, vector waits that expose a fresh load]"""
    per = {}
    for w in waits:
        row = per.setdefault(w["phase"], [0, 0, 0])
        row[0] += 1
        row[1] += w["scalar_fresh"]
        vm = w["waits"].get("vmcnt")
        row[2] += bool(vm and vm[1])
    return per


def report(waits, only=None):
    lines = []
    for w in waits:
        if only and w["phase"] != only:
            continue
        parts = []
        for name, (n, done, keep) in w["waits"].items():
            what = "; ".join(f"{t} @{i}" for i, t in done) if done else "nothing new"
            left = f" (left outstanding: {len(keep)})" if keep else ""
            parts.append(f"{name}({n}): {what}{left}")
        flag = " *" if w["scalar_fresh"] else ""
        lines.append(f"{w['line']:6d}  {w['phase']:8s}{flag:2s} {' | '.join(parts) or w['text']}")
    return lines


def main(args):
    kernel = "render_poolILi17ELi64ELb0ELb0ELb0ELb0EE"  # (render_pool<17, 64, false, false, false, false>)
    asm, only = None, None
    for opt in ("--kernel", "--asm", "--phase"):
        if opt in args:
            i = args.index(opt)
            val = args[i + 1]
            del args[i:i + 2]
            if opt == "--kernel":
                kernel = val
            elif opt == "--asm":
                asm = val
            else:
                only = val.upper()
    name, body, meta = isa_copies.cut_kernel(open(asm).read().splitlines(), kernel) if asm else isa_copies.compile_kernel(kernel, args)
    header = next((i for i, ln in enumerate(body) if "This Loop Header: Depth=1" in ln), None)
    phase_of = isa_copies.phase_function(body, header_line=header)
    waits = scan(body, phase_of)
    print(f"# {name}")
    print(f"# NumVgprs {meta['; NumVgprs:']}  ScratchSize {meta['; ScratchSize:']}  Occupancy {meta['; Occupancy:']}  flags: {' '.join(args) or '(library defaults)'}")
    print("# line (of the kernel's text), phase, * = a scalar wait that exposes a fresh load; per counter: the loads waited for, with their lines")
    for ln in report(waits, only):
        print(ln)
    print("phase      waits  scalar waits exposing a fresh load  vector waits exposing a fresh load")
    per = summary(waits)
    for p in isa_copies.PHASES:
        if p in per and (not only or p == only):
            print(f"{p:10s} {per[p][0]:5d} {per[p][1]:35d} {per[p][2]:34d}")


if __name__ == "__main__":
    main(sys.argv[1:])
