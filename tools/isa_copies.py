#!/usr/bin/env python3
"""tools/isa_copies.py [-D...] [--kernel MANGLED-SUBSTRING] [--weights PHASE-STATS.json] [--blocks] — where the register copies of a
render_pool instantiation sit.

The state machine's loop carries a path's whole state (origin, direction, 1/d, distance marched, radiance, throughput, the hit
record, rng, sample index, flags, candidate) from phase to phase.  Whatever the register allocator cannot keep in one place it moves:
`v_mov_b32 vA, vB` at the phases' entries and exits and in the block that leads back to the loop head, `v_cndmask_b32` where the
source selects.  None of it is work the image needs.  This tool counts both, per phase and for the blocks that matter.

Same compile step, phase landmarks and arguments as tools/isa_scratch.py: compiles csrc/render_pool.hip for gfx950 with the
library's flags (+ any -D given), cuts the instantiation's ISA out of hipcc's assembly and attributes every line to a phase
(PROLOGUE, SWAP, SHADE, BLOCK, MODELS, MARCH).  On top of that it reads the basic blocks and their loop comments:

  latch blocks    what runs between the end of a phase and the loop's head.  With the `; chunky-mark phase-end` comments of
                  pool_kernel.inc in the kernel: everything behind the last of them (the census).  Without them (the phases as one
                  if / else-if chain): the blocks of the main loop that control leaves only towards the head — the census, and every
                  block where flows join and whose one way on leads into such a block — each with the phases it is reached from.
  entry block     of a phase: the block of the main loop itself (depth 1) with the most copies ahead of the phase's inner loops —
                  where the phase takes the state out of the loop header's registers.
  exit copies     of a phase: the copies in its other depth-1 blocks (rejoining flow), an upper bound on what one execution issues.

Beside the counts: NumVgprs, ScratchSize, Occupancy.  With --weights (a phase-stats JSON as tools/phase_stats.py writes it, e.g.
profiles/r06_phase_stats_outdoor.json) an estimate of the copies issued per 64 samples: latch x iterations + each phase's entry and
exit copies x that phase's executions.  CPU only (hipcc cross-compiles); `parse` and `attribute` need no compiler."""
import json
import os
import re
import sys

PHASES = ("PROLOGUE", "SWAP", "SHADE", "BLOCK", "MODELS", "WALK", "MARCH", "LATCH")
# lines a phase's code reaches before its first / beyond its last landmark (tools/isa_scratch.py uses the same)
MARGINS = {"swap_before": 250, "swap_after": 60, "models": 40, "shade_after": 40, "march_before": 120}

_LABEL = re.compile(r"^(\.LBB\d+_\d+|; %bb\.\d+):")
_VREG = r"v\d+"
_COPY = re.compile(r"^\s*v_mov_b32_e(?:32|64)\s+(%s),\s*(%s)\s*(?:;.*)?$" % (_VREG, _VREG))
_CNDMASK = re.compile(r"^\s*v_cndmask_b32")
_BRANCH = re.compile(r"^\s*(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


def is_copy(line):
    """a register-to-register v_mov_b32 (constants, literals and scalar sources are not copies of path state)"""
    return bool(_COPY.match(line))


def is_cndmask(line):
    return bool(_CNDMASK.match(line))


def is_instruction(line):
    s = line.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":")


class Block:
    def __init__(self, label, start):
        self.label, self.start = label, start
        self.depth = 0          # loop depth as the assembler comments state it
        self.header = None      # label of the innermost loop's header ("in Loop: Header=BB1_4") or its own if it is one
        self.is_header = False
        self.lines = []         # (index into the body, text) of its instructions
        self.targets = []       # labels it branches to
        self.falls = True       # control can fall into the next block

    def count(self, pred):
        return sum(1 for _, ln in self.lines if pred(ln))


def parse(body):
    """basic blocks of a kernel's assembly (a list of lines), in program order"""
    blocks = [Block("(entry)", 0)]
    for i, ln in enumerate(body):
        m = _LABEL.match(ln)
        if m:
            name = m.group(1)
            blocks.append(Block(name if name.startswith(".") else name[3:], i))
        b = blocks[-1]
        c = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", ln)
        if c:
            b.depth, b.is_header, b.header = int(c.group(1)), True, b.label
            continue
        c = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", ln)
        if c:
            b.header, b.depth = ".L" + c.group(1), int(c.group(2))
            continue
        if m or not is_instruction(ln):
            continue
        b.lines.append((i, ln))
        br = _BRANCH.match(ln)
        if br:
            b.targets.append(br.group(2))
            if br.group(1) == "s_branch":
                b.falls = False
        elif re.match(r"^\s*(s_endpgm|s_setpc_b64)", ln):
            b.falls = False
    return blocks


def landmarks(body):
    marks = {p: [] for p in ("MARCH", "SWAP", "SHADE", "PROLOGUE", "MODELS", "MODELS-END")}
    for i, ln in enumerate(body):
        if "v_cvt_flr_i32_f32" in ln:
            marks["MARCH"].append(i)
        elif "ds_wrxchg_rtn_b64" in ln:
            marks["SWAP"].append(i)
        elif re.search(r"global_store_dword.* nt", ln) or "global_atomic_add" in ln:
            marks["SHADE"].append(i)
        elif "s_getreg_b32" in ln:
            marks["PROLOGUE"].append(i)
        elif "chunky-mark models-end" in ln:
            marks["MODELS-END"].append(i)
        elif "chunky-mark models" in ln:
            marks["MODELS"].append(i)
    return marks


# the comments pool_kernel.inc leaves where a phase's code ends (CHUNKY_PHASE_END), in the loop's order
_PHASE_ENDS = {"march": "MARCH", "block": "BLOCK", "model-blocks": "MODELS", "walk": "WALK", "shade": "SHADE"}


def phase_ends(body):
    """(line, phase) of every `; chunky-mark phase-end NAME` comment, in program order"""
    out = []
    for i, ln in enumerate(body):
        m = re.search(r"chunky-mark phase-end ([a-z-]+)", ln)
        if m and m.group(1) in _PHASE_ENDS:
            out.append((i, _PHASE_ENDS[m.group(1)]))
    return out


def phase_function(body, margins=MARGINS, shade_end=0, header_line=None):
    """line index -> phase.  A kernel whose phases are consecutive ifs says where each one ends (phase_ends): what lies between the swap
    and the first mark, or between two marks, is the phase the closing mark names, what follows the last one is the loop's LATCH (the
    census).  A kernel without the marks (the phases as one if / else-if chain) is cut by the landmarks no other phase contains, as
    tools/isa_scratch.py always did: the phases are contiguous regions in the program order SWAP, SHADE, BLOCK, MARCH.
    `shade_end`: a line known to end SHADE (see attribute), where that is further down than its last landmark + margin;
    `header_line`: where the main loop's header block starts."""
    mk = landmarks(body)
    first_swap, last_swap = min(mk["SWAP"], default=0), max(mk["SWAP"], default=0)
    ends = phase_ends(body)
    if ends:
        # (the compiler may rotate the loop: the census, and with it the last phase's mark, then stands ahead of the loop's head in program
        # order, and what follows the last mark further down is that last phase)
        rotated = ends[0] if len(ends) > 1 and ends[0][1] == "SHADE" else None  # (SHADE is the last phase of the loop)
        rest = ends[1:] if rotated else ends
        head = header_line if header_line is not None else first_swap - margins["swap_before"]

        def phase_of(i):
            if rotated and i <= rotated[0]:
                return rotated[1]
            if i < head:
                return "LATCH" if rotated else "PROLOGUE"
            if i <= last_swap + margins["swap_after"] and (not rest or i < rest[0][0]):
                return "SWAP"
            for line, name in rest:
                if i <= line:
                    return name
            return rotated[1] if rotated else "LATCH"
        return phase_of
    last_shade = max(mk["SHADE"], default=0)
    first_march = min(mk["MARCH"], default=len(body))
    first_models, last_models = min(mk["MODELS"], default=None), max(mk["MODELS-END"], default=None)

    def phase_of(i):
        if i < first_swap - margins["swap_before"]:
            return "PROLOGUE"
        if i <= last_swap + margins["swap_after"]:
            return "SWAP"
        if first_models is not None and last_models is not None and first_models - margins["models"] <= i <= last_models + margins["models"]:
            return "MODELS"
        if i <= max(last_shade + margins["shade_after"], shade_end):
            return "SHADE"
        if i < first_march - margins["march_before"]:
            return "BLOCK"
        return "MARCH"
    return phase_of


def attribute(body, margins=MARGINS):
    """counts of register copies and v_cndmask_b32: per phase, for the main loop's latch blocks and for each phase's entry block"""
    blocks = parse(body)
    by_label = {b.label: b for b in blocks}
    mk = landmarks(body)
    marked = bool(phase_ends(body))
    # the main loop: the depth-1 loop that holds the swap (every phase is inside it)
    main = None
    for b in blocks:
        if b.depth >= 1 and any(i in mk["SWAP"] for i, _ in b.lines):
            h = by_label.get(b.header)
            while h is not None and h.depth > 1:  # (the swap inside an inner loop: climb to the enclosing headers by program order)
                h = next((x for x in reversed(blocks[:blocks.index(h)]) if x.is_header and x.depth == h.depth - 1), None)
            main = h
            break
    if main is None:
        main = next((b for b in blocks if b.is_header and b.depth == 1), None)
    succ, pred = {}, {b.label: [] for b in blocks}
    for k, b in enumerate(blocks):
        s = list(b.targets)
        if b.falls and k + 1 < len(blocks):
            s.append(blocks[k + 1].label)
        succ[b.label] = s
        for t in s:
            pred.setdefault(t, []).append(b.label)

    # Without the marks, the latch blocks are found in the flow graph: the blocks of the main loop that control leaves only towards the
    # loop's head (a way out of the loop does not count) — the census, and every block where flows join and whose one way on leads into such a block
    chain = set()
    if main is not None and not marked:
        grew = True
        while grew:
            grew = False
            for b in blocks:
                if b.label in chain or b.depth != 1 or b.header != main.label or b.is_header:
                    continue
                s = [t for t in succ[b.label] if by_label[t].depth >= 1]
                if main.label not in s and len(pred[b.label]) < 2:  # (the straight-line tail of one phase is that phase's)
                    continue
                if s and all(t == main.label or t in chain for t in s) and (chain or main.label in s):
                    chain.add(b.label)
                    grew = True
    # (there SHADE is the last alternative of the if-chain: its code — new samples, trace_setup — runs down to the latch block the
    # compiler puts behind it, far beyond SHADE's last landmark; when that block lies between SHADE's landmarks and the march loops, SHADE ends with it)
    lo, hi = max(mk["SHADE"], default=0), min(mk["MARCH"], default=len(body))
    ends = [b.lines[-1][0] for b in blocks if b.label in chain and b.lines and lo < b.start < hi]
    phase_of = phase_function(body, margins, max(ends, default=0), main.start if main is not None else None)

    def phase_of_block(b):
        if b.depth == 0:
            return "PROLOGUE"
        if b.label in chain:
            return "LATCH"
        return phase_of(b.lines[0][0] if b.lines else b.start)

    per_phase = {p: {"copies": 0, "cndmask": 0, "valu": 0} for p in PHASES}
    for b in blocks:
        ph = phase_of_block(b)
        for i, ln in b.lines:
            per_phase[ph]["copies"] += is_copy(ln)
            per_phase[ph]["cndmask"] += is_cndmask(ln)
            per_phase[ph]["valu"] += ln.strip().startswith("v_")
    latch = [b for b in blocks if b.depth >= 1 and phase_of_block(b) == "LATCH"]

    # which phases' iterations pass through a latch block: with the marks all of them; in the if-chain layout the phases it can be reached from
    def reached_from(b):
        seen, todo, found = set(), [b.label], set()
        while todo:
            for q in pred.get(todo.pop(), []):
                if q in seen or q not in by_label:
                    continue
                seen.add(q)
                x = by_label[q]
                if x.depth == 0 or x.is_header and x.depth == 1:
                    continue
                if x.label in chain:
                    todo.append(q)
                else:
                    found.add(phase_of_block(x))
        return found
    latch_phases = {b.label: (None if marked else reached_from(b)) for b in latch}

    # a phase's entry block: the depth-1 block with the most copies ahead of the phase's first inner loop or landmark; the rest are its exits
    entry, exits, inner = {}, {}, {}
    for p in PHASES:
        mine = [b for b in blocks if b.depth == 1 and not b.is_header and phase_of_block(b) == p]
        deeper = [b.start for b in blocks if b.depth >= 2 and phase_of_block(b) == p]
        stop = min(deeper, default=None)
        cand = [b for b in mine if b.count(is_copy) and (stop is None or b.start < stop)]
        e = max(cand, key=lambda b: b.count(is_copy)) if cand else None
        entry[p] = e
        exits[p] = sum(b.count(is_copy) for b in mine if b is not e)
        inner[p] = sum(b.count(is_copy) for b in blocks if b.depth >= 2 and phase_of_block(b) == p)
    return {"blocks": blocks, "main": main, "per_phase": per_phase, "latch": latch, "latch_phases": latch_phases, "entry": entry,
            "exit_copies": exits, "inner_copies": inner, "phase_of_block": phase_of_block, "marked": marked}


def weighted_estimate(result, stats):
    """Copies issued per 64 samples, as an upper bound: every block of the main loop itself (depth 1) counted once per execution of its
    phase — latch x iterations + (entry + exit copies) x executions of each phase; copies inside inner loops are left out (their trip
    counts are not in the statistics).  `stats`: a phase-stats JSON; its "execs_per_sample" are a wave's executions per 64 samples — for
    the march that is steps, so the march's weight is loop.march_entries_per_64_samples — loop.iterations_per_64_samples the passes
    through the loop, swaps.rounds_per_sample those that swapped."""
    loop = stats["loop"]
    weight = {"MARCH": float(loop["march_entries_per_64_samples"]), "BLOCK": float(stats["block"]["execs_per_sample"]),
              "MODELS": float(stats.get("model", {}).get("execs_per_sample", 0.0)), "SHADE": float(stats["shade"]["execs_per_sample"]),
              "SWAP": float(stats.get("swaps", {}).get("rounds_per_sample", loop["iterations_per_64_samples"])), "WALK": 0.0}
    iterations = float(loop["iterations_per_64_samples"])
    rows = []
    for b in result["latch"]:
        n = b.count(is_copy)
        via = result["latch_phases"].get(b.label)
        w = iterations if via is None else min(iterations, sum(weight.get(p, 0.0) for p in via))
        if n:
            rows.append((f"latch {b.label}", n, w))
    for p in ("SWAP", "MARCH", "BLOCK", "MODELS", "SHADE"):
        e = result["entry"].get(p)
        rows.append((p, (e.count(is_copy) if e else 0) + result["exit_copies"].get(p, 0), weight[p]))
    return rows, sum(n * w for _, n, w in rows)


def compile_kernel(kernel, extra):
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from chunkyclplugin_amd import native
    flags = [f for f in native.HIPCC_FLAGS if f != "-shared"] + extra
    # (the entity-BVH instantiations — the fourth template argument true — are compiled in render_pool_bvh.hip)
    # (digits only between the markers: `\w+` would run across them and take the sorted kernel's last flag for the fourth argument)
    unit = "render_pool_bvh" if re.search(r"render_poolILin?\d+ELi\d+ELb[01]ELb1E", kernel) else "render_pool"
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["hipcc", *flags, "-x", "hip", "-c", os.path.join(native.CSRC, unit + ".hip"), "-o", os.path.join(td, "rp.o"), "--save-temps"],
                       cwd=td, check=True, capture_output=True)
        text = open(os.path.join(td, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    return cut_kernel(text, kernel)


def cut_kernel(text, kernel):
    found = [i for i, ln in enumerate(text) if ln.startswith("_ZN6chunky") and kernel in ln and ln.rstrip().split(":")[0].endswith("E") and ":" in ln]
    # (the substring names chunky::render_pool and chunky::proj::render_pool alike: the pinhole kernel unless proj is asked for)
    start = next((i for i in found if ("4proj" in text[i]) == ("proj" in kernel)), found[0])
    end = next(i for i in range(start, len(text)) if ".end_amdhsa_kernel" in text[i])
    tail = text[end:end + 60]  # the resource comments follow the kernel descriptor
    meta = {k: next((re.search(r"(\d+)", ln.split(k)[1]).group(1) for ln in tail if k in ln), None)
            for k in ("; NumVgprs:", "; ScratchSize:", "; Occupancy:")}
    return text[start].split(":")[0], text[start:end], meta


def main(args):
    kernel = "render_poolILi17ELi64ELb0ELb0ELb0ELb0EE"  # (render_pool<17, 64, false, false, false, false>; the last flag: sorted block tests)
    weights, show_blocks, asm = None, False, None
    for opt in ("--kernel", "--weights", "--asm"):
        if opt in args:
            i = args.index(opt)
            val = args[i + 1]
            del args[i:i + 2]
            if opt == "--kernel":
                kernel = val
            elif opt == "--weights":
                weights = val
            else:
                asm = val  # an assembly file compiled earlier (hipcc --save-temps), instead of compiling
    if "--blocks" in args:
        args.remove("--blocks")
        show_blocks = True
    name, body, meta = cut_kernel(open(asm).read().splitlines(), kernel) if asm else compile_kernel(kernel, args)
    r = attribute(body)
    print(f"# {name}")
    print(f"# NumVgprs {meta['; NumVgprs:']}  ScratchSize {meta['; ScratchSize:']}  Occupancy {meta['; Occupancy:']}  flags: {' '.join(args) or '(library defaults)'}")
    tot = {k: sum(v[k] for v in r["per_phase"].values()) for k in ("copies", "cndmask", "valu")}
    print(f"# whole kernel: {tot['valu']} VALU instructions, {tot['copies']} register-to-register v_mov_b32, {tot['cndmask']} v_cndmask_b32")
    print("phase      copies  cndmask   VALU")
    for p in PHASES:
        v = r["per_phase"][p]
        print(f"{p:10s} {v['copies']:6d} {v['cndmask']:8d} {v['valu']:6d}")
    print(f"main loop header: {r['main'].label if r['main'] else '(not found)'}; phases cut by {'the phase-end marks' if r['marked'] else 'landmarks (no phase-end marks: the if / else-if layout)'}")
    for b in r["latch"]:
        via = r["latch_phases"][b.label]
        if b.count(is_copy) or b.count(is_cndmask):
            print(f"latch block {b.label:12s} line {b.start:5d}: {b.count(is_copy):3d} copies, {b.count(is_cndmask):3d} cndmask; reached from {'every phase' if via is None else ', '.join(sorted(via)) or '-'}")
    print(f"latch total: {sum(b.count(is_copy) for b in r['latch'])} copies in {len(r['latch'])} blocks; the largest block: {max((b.count(is_copy) for b in r['latch']), default=0)}")
    for p in ("SWAP", "SHADE", "BLOCK", "MODELS", "MARCH"):
        e = r["entry"][p]
        where = f"{e.label:12s} line {e.start:5d}: {e.count(is_copy):3d} copies, {e.count(is_cndmask):3d} cndmask" if e is not None else "(no depth-1 block with copies ahead of its loops)"
        print(f"entry block of {p:7s} {where}; its other depth-1 blocks: {r['exit_copies'][p]} copies; in its inner loops: {r['inner_copies'][p]}")
    if show_blocks:
        for b in r["blocks"]:
            n = b.count(is_copy)
            if n >= 3:
                print(f"  {b.label:12s} line {b.start:5d} depth {b.depth} {r['phase_of_block'](b):8s} {n:3d} copies {b.count(is_cndmask):3d} cndmask of {len(b.lines)} instructions")
    if weights:
        rows, total = weighted_estimate(r, json.load(open(weights)))
        print(f"# estimate per 64 samples ({weights}):")
        for nm, n, w in rows:
            print(f"  {nm:18s} {n:4d} copies x {w:6.2f} = {n * w:8.1f}")
        print(f"  total   {total:8.1f} copies per 64 samples (an upper bound: each depth-1 block once per execution of its phase)")


if __name__ == "__main__":
    main(sys.argv[1:])
