"""tools/isa_divsqrt.py on canned assembly (no compiler, no GPU): a division's expansion counted once by its v_div_fixup_f32, a root
by its v_sqrt_f32 whatever its encoding suffix, the static VALU count, the cut into phases by the kernel's `; chunky-mark phase-end`
comments, and the block a site sits in — a slow path stands in a small block of its own, behind a branch."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_copies  # noqa: E402
import isa_divsqrt  # noqa: E402


def asm(text):
    return ["\t" + ln.strip() if not ln.strip().startswith((".", ";")) or ln.strip().startswith("; chunky") else ln.strip()
            for ln in text.strip().splitlines()]


DIVISION = """
    v_div_scale_f32 v3, s[0:1], v2, v2, 1.0
    v_rcp_f32_e32 v4, v3
    v_div_scale_f32 v5, vcc, 1.0, v2, 1.0
    v_fma_f32 v8, -v3, v4, 1.0
    v_fmac_f32_e32 v4, v8, v4
    v_mul_f32_e32 v8, v5, v4
    v_fma_f32 v9, -v3, v8, v5
    v_fmac_f32_e32 v8, v9, v4
    v_fma_f32 v3, -v3, v8, v5
    v_div_fmas_f32 v3, v3, v4, v8
    v_div_fixup_f32 v2, v3, v2, 1.0
"""

KERNEL = """
    s_load_dwordx2 s[2:3], s[0:1], 0x0
    v_sqrt_f32_e32 v1, v0
.LBB0_1:                                ; =>This Loop Header: Depth=1
    ds_wrxchg_rtn_b64 v[0:1], v2, v[0:1]
    s_waitcnt lgkmcnt(0)
    v_cvt_flr_i32_f32_e32 v3, v4
    ; chunky-mark phase-end march
""" + DIVISION + """
    v_div_fixup_f64 v[2:3], v[4:5], s[0:1], v[2:3]
    ; chunky-mark phase-end block
    ; chunky-mark phase-end model-blocks
    ; chunky-mark phase-end walk
    v_rcp_f32_e32 v2, v6
    v_fma_f32 v4, -v6, v2, 1.0
    v_fmac_f32_e32 v2, v2, v4
    v_cmp_ge_f32_e64 s[0:1], |v6|, s4
    s_cbranch_vccz .LBB0_3
.LBB0_2:                                ;   in Loop: Header=BB0_1 Depth=1
    ;;#ASMSTART
    ; chunky-mark exact-slow-path
    ;;#ASMEND
""" + DIVISION + """
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
    v_rsq_f32_e32 v2, v6
    v_sqrt_f32_e64 v3, |v6|
    global_store_dword v[4:5], v2, off nt
    ; chunky-mark phase-end shade
    s_cbranch_scc1 .LBB0_1
    s_endpgm
"""


def scanned():
    body = asm(KERNEL)
    header = next(i for i, ln in enumerate(body) if "Loop Header: Depth=1" in ln)
    phase_of = isa_copies.phase_function(body, margins={**isa_copies.MARGINS, "swap_after": 1}, header_line=header)
    return body, isa_divsqrt.scan(body, phase_of)


def test_opcode_drops_the_encoding_suffix_only():
    assert isa_divsqrt.opcode("\tv_sqrt_f32_e32 v1, v0") == "v_sqrt_f32"
    assert isa_divsqrt.opcode("\tv_sqrt_f32_e64 v3, |v6|") == "v_sqrt_f32"
    assert isa_divsqrt.opcode("\tv_div_fixup_f32 v2, v3, v2, 1.0") == "v_div_fixup_f32"
    assert isa_divsqrt.opcode("\tv_div_fixup_f64 v[2:3], v[4:5], s[0:1], v[2:3]") == "v_div_fixup_f64"   # a double division is not counted
    assert isa_divsqrt.opcode("; v_sqrt_f32 in a comment") is None and isa_divsqrt.opcode(".LBB0_2:") is None


def test_counts_per_phase():
    _, (per, _) = scanned()
    assert per["PROLOGUE"]["v_sqrt_f32"] == 1 and per["PROLOGUE"]["valu"] == 1
    assert per["MARCH"]["valu"] == 1 and not any(per["MARCH"][o] for o in isa_divsqrt.OPS)
    b = per["BLOCK"]
    assert (b["v_div_scale_f32"], b["v_div_fmas_f32"], b["v_div_fixup_f32"], b["v_rcp_f32"], b["v_sqrt_f32"], b["valu"]) == (2, 1, 1, 1, 0, 12)
    s = per["SHADE"]
    assert (s["v_div_scale_f32"], s["v_div_fmas_f32"], s["v_div_fixup_f32"], s["v_rcp_f32"], s["v_rsq_f32"], s["v_sqrt_f32"]) == (2, 1, 1, 2, 1, 1)
    assert s["valu"] == 4 + 11 + 2
    tot = isa_divsqrt.summary(per)
    assert tot["v_div_fixup_f32"] == 2 and tot["v_sqrt_f32"] == 2 and tot["valu"] == sum(r["valu"] for r in per.values())


def test_sites_name_their_block():
    body, (_, sites) = scanned()
    assert [(s["op"], s["phase"]) for s in sites] == [("v_sqrt_f32", "PROLOGUE"), ("v_div_fixup_f32", "BLOCK"), ("v_div_fixup_f32", "SHADE"),
                                                     ("v_sqrt_f32", "SHADE")]
    slow = sites[2]
    assert slow["block"] == ".LBB0_2" and slow["depth"] == 1 and slow["block_valu"] == 11   # nothing but the expansion: a slow path
    assert sites[0]["depth"] == 0 and sites[3]["block"] == ".LBB0_3"
    assert all(isa_divsqrt.opcode(body[s["line"]]) == s["op"] for s in sites)


def test_report_lists_phases_in_order_and_a_total():
    _, (per, sites) = scanned()
    text = isa_divsqrt.report(per, sites)
    names = [ln.split()[0] for ln in text[1:1 + len(per) + 1]]
    assert names == ["PROLOGUE", "SWAP", "SHADE", "BLOCK", "MARCH", "LATCH", "(whole)"]   # (LATCH: the loop's closing branch)
    assert sum("v_div_fixup_f32" in ln for ln in text) == 2 and sum("v_sqrt_f32" in ln for ln in text) == 2
    assert len(isa_divsqrt.report(per)) == len(per) + 2
