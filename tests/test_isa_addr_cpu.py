"""tools/isa_addr.py on canned assembly (no compiler, no GPU): integer multiplies attributed to their use (an address, the division by
an invariant, the PCG step), the pieces of a 64-bit address (v_lshl_add_u64, a sign extension that only feeds one, a carry pair), every
global load and store with its form, per phase as the kernel's `; chunky-mark phase-end` comments cut it."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_addr  # noqa: E402
import isa_copies  # noqa: E402


def asm(text):
    return ["\t" + ln.strip() if not ln.strip().startswith((".", ";")) or ln.strip().startswith("; chunky") else ln.strip()
            for ln in text.strip().splitlines()]


# one texel address as a size_t product off a per-lane pointer: the nine instructions, then the load
TEXEL64 = """
    v_ashrrev_i32_e32 v19, 31, v18
    v_mad_i64_i32 v[12:13], s[8:9], v17, s92, v[18:19]
    v_mul_lo_u32 v0, v13, s94
    v_mul_lo_u32 v14, v12, s93
    v_mad_u64_u32 v[12:13], s[8:9], v12, s94, 0
    v_add3_u32 v13, v13, v14, v0
    v_ashrrev_i32_e32 v17, 31, v16
    v_lshl_add_u64 v[12:13], v[12:13], 2, s[36:37]
    v_lshl_add_u64 v[22:23], v[16:17], 2, v[12:13]
    global_load_dword v17, v[22:23], off
"""
# the same texel as a 32-bit offset off a scalar base
TEXEL32 = """
    v_mad_u32_u24 v12, v17, s92, v18
    v_mad_u32_u24 v12, v12, s94, v16
    v_lshlrev_b32_e32 v12, 2, v12
    global_load_dword v17, v12, s[36:37]
"""

KERNEL = """
    s_load_dwordx2 s[2:3], s[0:1], 0x0
.LBB0_1:                                ; =>This Loop Header: Depth=1
    ds_wrxchg_rtn_b64 v[0:1], v2, v[0:1]
    s_waitcnt lgkmcnt(0)
    v_cvt_flr_i32_f32_e32 v3, v4
    global_load_dword v5, v6, s[4:5] offset:16
    ; chunky-mark phase-end march
""" + TEXEL64 + """
    v_ashrrev_i32_e32 v30, 31, v29
    v_xor_b32_e32 v31, v30, v29
    ; chunky-mark phase-end block
    ; chunky-mark phase-end model-blocks
    ; chunky-mark phase-end walk
""" + TEXEL32 + """
    v_mul_lo_u32 v40, v40, s20
    v_lshrrev_b32_e32 v41, 22, v40
    v_xor_b32_e32 v40, v41, v40
    v_mul_hi_u32 v50, v51, s21
    v_lshrrev_b32_e32 v50, 3, v50
    v_mul_lo_u32 v52, v50, s22
    v_sub_u32_e32 v52, v51, v52
    v_add_co_u32_e32 v60, vcc, s6, v61
    v_addc_co_u32_e32 v61, vcc, 0, v62, vcc
    global_store_dword v[60:61], v2, off nt
    ; chunky-mark phase-end shade
    s_cbranch_scc1 .LBB0_1
    s_endpgm
"""


def scanned():
    body = asm(KERNEL)
    header = next(i for i, ln in enumerate(body) if "Loop Header: Depth=1" in ln)
    phase_of = isa_copies.phase_function(body, margins={**isa_copies.MARGINS, "swap_after": 1}, header_line=header)
    return body, isa_addr.scan(body, phase_of)


def test_operands_and_forms():
    assert isa_addr.vregs("v[4:6]") == {4, 5, 6} and isa_addr.vregs("v3") == {3} and isa_addr.vregs("s[4:5]") == set()
    assert isa_addr.mem_form("\tglobal_load_dword v17, v[22:23], off") == "vaddr64"
    assert isa_addr.mem_form("\tglobal_load_dwordx4 v[0:3], v12, s[36:37] offset:32") == "saddr"
    assert isa_addr.mem_form("\tglobal_store_dword v[60:61], v2, off nt") == "vaddr64"
    assert isa_addr.mem_address("\tglobal_store_dword v[60:61], v2, off nt") == {60, 61}
    assert isa_addr.mem_address("\tglobal_load_dword v17, v12, s[36:37]") == {12}
    assert isa_addr.is_sext("\tv_ashrrev_i32_e32 v19, 31, v18") and not isa_addr.is_sext("\tv_ashrrev_i32_e32 v19, 3, v18")


def test_the_64_bit_texel_is_all_address():
    _, (per, _) = scanned()
    b = per["BLOCK"]
    assert (b["v_mul_lo_u32"], b["v_mad_u64_u32"], b["v_mad_i64_i32"], b["v_mul_hi_u32"]) == (2, 1, 1, 0)
    assert (b["mul_address"], b["mul_fast_quotient"], b["mul_other"]) == (4, 0, 0)
    assert b["v_lshl_add_u64"] == 2
    assert b["sext_for_address"] == 2          # the third sign extension feeds an xor: no address
    assert (b["mem_saddr"], b["mem_vaddr64"]) == (0, 1)
    assert isa_addr.address_instructions(b) == 4 + 2 + 2


def test_the_32_bit_texel_and_the_other_multiplies():
    _, (per, _) = scanned()
    s = per["SHADE"]
    assert (s["v_mul_lo_u32"], s["v_mul_hi_u32"], s["v_mad_u64_u32"], s["v_mad_i64_i32"]) == (2, 1, 0, 0)
    assert (s["mul_address"], s["mul_fast_quotient"], s["mul_other"]) == (0, 2, 1)   # quotient: the mul_hi and the remainder's mul_lo; other: PCG
    assert s["v_lshl_add_u64"] == 0 and s["sext_for_address"] == 0 and s["add_co_pairs"] == 1
    assert (s["mem_saddr"], s["mem_vaddr64"]) == (1, 1)                               # the texel by saddr, the store by a pair
    m = per["MARCH"]
    assert (m["mem_saddr"], m["mem_vaddr64"], m["mul_address"]) == (1, 0, 0)


def test_sites_and_report():
    body, (per, sites) = scanned()
    uses = [(s["op"], s["use"], s["phase"]) for s in sites if s["op"] in isa_addr.MULS]
    assert uses[:4] == [("v_mad_i64_i32", "address", "BLOCK"), ("v_mul_lo_u32", "address", "BLOCK"), ("v_mul_lo_u32", "address", "BLOCK"),
                        ("v_mad_u64_u32", "address", "BLOCK")]
    assert uses[4:] == [("v_mul_lo_u32", "pcg/other", "SHADE"), ("v_mul_hi_u32", "fast_quotient", "SHADE"), ("v_mul_lo_u32", "fast_quotient", "SHADE")]
    assert all(isa_addr.opcode(body[s["line"]]) == s["op"] for s in sites)
    tot = isa_addr.summary(per)
    assert tot["mem_saddr"] == 2 and tot["mem_vaddr64"] == 2 and tot["valu"] == sum(r["valu"] for r in per.values())
    text = isa_addr.report(per, sites)
    assert [ln.split()[0] for ln in text[1:1 + len(per) + 1]][-1] == "(whole)"
    assert len(isa_addr.report(per)) == len(per) + 2
