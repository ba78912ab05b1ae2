"""tools/isa_copies.py reads a compiled kernel's assembly: these tests feed its parser two canned snippets — a loop header, two phases and
a latch, once in the layout of an if / else-if chain (no marks: cut by landmarks, the latch found in the flow graph) and once as
consecutive ifs with the `; chunky-mark phase-end` comments in a rotated loop — and check what it attributes to whom.  Nothing is compiled."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_copies", os.path.join(ROOT, "tools", "isa_copies.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)

TIGHT = {"swap_before": 0, "swap_after": 0, "models": 0, "shade_after": 0, "march_before": 5}
STATS = {"loop": {"iterations_per_64_samples": 10.0, "march_entries_per_64_samples": 6.0}, "block": {"execs_per_sample": 1.0},
         "shade": {"execs_per_sample": 3.0}, "model": {"execs_per_sample": 0.0}, "swaps": {"rounds_per_sample": 8.0}}

CHAIN = """\
_ZN6chunky11render_poolILi17ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE: ; @kernel
; %bb.0:
	s_getreg_b32 s3, hwreg(HW_REG_XCC_ID)
	v_mov_b32_e32 v1, 0
	s_branch .LBB0_2
.LBB0_1:                                ; %census
                                        ;   in Loop: Header=BB0_2 Depth=1
	v_cmp_eq_u32_e32 vcc, 0, v9
	s_cbranch_scc0 .LBB0_9
.LBB0_2:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_7 Depth 2
	ds_wrxchg_rtn_b64 v[2:3], v8, v[2:3]
	s_cbranch_scc1 .LBB0_6
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v10, v2
	v_mov_b32_e32 v11, v3
	v_mov_b32_e32 v12, 0x7fc00000
	v_cndmask_b32_e64 v10, v10, v4, s[2:3]
	global_store_dwordx3 v[14:15], v[10:12], off nt
	s_cbranch_execz .LBB0_5
; %bb.4:                                ;   in Loop: Header=BB0_2 Depth=1
	v_add_f32_e32 v10, v10, v11
.LBB0_5:                                ; %Flow
                                        ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v2, v10
	v_mov_b32_e32 v3, v11
	v_mov_b32_e32 v4, s5
	s_branch .LBB0_1
.LBB0_6:                                ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v20, v5
.LBB0_7:                                ;   Parent Loop BB0_2 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
	;;#ASMSTART
	v_cvt_flr_i32_f32 v6, v5
	;;#ASMEND
	v_cndmask_b32_e64 v5, v5, v6, s[6:7]
	s_cbranch_scc1 .LBB0_7
; %bb.8:                                ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v5, v20
	s_branch .LBB0_1
.LBB0_9:                                ; %._crit_edge
	s_endpgm
""".splitlines()

MARKED = """\
_ZN6chunky11render_poolILi17ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE: ; @kernel
; %bb.0:
	s_getreg_b32 s3, hwreg(HW_REG_XCC_ID)
	s_branch .LBB0_2
.LBB0_1:                                ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v7, v8
	;;#ASMSTART
	; chunky-mark phase-end shade
	;;#ASMEND
.LBB0_10:                               ; %census
                                        ;   in Loop: Header=BB0_2 Depth=1
	v_cmp_eq_u32_e32 vcc, 0, v9
	s_cbranch_scc0 .LBB0_9
.LBB0_2:                                ; =>This Loop Header: Depth=1
	ds_wrxchg_rtn_b64 v[2:3], v8, v[2:3]
	s_cbranch_scc1 .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=1
	;;#ASMSTART
	v_cvt_flr_i32_f32 v6, v5
	;;#ASMEND
	v_mov_b32_e32 v5, v6
.LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=1
	;;#ASMSTART
	; chunky-mark phase-end march
	;;#ASMEND
	s_cbranch_scc1 .LBB0_6
; %bb.5:                                ;   in Loop: Header=BB0_2 Depth=1
	v_mov_b32_e32 v10, v2
	v_cndmask_b32_e64 v10, v10, v4, s[2:3]
.LBB0_6:                                ;   in Loop: Header=BB0_2 Depth=1
	;;#ASMSTART
	; chunky-mark phase-end block
	;;#ASMEND
	;;#ASMSTART
	; chunky-mark phase-end model-blocks
	;;#ASMEND
	;;#ASMSTART
	; chunky-mark phase-end walk
	;;#ASMEND
	s_cbranch_scc1 .LBB0_1
; %bb.7:                                ;   in Loop: Header=BB0_2 Depth=1
	global_store_dwordx3 v[14:15], v[10:12], off nt
	v_mov_b32_e32 v2, v10
	v_mov_b32_e32 v3, v11
	s_branch .LBB0_1
.LBB0_9:                                ; %._crit_edge
	s_endpgm
""".splitlines()


def copies(r, phase):
    return r["per_phase"][phase]["copies"], r["per_phase"][phase]["cndmask"]


def test_what_counts_as_a_copy():
    assert ic.is_copy("\tv_mov_b32_e32 v2, v10")
    assert ic.is_copy("\tv_mov_b32_e32 v2, v10 ; a comment")
    for other in ("\tv_mov_b32_e32 v2, 0", "\tv_mov_b32_e32 v2, 0x7fc00000", "\tv_mov_b32_e32 v4, s5", "\tv_mov_b32_e32 v4, 1.0",
                  "\tv_cndmask_b32_e64 v5, v5, v6, s[6:7]", "\tv_mov_b32_dpp v2, v3 quad_perm:[1,0,3,2]", "\ts_mov_b32 s2, s3"):
        assert not ic.is_copy(other), other
    assert ic.is_cndmask("\tv_cndmask_b32_e64 v5, v5, v6, s[6:7]") and not ic.is_cndmask("\tv_mov_b32_e32 v2, v10")


def test_blocks_and_loops():
    blocks = {b.label: b for b in ic.parse(CHAIN)}
    assert blocks[".LBB0_2"].is_header and blocks[".LBB0_2"].depth == 1
    assert blocks[".LBB0_7"].is_header and blocks[".LBB0_7"].depth == 2
    assert blocks["bb.3"].depth == 1 and blocks["bb.3"].header == ".LBB0_2"
    assert blocks["bb.0"].depth == 0 and blocks[".LBB0_9"].depth == 0
    assert blocks[".LBB0_5"].targets == [".LBB0_1"] and not blocks[".LBB0_5"].falls
    assert blocks[".LBB0_1"].targets == [".LBB0_9"] and blocks[".LBB0_1"].falls
    assert len(blocks["bb.3"].lines) == 6   # comments and directives are no instructions


def test_if_chain_layout():
    r = ic.attribute(CHAIN, TIGHT)
    assert r["main"].label == ".LBB0_2" and not r["marked"]
    # the census and the join behind SHADE lead nowhere but to the loop's head; the march's straight-line exit is the march's
    assert [b.label for b in r["latch"]] == [".LBB0_1", ".LBB0_5"]
    assert r["latch_phases"][".LBB0_5"] == {"SHADE"} and r["latch_phases"][".LBB0_1"] == {"SHADE", "MARCH"}
    assert copies(r, "LATCH") == (2, 0)      # (the move from a scalar register is no copy)
    assert copies(r, "SHADE") == (2, 1)      # (nor is the literal)
    assert copies(r, "MARCH") == (2, 1)
    assert copies(r, "PROLOGUE") == (0, 0) and copies(r, "SWAP") == (0, 0) and copies(r, "BLOCK") == (0, 0)
    assert r["entry"]["SHADE"].label == "bb.3" and r["exit_copies"]["SHADE"] == 0
    assert r["entry"]["MARCH"].label == ".LBB0_6" and r["exit_copies"]["MARCH"] == 1 and r["inner_copies"]["MARCH"] == 0
    rows, total = ic.weighted_estimate(r, STATS)
    # a latch block counts for the executions of the phases that reach it: 2 x 3 (SHADE); + the phases' own blocks, 2 x 3 + 2 x 6
    assert dict((n, (c, w)) for n, c, w in rows)["latch .LBB0_5"] == (2, 3.0)
    assert total == 24.0


def test_marked_layout_in_a_rotated_loop():
    r = ic.attribute(MARKED, TIGHT)
    assert r["main"].label == ".LBB0_2" and r["marked"]
    assert [(p, n) for n, p in ic.phase_ends(MARKED)] == [("SHADE", 7), ("MARCH", 23), ("BLOCK", 31), ("MODELS", 34), ("WALK", 37)]
    # what stands ahead of the shade mark, and what follows the last mark further down, is SHADE; the census between the mark and the head is the latch
    assert [b.label for b in r["latch"]] == [".LBB0_10"] and r["latch_phases"][".LBB0_10"] is None
    assert copies(r, "SHADE") == (3, 0)
    assert copies(r, "MARCH") == (1, 0)
    assert copies(r, "BLOCK") == (1, 1)
    assert copies(r, "LATCH") == (0, 0) and copies(r, "MODELS") == (0, 0)
    rows, total = ic.weighted_estimate(r, STATS)
    assert total == 1 * 6.0 + 1 * 1.0 + 3 * 3.0


def test_cut_kernel_prefers_the_pinhole_kernel():
    text = ["_ZN6chunky4proj11render_poolILi17ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE: ; @a", "\ts_endpgm", "\t.end_amdhsa_kernel",
            "; NumVgprs: 96", "; ScratchSize: 8", "; Occupancy: 5",
            "_ZN6chunky11render_poolILi17ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE: ; @b", "\ts_endpgm", "\t.end_amdhsa_kernel",
            "; NumVgprs: 80", "; ScratchSize: 16", "; Occupancy: 6"]
    name, body, meta = ic.cut_kernel(text, "render_poolILi17ELi64ELb0ELb0ELb0ELb0EE")
    assert name.startswith("_ZN6chunky11render_pool") and meta == {"; NumVgprs:": "80", "; ScratchSize:": "16", "; Occupancy:": "6"}
    name, _body, meta = ic.cut_kernel(text, "4proj11render_poolILi17ELi64ELb0ELb0ELb0ELb0EE")
    assert "4proj" in name and meta["; NumVgprs:"] == "96"
