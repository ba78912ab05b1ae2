"""tools/isa_same.py says whether two assembly files hold the same kernels: these tests feed it canned snippets — the same two kernels in
the other order with their local labels renumbered and their comments changed must compare as the same, one changed instruction, a
changed descriptor or a missing kernel as different.  Nothing is compiled."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_same", os.path.join(ROOT, "tools", "isa_same.py"))
same = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(same)


def kernel(name, index, first_block, extra="", vgprs=12):
    return f"""\
	.section	.text.{name},"axG",@progbits,{name},comdat
	.globl	{name}
	.p2align	8
	.type	{name},@function
{name}: ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
	s_cbranch_scc1 .LBB{index}_{first_block + 1}
.LBB{index}_{first_block}:                                ; =>This Loop Header: Depth=1
	;;#ASMSTART
	; chunky-mark phase-end march
	;;#ASMEND
	v_add_u32_e32 v1, 1, v1 ; a comment behind an instruction
{extra}	s_cbranch_vccnz .LBB{index}_{first_block}
.LBB{index}_{first_block + 1}:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_next_free_vgpr {vgprs}
	.end_amdhsa_kernel
	.section	.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{index}:
	.size	{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
; NumVgprs: {vgprs}
""".splitlines()


A, B = "_ZN6chunky11render_poolILi17ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE", "_ZN6chunky4proj11render_poolILin1ELi64ELb0ELb0ELb0ELb0EEEvNS_8WaveArgsE"
BEFORE = kernel(A, 0, 1) + kernel(B, 1, 1, extra="\tv_mul_f32_e32 v2, v2, v3\n")


def test_kernels_are_cut_at_their_labels_and_stripped_of_comments():
    k = same.kernels(BEFORE)
    assert set(k) == {A, B}
    assert k[A][:3] == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "s_cbranch_scc1 .LBB_2"]
    assert "v_add_u32_e32 v1, 1, v1" in k[A] and not any("chunky-mark" in l or "ASMSTART" in l for l in k[A])
    assert ".amdhsa_next_free_vgpr 12" in k[A] and "v_mul_f32_e32 v2, v2, v3" in k[B] and "v_mul_f32_e32 v2, v2, v3" not in k[A]


def test_reordered_kernels_with_renumbered_labels_are_the_same():
    after = kernel(B, 0, 1, extra="\tv_mul_f32_e32 v2, v2, v3\n") + ["; another comment"] + kernel(A, 7, 1)
    assert same.compare(BEFORE, after) == []


def test_a_changed_instruction_is_a_difference():
    after = kernel(A, 0, 1) + kernel(B, 1, 1, extra="\tv_mul_f32_e32 v2, v2, v4\n")
    msgs = same.compare(BEFORE, after)
    assert len(msgs) == 1 and msgs[0].startswith(B) and "v_mul_f32_e32 v2, v2, v3" in msgs[0] and "v_mul_f32_e32 v2, v2, v4" in msgs[0]
    # a block numbered otherwise INSIDE its function is another flow, not a renumbered function
    assert same.compare(BEFORE, kernel(A, 0, 2) + kernel(B, 1, 1, extra="\tv_mul_f32_e32 v2, v2, v3\n")) != []
    # ... and so are more registers in the descriptor, and an instruction more
    assert same.compare(BEFORE, kernel(A, 0, 1, vgprs=16) + BEFORE[len(kernel(A, 0, 1)):]) != []
    assert same.compare(BEFORE, kernel(A, 0, 1, extra="\ts_nop 0\n") + BEFORE[len(kernel(A, 0, 1)):]) != []


def test_a_missing_or_an_added_kernel_is_a_difference():
    assert same.compare(BEFORE, kernel(A, 0, 1)) == [f"only before: {B}"]
    assert same.compare(kernel(A, 0, 1), BEFORE) == [f"only after: {B}"]
