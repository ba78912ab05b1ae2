"""tools/isa_waits.py on canned assembly (no compiler, no GPU): which loads a wait waits for, which scalar waits expose a fresh load,
what a partial vmcnt(n) leaves outstanding, and the cut into phases by the kernel's `; chunky-mark phase-end` comments."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_copies  # noqa: E402
import isa_waits  # noqa: E402


def asm(text):
    return ["\t" + ln.strip() if not ln.strip().startswith((".", ";")) or ln.strip().startswith("; chunky") else ln.strip()
            for ln in text.strip().splitlines()]


def test_a_scalar_wait_with_and_without_a_fresh_load():
    body = asm("""
        s_load_dword s2, s[0:1], 0x620
        s_waitcnt lgkmcnt(0)
        v_mov_b32_e32 v0, s2
        s_waitcnt lgkmcnt(0)
        s_load_dwordx2 s[4:5], s[0:1], 0x610
        s_load_dwordx16 s[8:23], s[0:1], 0x150
        v_add_u32_e32 v1, v0, v0
        s_waitcnt lgkmcnt(0)
    """)
    w = isa_waits.scan(body)
    assert [x["line"] for x in w] == [1, 3, 7]
    assert [x["scalar_fresh"] for x in w] == [True, False, True]
    assert [t for _, t in w[0]["waits"]["lgkmcnt"][1]] == ["s_load_dword s2, s[0:1], 0x620"]
    assert w[1]["waits"]["lgkmcnt"] == (0, [], [])                        # nothing new since the last full wait
    assert [i for i, _ in w[2]["waits"]["lgkmcnt"][1]] == [4, 5]          # two loads, one round trip
    assert isa_waits.summary(w) == {"KERNEL": [3, 2, 0]}
    text = "\n".join(isa_waits.report(w))
    assert "nothing new" in text and "s_load_dwordx16 s[8:23], s[0:1], 0x150 @5" in text


def test_lds_traffic_alone_is_not_a_scalar_round_trip():
    body = asm("""
        ds_read_b64 v[0:1], v2
        s_waitcnt lgkmcnt(0)
        ds_bpermute_b32 v3, v4, v5
        s_load_dword s2, s[0:1], 0x0
        s_waitcnt lgkmcnt(0)
    """)
    w = isa_waits.scan(body)
    assert [x["scalar_fresh"] for x in w] == [False, True]
    assert len(w[1]["waits"]["lgkmcnt"][1]) == 2


def test_a_partial_lgkmcnt_retires_lds_traffic_only():
    body = asm("""
        ds_read_b64 v[0:1], v2
        s_load_dword s2, s[0:1], 0x0
        ds_read_b64 v[4:5], v2 offset:8
        ds_read_b64 v[6:7], v2 offset:16
        s_waitcnt lgkmcnt(1)
        s_waitcnt lgkmcnt(0)
    """)
    w = isa_waits.scan(body)
    assert [i for i, _ in w[0]["waits"]["lgkmcnt"][1]] == [0, 2] and [i for i, _ in w[0]["waits"]["lgkmcnt"][2]] == [1, 3]
    assert not w[0]["scalar_fresh"]                      # scalar loads return out of order: only lgkmcnt(0) waits for one
    assert [i for i, _ in w[1]["waits"]["lgkmcnt"][1]] == [1, 3] and w[1]["scalar_fresh"]


def test_a_partial_vmcnt_leaves_the_youngest_outstanding():
    body = asm("""
        global_load_dwordx3 v[0:2], v[10:11], off
        global_load_dwordx3 v[3:5], v[12:13], off
        global_load_dwordx3 v[6:8], v[14:15], off
        global_atomic_add v9, v1, v9, s[18:19] offset:256 sc0
        s_waitcnt vmcnt(3)
        s_waitcnt vmcnt(1)
        s_waitcnt vmcnt(4)
        s_waitcnt vmcnt(0) lgkmcnt(0)
        s_waitcnt vmcnt(0)
    """)
    w = isa_waits.scan(body)
    done = [[i for i, _ in x["waits"]["vmcnt"][1]] for x in w]
    left = [[i for i, _ in x["waits"]["vmcnt"][2]] for x in w]
    assert done == [[0], [1, 2], [], [3], []]
    assert left == [[1, 2, 3], [3], [3], [], []]
    assert w[3]["waits"]["lgkmcnt"] == (0, [], []) and not w[3]["scalar_fresh"]
    assert isa_waits.summary(w)["KERNEL"] == [5, 0, 3]


def test_only_the_named_prefixes_count():
    body = asm("""
        buffer_load_dword v0, v1, s[0:3], 0 offen
        flat_load_dword v2, v[4:5]
        global_store_dword v[4:5], v2, off
        v_mov_b32_e32 v0, v1
        s_waitcnt vmcnt(0) lgkmcnt(0)
    """)
    (w,) = isa_waits.scan(body)
    assert w["waits"] == {"vmcnt": (0, [], []), "lgkmcnt": (0, [], [])}
    assert [isa_waits.classify(x) for x in body] == [None, None, None, None, "wait"]


KERNEL = """
    s_load_dwordx2 s[2:3], s[0:1], 0x0
    s_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
    ds_wrxchg_rtn_b64 v[0:1], v2, v[0:1]
    s_waitcnt lgkmcnt(0)
    global_load_dword v3, v4, s[2:3]
    s_waitcnt vmcnt(0)
    ; chunky-mark phase-end march
    global_load_dwordx4 v[4:7], v[8:9], off
    global_load_dwordx4 v[10:13], v[8:9], off offset:16
    s_waitcnt vmcnt(1)
    s_waitcnt vmcnt(0)
    ; chunky-mark phase-end block
    ; chunky-mark phase-end model-blocks
    ; chunky-mark phase-end walk
    s_load_dword s4, s[0:1], 0x618
    s_waitcnt lgkmcnt(0)
    s_load_dword s5, s[0:1], 0x620
    s_waitcnt lgkmcnt(0)
    s_load_dwordx8 s[8:15], s[0:1], 0x5c0
    s_load_dwordx4 s[16:19], s[0:1], 0x5e0
    global_load_dword v14, v15, s[8:9]
    v_add_u32_e32 v16, v16, v16
    s_waitcnt lgkmcnt(0)
    s_waitcnt vmcnt(0)
    ; chunky-mark phase-end shade
    s_cbranch_scc1 .LBB0_1
    s_endpgm
"""


def test_the_phases_are_cut_by_the_kernels_marks():
    body = asm(KERNEL)
    header = next(i for i, ln in enumerate(body) if "Loop Header: Depth=1" in ln)
    phase_of = isa_copies.phase_function(body, margins={**isa_copies.MARGINS, "swap_after": 1}, header_line=header)
    w = isa_waits.scan(body, phase_of)
    assert [x["phase"] for x in w] == ["PROLOGUE", "SWAP", "MARCH", "BLOCK", "BLOCK", "SHADE", "SHADE", "SHADE", "SHADE"]
    per = isa_waits.summary(w)
    assert per["SHADE"] == [4, 3, 1]      # three scalar round trips in a row — the last one fetches two words at once — and the seed's
    assert per["BLOCK"] == [2, 0, 2] and per["MARCH"] == [1, 0, 1] and per["PROLOGUE"] == [1, 1, 0] and per["SWAP"] == [1, 0, 0]
    only = isa_waits.report(w, only="SHADE")
    assert len(only) == 4 and all(" SHADE " in ln for ln in only) and sum(" * " in ln for ln in only) == 3


@pytest.mark.parametrize("line,kind", [("\ts_load_dwordx16 s[36:51], s[54:55], 0x5c8", "lgkm"), ("\tds_bpermute_b32 v9, v8, v9", "lgkm"),
                                       ("\tglobal_load_dwordx3 v[8:10], v[8:9], off", "vm"), ("\tglobal_atomic_add v9, v1, v9, s[60:61] sc0", "vm"),
                                       ("\ts_waitcnt vmcnt(0)", "wait"), ("\ts_mov_b32 s0, s1", None), ("; s_load_ in a comment", None)])
def test_classify(line, kind):
    assert isa_waits.classify(line) == kind
