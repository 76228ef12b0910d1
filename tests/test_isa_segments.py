"""tools/isa_segments.py on a short synthetic listing: the split at an opcode,
the instruction classes, the watched opcodes and the grouping by (VMEM, LDS
writes) key."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_segments as S  # noqa: E402
from isa_waits import kernel_body  # noqa: E402

LISTING = """
	.globl	other
other:
	s_endpgm
.Lfunc_end0:
k_demo:                                 ; @k_demo
; %bb.0:
	s_load_dwordx4 s[0:3], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	s_mul_i32 s6, s0, s1            ; preamble
	s_barrier
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
	s_mul_hi_i32 s7, s6, 0x92492493
	s_cselect_b32 s8, s7, 2.0
	v_add_u32_e32 v1, s8, v0
	buffer_load_dwordx4 v[4:7], v1, s[0:3], 0 offen
	buffer_load_dwordx2 v[8:9], v1, s[0:3], s9 offen
	v_rcp_f32_e32 v2, v4
	v_cndmask_b32_e32 v3, 0, v2, vcc
	v_mov_b32_e32 v10, v3
	ds_write_b128 v11, v[4:7]
	ds_read_b64 v[12:13], v11
	s_waitcnt vmcnt(0) lgkmcnt(0)
	buffer_store_dwordx4 v[4:7], v1, s[0:3], 0 offen
	s_cbranch_scc1 .LBB1_3
; %bb.2:
	v_pk_fma_f32 v[4:5], v[4:5], v[6:7], v[8:9]
.LBB1_3:
	s_barrier
	v_pk_mul_f32 v[4:5], v[4:5], v[6:7]
	v_mov_b32_dpp v6, v5 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1
	ds_write_b64 v11, v[4:5]
	s_add_i32 s6, s6, 1
	s_cmp_lt_i32 s6, s10
	s_barrier
	s_cbranch_scc1 .LBB1_1
	s_endpgm
.Lfunc_end1:
"""


def _segs():
    return S.segments(kernel_body(LISTING, "k_demo"), "s_barrier")


def test_opcode_skips_labels_directives_comments():
    assert S.opcode(".LBB1_3:") is None
    assert S.opcode("; %bb.2:") is None
    assert S.opcode("\t.globl\tother") is None
    assert S.opcode("\ts_mul_i32 s6, s0, s1            ; preamble") == "s_mul_i32"


def test_split_and_classes():
    segs = _segs()
    assert len(segs) == 4  # preamble, two steps, the tail after the last barrier
    pre, a, b, tail = segs
    assert pre["instr"] == 4 and pre["smem"] == 1 and pre["wait"] == 2 and pre["salu"] == 1 and pre["s_mul_i32"] == 1
    assert a["instr"] == 15
    assert a["vmem"] == 3 and a["lds"] == 2 and a["lds_write"] == 1 and a["branch"] == 1
    assert a["valu"] == 5 and a["salu"] == 2 and a["wait"] == 2  # the closing s_barrier counts in its segment
    assert a["s_mul_hi"] == 1 and a["s_cselect"] == 1 and a["v_rcp_f32"] == 1 and a["v_cndmask"] == 1
    assert a["v_mov_b32"] == 1
    assert b["instr"] == 6 and b["valu"] == 2 and b["v_mov_b32"] == 1 and b["lds_write"] == 1 and b["vmem"] == 0
    assert tail["instr"] == 2 and tail["branch"] == 1
    assert S.key_of(a) == (3, 1) and S.key_of(b) == (0, 1)


def test_group_and_table():
    segs = _segs()
    g = S.group(segs * 3, min_members=3)
    assert set(g) == {(3, 1), (0, 1), (0, 0)}  # preamble and tail share the key (0, 0)
    assert g[(3, 1)]["segments"] == 3 and g[(3, 1)]["instr"] == (15, 15, 15)
    assert g[(0, 0)]["instr"] == (2, 4, 2)  # min, max, (low) median
    g = S.group(segs, min_members=2)
    assert set(g) == {(0, 0), "other"} and g["other"]["segments"] == 2 and g["other"]["instr"] == (6, 15, 6)
    txt = S.table([("x", g["other"]), ("y", segs[1])])
    lines = txt.splitlines()
    assert lines[0].startswith("| segment | instr | valu |") and len(lines) == 4
    assert lines[2].startswith("| x | 6-15 (6) |") and lines[3].startswith("| y | 15 | 5 | 2 | 1 | 2 | 3 | 2 |")
