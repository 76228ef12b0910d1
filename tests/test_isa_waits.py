"""tools/isa_waits.py on a ten-line listing: a loop that issues two loads for
a later trip and waits for an earlier trip's data."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_waits  # noqa: E402

ASM = """
k_demo:                                 ; @k_demo
	buffer_load_dwordx4 v[0:3], v8, s[0:3], 0 offen
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	buffer_load_dwordx4 v[4:7], v8, s[0:3], 0 offen
	global_load_dword v9, v[10:11], off
	s_waitcnt vmcnt(2)
	v_add_f32_e32 v0, v0, v4
	buffer_store_dwordx4 v[0:3], v8, s[4:7], 0 offen
	s_waitcnt vmcnt(1) lgkmcnt(0)
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
k_other:
	s_waitcnt vmcnt(0)
"""


def test_loop_waits_counts_and_flags():
    body = isa_waits.kernel_body(ASM, "k_demo")
    assert body[-1] == "s_endpgm" and not any("k_other" in t for t in body)
    loops = isa_waits.loop_waits(body)
    assert len(loops) == 1
    lp = loops[0]
    assert lp["label"] == ".LBB0_1" and lp["vmem"] == 3   # the load before the label is outside the loop
    # vmcnt(2) after two loads of this trip leaves both in flight; vmcnt(1)
    # after the store as well waits for this trip's second load
    assert [(w["n"], w["issued"], w["short"]) for w in lp["waits"]] == [(2, 2, False), (1, 3, True)]
    txt = isa_waits.report("k_demo", loops)
    assert txt.count("<--") == 1 and "vmcnt(1)  issued 3" in txt


def test_step_at_restarts_the_count():
    body = ["k:", ".L1:", "buffer_load_dword v0, v1, s[0:3], 0 offen", "s_barrier",
            "buffer_load_dword v2, v1, s[0:3], 0 offen", "s_waitcnt vmcnt(1)", "s_cbranch_scc1 .L1"]
    assert [w["short"] for w in isa_waits.loop_waits(body)[0]["waits"]] == [True]
    lp = isa_waits.loop_waits(body, step_at="s_barrier")[0]
    assert [(w["n"], w["issued"], w["short"]) for w in lp["waits"]] == [(1, 1, False)] and lp["vmem"] == 2


def test_unknown_kernel():
    try:
        isa_waits.kernel_body(ASM, "k_missing")
    except ValueError as e:
        assert "k_missing" in str(e)
    else:
        raise AssertionError("expected ValueError")
