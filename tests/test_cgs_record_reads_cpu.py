"""The shapes of tests/cgs_record_reads_cases.py walk what they claim to (no
device: of_solver_geometry): every shape reaches k_cgs, and the walks of the
unflipped and of the flipped bands each cover every residue mod 8, so that
the register-carried records of waves 2 and 3 meet every position of the
8-step trip at loop entry's far end (the last, partial trip).
"""
import cgs_record_reads_cases as RR


def test_shapes_reach_k_cgs():
    for H, W in RR.SHAPES:
        assert H * W > RR.SMALL_PX and W % 2 == 0, (H, W)
    assert max(H * W for H, W in RR.SHAPES) < 14000  # the tests stay small


def test_walks_are_the_documented_ones():
    for H in range(1, 9):  # one unflipped band of H rows
        assert RR.walk_steps(H, RR.width_of(H)) == [(H + 20, False)], H
    for H, rows in [(9, 4), (10, 5), (12, 6), (14, 7), (16, 8)]:  # flipped second band
        w = RR.walk_steps(H, RR.width_of(H))
        assert len(w) == 2 and w[1] == (rows + 21, True), (H, w)
    for H, W in [(57, RR.width_of(57)), (58, RR.width_of(58)), (59, RR.width_of(59)), RR.SEAM_SHAPE]:
        w = RR.walk_steps(H, W)
        assert len(w) == 8 and w[:7] == [(28 + (i & 1), bool(i & 1)) for i in range(7)], (H, w)
        assert w[7] == (H - 56 + 21, True), (H, w)


def test_residues_are_complete():
    seen = {False: set(), True: set()}
    for H, W in RR.SHAPES:
        for steps, flipped in RR.walk_steps(H, W):
            seen[flipped].add(steps % 8)
    assert seen[False] == set(range(8)), seen
    assert seen[True] == set(range(8)), seen


def test_seam_and_single_strip():
    from optical_flow import _native
    strips = {(H, W): _native.solver_geometry(H, W, "backslash")["grid_x"] for H, W in RR.SHAPES}
    assert strips[(59, 70)] == 1 and strips[RR.SEAM_SHAPE] == 2, strips
    assert sum(1 for n in strips.values() if n > 1) >= 10, strips
