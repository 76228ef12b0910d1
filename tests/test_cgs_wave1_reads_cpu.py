"""The shapes of tests/cgs_wave1_reads_cases.py walk what they claim to (no
device: of_solver_geometry): every shape is odd-width and reaches k_cgs, and
the walks of the unflipped and of the flipped bands each cover every residue
mod 8, so that the records and y rows wave 1 carries in registers meet every
position of the 8-step trip in the ODD instances.
"""
import cgs_wave1_reads_cases as WR


def test_shapes_are_the_listed_ones():
    assert WR.SHAPES == [(1, 4097), (2, 2049), (3, 1367), (4, 1025), (5, 821), (6, 683), (7, 587), (8, 513),
                         (9, 457), (10, 411), (12, 343), (14, 293), (16, 257), (57, 73), (58, 71), (59, 71),
                         (59, 231)]
    assert len(WR.cases()) == 103
    assert len({c["id"] for c in WR.cases()}) == 103


def test_shapes_reach_k_cgs_with_odd_width():
    for H, W in WR.SHAPES:
        assert H * W > WR.SMALL_PX and W % 2 == 1 and W >= 71, (H, W)
        if (H, W) != WR.SEAM_SHAPE:  # the smallest such width
            assert W == 71 or H * (W - 2) <= WR.SMALL_PX, (H, W)
    assert max(H * W for H, W in WR.SHAPES) == 13629 < 14000  # the tests stay small


def test_walks_are_the_documented_ones():
    for H in range(1, 9):  # one unflipped band of H rows
        assert WR.walk_steps(H, WR.width_of(H)) == [(H + 20, False)], H
    for H, rows in [(9, 4), (10, 5), (12, 6), (14, 7), (16, 8)]:  # flipped second band
        w = WR.walk_steps(H, WR.width_of(H))
        assert len(w) == 2 and w[1] == (rows + 21, True), (H, w)
    for H, W in [(57, WR.width_of(57)), (58, WR.width_of(58)), (59, WR.width_of(59)), WR.SEAM_SHAPE]:
        w = WR.walk_steps(H, W)
        assert len(w) == 8 and w[:7] == [(28 + (i & 1), bool(i & 1)) for i in range(7)], (H, w)
        assert w[7] == (H - 56 + 21, True), (H, w)


def test_residues_are_complete():
    seen = {False: set(), True: set()}
    for H, W in WR.SHAPES:
        for steps, flipped in WR.walk_steps(H, W):
            seen[flipped].add(steps % 8)
    assert seen[False] == set(range(8)), seen
    assert seen[True] == set(range(8)), seen


def test_seam_and_single_strip():
    from optical_flow import _native
    strips = {(H, W): _native.solver_geometry(H, W, "backslash")["grid_x"] for H, W in WR.SHAPES}
    assert strips[(59, 71)] == 1 and strips[WR.SEAM_SHAPE] == 2, strips
