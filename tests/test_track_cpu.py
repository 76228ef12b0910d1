"""Point tracker: what can be checked without a GPU -- the Python surface, the
argument checks, and the numpy restatement (tests/track_numpy.py) on
hand-made cases."""
import numpy as np
import pytest

import track_numpy as tn


def test_package_exports_tracking_api():
    import optical_flow
    from optical_flow import tracking
    for name in ("advance_points", "seed_points", "PointTracker", "track_points", "Trajectories"):
        assert getattr(optical_flow, name) is getattr(tracking, name)
        assert name in optical_flow.__all__
    assert (optical_flow.TRACK_ALIVE, optical_flow.TRACK_OCCLUDED, optical_flow.TRACK_LEFT_FRAME,
            optical_flow.TRACK_MOTION_BOUNDARY) == (0, 1, 2, 3)
    assert (tn.ALIVE, tn.OCCLUDED, tn.LEFT_FRAME, tn.MOTION_BOUNDARY) == (0, 1, 2, 3)
    for name in ("TRACK_ALIVE", "TRACK_OCCLUDED", "TRACK_LEFT_FRAME", "TRACK_MOTION_BOUNDARY"):
        assert name in optical_flow.__all__


def test_c_abi_mirror_declares_the_six_entries():
    import ctypes
    from optical_flow import _abi, _native
    want = {"of_track_advance": 11, "of_track_seed": 12, "of_tracks_open": 6, "of_tracks_push": 11,
            "of_tracks_read": 6, "of_tracks_close": 1}
    for name, n in want.items():
        assert len(_native._SIGS[name][0]) == n, name
    assert ctypes.sizeof(_abi.OfTrackOpts) == 48 and _abi.OfTrackOpts.alpha1.offset == 8
    assert _abi.OF_ABI_VERSION == 3


@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


Z = np.zeros((8, 9, 2))
PTS = np.array([[1.0, 2.0], [3.0, 4.0]])


@pytest.mark.parametrize("kw", [
    dict(xy=None), dict(xy=np.zeros((2, 3))), dict(xy=np.zeros(4)), dict(xy=np.zeros((2, 2), dtype=complex)),
    dict(fw=np.zeros((8, 9))), dict(fw=np.zeros((8, 9, 3))), dict(bw=np.zeros((8, 10, 2))), dict(fw=np.zeros((0, 9, 2)),
                                                                                               bw=np.zeros((0, 9, 2))),
    dict(status=np.zeros(3, np.uint8)), dict(status=np.zeros(2)), dict(status=np.array([0, 256])),
    dict(status=np.array([0, -1])), dict(alpha1=-1.0), dict(alpha2=float("nan")), dict(beta1=float("inf")),
    dict(beta2=-0.1), dict(alpha1="x"), dict(beta1=None)])
def test_advance_points_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(xy=PTS, fw=Z, bw=Z)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.advance_points(**a)


@pytest.mark.parametrize("kw", [
    dict(gray=np.zeros((8, 9, 3))), dict(gray=np.zeros(8)), dict(gray=np.zeros((0, 9))),
    dict(gray=np.zeros((8, 9), dtype=complex)), dict(step=0), dict(step=65), dict(step=2.0), dict(step=True),
    dict(max_tracks=0), dict(max_tracks=(1 << 24) + 1), dict(max_tracks=1.5), dict(min_eig=-1.0),
    dict(min_eig=float("nan")), dict(min_eig=float("inf")), dict(frame=-1), dict(frame=0.5),
    dict(xy=np.zeros((2, 3))), dict(status=np.zeros(2, np.uint8)), dict(xy=PTS, status=np.zeros(3, np.uint8)),
    dict(xy=PTS, max_tracks=1)])
def test_seed_points_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(gray=np.zeros((8, 9)))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.seed_points(**a)


@pytest.mark.parametrize("kw", [
    dict(shape=(8,)), dict(shape=(8, 9, 2)), dict(shape=(8, 9, 3, 1)), dict(shape=(0, 9)), dict(shape=(8, 9, 1)),
    dict(method="nonexistent_method"), dict(step=0), dict(step=65), dict(max_tracks=0), dict(max_tracks=1 << 25),
    dict(min_eig=-1.0), dict(min_eig=float("nan")), dict(alpha1=-0.5), dict(alpha2=float("inf")), dict(beta1=-1.0),
    dict(beta2=float("nan"))])
def test_point_tracker_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(shape=(8, 9))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.PointTracker(**a)
    if "shape" not in kw:
        with pytest.raises(ValueError):
            optical_flow.track_points([np.zeros((8, 9))], **kw)


def test_track_points_bad_frames_raise_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.track_points([])
    with pytest.raises(ValueError):
        optical_flow.track_points([np.zeros((8, 9)), np.zeros((8, 10))])
    with pytest.raises(ValueError):
        optical_flow.track_points([np.zeros((8, 9, 2))])


def test_default_max_tracks_is_four_times_the_cells():
    from optical_flow.tracking import _track_opts
    assert _track_opts(37, 53, 8).max_tracks == 4 * 5 * 7
    assert _track_opts(37, 53, 1).max_tracks == 4 * 37 * 53
    assert _track_opts(8192, 8192, 1).max_tracks == 1 << 24
    o = _track_opts(37, 53)
    assert (o.step, o.alpha1, o.alpha2, o.beta1, o.beta2, o.min_eig) == (8, 0.01, 0.5, 0.01, 0.002, 25.0)


# ---- the restatement on hand-made cases ------------------------------------
def grid_points(H, W, m):
    ys, xs = np.mgrid[m:H - m, m:W - m]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def test_constant_integer_flow_moves_every_point_exactly():
    H, W = 20, 30
    fw = np.zeros((H, W, 2))
    fw[..., 0], fw[..., 1] = 3.0, -2.0
    pts = grid_points(H, W, 4) + np.float32(0.25)
    xy, st = tn.advance(pts, np.zeros(len(pts), np.uint8), fw, -fw)
    assert np.all(st == tn.ALIVE)
    np.testing.assert_array_equal(xy, pts + np.array([3.0, -2.0], np.float32))


def test_disagreeing_backward_flow_ends_tracks_occluded():
    H, W = 20, 30
    fw = np.zeros((H, W, 2))
    fw[..., 0] = 2.0
    bw = -fw.copy()
    bw[:, 15:, 0] += 1.0  # |fw + bw|^2 = 1 > 0.01 * (4 + 1) + 0.5 right of column 15
    pts = grid_points(H, W, 4)
    xy, st = tn.advance(pts, np.zeros(len(pts), np.uint8), fw, bw)
    hit = pts[:, 0] + 2.0 >= 15
    assert np.all(st[hit] == tn.OCCLUDED) and np.all(st[~hit] == tn.ALIVE)
    np.testing.assert_array_equal(xy[hit], pts[hit])  # an ended track keeps its position
    np.testing.assert_array_equal(xy[~hit], pts[~hit] + np.array([2.0, 0.0], np.float32))


def test_step_edge_in_the_flow_ends_tracks_at_the_motion_boundary():
    H, W = 20, 30
    fw = np.zeros((H, W, 2))
    fw[:, 15:, 0] = 1.0  # a step of 1 px between columns 14 and 15
    pts = grid_points(H, W, 4)
    xy, st = tn.advance(pts, np.zeros(len(pts), np.uint8), fw, -fw)
    edge = (pts[:, 0] == 14) | (pts[:, 0] == 15)  # g = 0.25 > 0.01 * |w|^2 + 0.002 there
    assert np.all(st[edge] == tn.MOTION_BOUNDARY) and np.all(st[~edge] == tn.ALIVE)
    np.testing.assert_array_equal(xy[edge], pts[edge])


def test_flow_out_of_the_frame_and_bad_positions_give_left_frame():
    H, W = 20, 30
    fw = np.zeros((H, W, 2))
    fw[..., 0] = 5.0
    pts = np.array([[26.0, 5.0], [24.0, 5.0], [np.nan, 3.0], [3.0, np.inf], [-0.5, 2.0], [29.0, 19.0]], np.float32)
    xy, st = tn.advance(pts, np.zeros(len(pts), np.uint8), fw, -fw)
    assert list(st) == [tn.LEFT_FRAME, tn.ALIVE, tn.LEFT_FRAME, tn.LEFT_FRAME, tn.LEFT_FRAME, tn.LEFT_FRAME]
    assert xy[1, 0] == 29.0 and np.array_equal(xy[0], pts[0])
    nanflow = fw.copy()
    nanflow[5, 10] = np.nan
    _, st = tn.advance(np.array([[10.0, 5.0]], np.float32), np.zeros(1, np.uint8), nanflow, -fw)
    assert st[0] == tn.LEFT_FRAME


def test_dead_tracks_are_left_alone():
    fw = np.ones((10, 12, 2))
    pts = np.array([[2.0, 2.0], [3.0, 3.0], [4.0, 4.0], [5.0, 5.0]], np.float32)
    st0 = np.array([1, 2, 3, 0], np.uint8)
    xy, st = tn.advance(pts, st0, fw, -fw)
    np.testing.assert_array_equal(st, st0)
    np.testing.assert_array_equal(xy[:3], pts[:3])
    np.testing.assert_array_equal(xy[3], [6.0, 6.0])


def test_seed_ids_are_row_major_and_edge_cells_have_no_candidate():
    # 10 x 13, step 4: cells 3 x 4, candidates at rows 2, 6, (10: outside), columns 2, 6, 10, (14: outside)
    new, dropped = tn.seed(np.zeros((10, 13)), None, None, 4, 100, 0.0)
    assert dropped == 0
    np.testing.assert_array_equal(new, [[2, 2], [6, 2], [10, 2], [2, 6], [6, 6], [10, 6]])


def test_seed_capacity_and_dropped_count():
    new, dropped = tn.seed(np.zeros((10, 13)), None, None, 4, 4, 0.0)
    assert dropped == 2
    np.testing.assert_array_equal(new, [[2, 2], [6, 2], [10, 2], [2, 6]])
    table = np.array([[0.0, 9.0], [12.0, 9.0]], np.float32)  # both in candidate-less cells of the last row
    new, dropped = tn.seed(np.zeros((10, 13)), table, np.zeros(2, np.uint8), 4, 5, 0.0)
    assert len(new) == 3 and dropped == 3


def test_seed_skips_occupied_cells_but_not_those_of_dead_tracks():
    table = np.array([[5.4, 1.6], [9.0, 5.0], [7.5, 3.4]], np.float32)  # cells (0, 1), (1, 2), near -> (8, 3): (0, 2)
    status = np.array([0, 1, 0], np.uint8)
    new, dropped = tn.seed(np.zeros((10, 13)), table, status, 4, 100, 0.0)
    np.testing.assert_array_equal(new, [[2, 2], [2, 6], [6, 6], [10, 6]])
    assert dropped == 0


def test_seed_eigenvalue_test():
    H, W = 12, 12
    g = np.zeros((H, W))
    g[:, 6:] = 100.0  # a vertical edge only: lambda_min = 0
    assert not tn.seed_flags(g, None, None, 4, 1.0).any()
    assert tn.seed_flags(g, None, None, 4, 0.0).all()
    c = g.copy()
    c[6:, :] += 100.0  # a corner at (6, 6): the candidate (6, 6) of cell (1, 1) has both gradients
    f = tn.seed_flags(c, None, None, 4, 25.0)
    assert f[1, 1] and f.sum() == 1


def test_trajectories_assembly_from_snapshots():
    from optical_flow.tracking import Trajectories
    nan = np.nan
    s0 = (np.array([[1, 1], [5, 5]], np.float32), np.array([0, 0], np.uint8), np.array([0, 0], np.int32))
    s1 = (np.array([[2, 1], [5, 5], [9, 9]], np.float32), np.array([0, 1, 0], np.uint8),
          np.array([0, 0, 1], np.int32))
    s2 = (np.array([[3, 1], [5, 5], [9, 9], [4, 4]], np.float32), np.array([0, 1, 2, 0], np.uint8),
          np.array([0, 0, 1, 2], np.int32))
    want = np.array([[[1, 1], [5, 5], [nan, nan], [nan, nan]],
                     [[2, 1], [nan, nan], [9, 9], [nan, nan]],
                     [[3, 1], [nan, nan], [nan, nan], [4, 4]]], np.float32)
    xy, start, length, status = tn.assemble([s0, s1, s2])
    np.testing.assert_array_equal(xy, want)
    assert list(start) == [0, 0, 1, 2] and list(length) == [3, 1, 1, 1] and list(status) == [0, 1, 2, 0]
    tr = Trajectories.from_snapshots([s0, s1, s2])
    assert len(tr) == 4 and tr.xy.dtype == np.float32 and tr.xy.shape == (3, 4, 2)
    np.testing.assert_array_equal(tr.xy, want)
    np.testing.assert_array_equal(tr.start, start)
    np.testing.assert_array_equal(tr.length, length)
    np.testing.assert_array_equal(tr.status, status)
    assert len(Trajectories.from_snapshots([])) == 0
