"""The point tracker on the GPU: of_track_advance and of_track_seed bitwise
against the numpy float64 restatement (tests/track_numpy.py), the session
(of_tracks_*) bitwise against its parts run by hand, its lifecycle, and an
end-to-end check that it tracks an exactly known motion."""
import ctypes as C

import numpy as np
import pytest

import track_numpy as tn

pytestmark = pytest.mark.gpu

H0, W0 = 37, 53


# ---- of_track_advance -------------------------------------------------------
@pytest.fixture(scope="module")
def advance_case():
    """37 x 53 smooth flows with rows and columns of NaN / Inf, 1000 points
    (on the borders, random, a few outside or not finite) with mixed statuses,
    and the restatement's answer, computed once."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H0, 0:W0].astype(np.float64)
    fw = np.stack([2.5 * np.sin(0.11 * xx + 0.07 * yy) + 0.8, 1.8 * np.cos(0.09 * xx - 0.13 * yy)], -1)
    fw[:, 30:, 0] += 1.2                      # a motion boundary
    bw = -fw + rng.normal(0, 0.35, fw.shape)  # disagrees here and there
    fw, bw = fw.astype(np.float32), bw.astype(np.float32)
    fw[5, :, 0] = np.nan
    fw[:, 44, 1] = np.inf
    fw[20, :, :] = -np.inf
    bw[9, :, 1] = np.nan
    bw[:, 12, 0] = np.inf
    bw[:, 3, :] = np.nan
    border = [(0, 0), (W0 - 1, 0), (0, H0 - 1), (W0 - 1, H0 - 1)]
    border += [(0, y) for y in (3.5, 17, 30.25)] + [(W0 - 1, y) for y in (2, 18.75, 33)]
    border += [(x, 0) for x in (7.5, 25, 48)] + [(x, H0 - 1) for x in (4, 26.5, 50)]
    odd = [(np.nan, 4), (6, np.inf), (-0.25, 8), (W0 - 0.75, 9), (10, -1e-3), (11, H0 - 1 + 1e-3), (-np.inf, np.nan)]
    rnd = np.stack([rng.uniform(0, W0 - 1, 1000), rng.uniform(0, H0 - 1, 1000)], 1)
    rnd[::7] = np.round(rnd[::7])  # some exactly on pixel centres
    pts = np.concatenate([np.array(border, np.float64), np.array(odd, np.float64), rnd])[:1000].astype(np.float32)
    status = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3], np.uint8), 1000)
    status[:len(border) + len(odd)] = 0
    want_xy, want_st = tn.advance(pts, status, fw, bw)
    assert set(np.unique(want_st[status == 0])) == {0, 1, 2, 3}  # every outcome occurs
    return fw, bw, pts, status, want_xy, want_st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_advance_bitwise(advance_case, n):
    import optical_flow
    fw, bw, pts, status, want_xy, want_st = advance_case
    xy, st = optical_flow.advance_points(pts[:n], fw, bw, status[:n])
    assert xy.dtype == np.float32 and st.dtype == np.uint8
    np.testing.assert_array_equal(st, want_st[:n])
    np.testing.assert_array_equal(xy.view(np.uint32), want_xy[:n].view(np.uint32))
    dead = status[:n] != 0
    np.testing.assert_array_equal(xy[dead].view(np.uint32), pts[:n][dead].view(np.uint32))
    np.testing.assert_array_equal(st[dead], status[:n][dead])


def test_advance_other_thresholds(advance_case):
    import optical_flow
    fw, bw, pts, status, _, _ = advance_case
    kw = dict(alpha1=0.05, alpha2=0.1, beta1=0.0, beta2=0.01)
    xy, st = optical_flow.advance_points(pts, fw, bw, status, **kw)
    want_xy, want_st = tn.advance(pts, status, fw, bw, **kw)
    np.testing.assert_array_equal(st, want_st)
    np.testing.assert_array_equal(xy.view(np.uint32), want_xy.view(np.uint32))


# ---- of_track_seed ----------------------------------------------------------
def gray_plane(H, W, seed):
    """Integer-valued grays: flat 6 x 6 blocks (the eigenvalue test fails
    inside them) with a noisy band (it passes there)."""
    rng = np.random.default_rng(seed)
    g = np.kron(rng.integers(0, 256, (-(-H // 6), -(-W // 6))), np.ones((6, 6)))[:H, :W].astype(np.float64)
    g[H // 3:H // 3 + H // 4] = rng.integers(0, 256, (H // 4, W))
    return g


def table_for(H, W, seed, n=40):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], 1).astype(np.float32)
    return xy, rng.choice(np.array([0, 0, 1, 2, 3], np.uint8), n)


@pytest.mark.parametrize("H,W,step", [(H0, W0, 4), (H0, W0, 7), (150, 170, 1)])
@pytest.mark.parametrize("min_eig", [0.0, 40.0])
def test_seed_bitwise(H, W, step, min_eig):
    import optical_flow
    g = gray_plane(H, W, 5)
    xy, st = table_for(H, W, 6)
    flags = tn.seed_flags(g, xy, st, step, min_eig)
    assert flags.any() and not flags.all()
    if min_eig:
        free = tn.seed_flags(g, xy, st, step, 0.0)
        assert (free & ~flags).any()  # both outcomes of the eigenvalue test
    for table in ((None, None), (xy, st)):
        total = int(tn.seed_flags(g, table[0], table[1], step, min_eig).sum())
        n = 0 if table[0] is None else len(table[0])
        for max_tracks in (n + total + 5, n + total - 1):
            want, want_drop = tn.seed(g, table[0], table[1], step, max_tracks, min_eig)
            assert want_drop == (0 if max_tracks >= n + total else 1)
            got, drop = optical_flow.seed_points(g, table[0], table[1], step, max_tracks, min_eig, frame=3,
                                                 return_dropped=True)
            assert got.dtype == np.float32 and drop == want_drop
            np.testing.assert_array_equal(got, want)
            again, drop2 = optical_flow.seed_points(g, table[0], table[1], step, max_tracks, min_eig, frame=3,
                                                    return_dropped=True)
            np.testing.assert_array_equal(again, got)
            assert drop2 == drop


def test_seed_full_table_adds_nothing():
    import optical_flow
    g = gray_plane(H0, W0, 5)
    xy, st = table_for(H0, W0, 6)
    got, drop = optical_flow.seed_points(g, xy, st, 4, len(xy), 0.0, return_dropped=True)
    assert got.shape == (0, 2) and drop == int(tn.seed_flags(g, xy, st, 4, 0.0).sum())


# ---- the session equals its parts ------------------------------------------
def moving_frames(H, W, C, n, seed):
    """n integer-valued frames: windows of one smooth random canvas, moving by
    (2, 1) px per frame."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 255, (H // 4 + 4, W // 4 + 6, C))
    c = np.kron(c, np.ones((4, 4, 1)))
    for _ in range(3):  # smooth the blocks a little
        c = (c + np.roll(c, 1, 0) + np.roll(c, 1, 1) + np.roll(c, (1, 1), (0, 1))) / 4.0
    c = np.round(c + rng.uniform(-6, 6, c.shape)).clip(0, 255)
    fr = [c[4 + k:4 + k + H, 8 - 2 * k:8 - 2 * k + W] for k in range(n)]
    return [f[..., 0].copy() if C == 1 else f.copy() for f in fr]


@pytest.mark.parametrize("C_", [3, 1])
def test_session_equals_its_parts(C_):
    import optical_flow
    from optical_flow.interface import _rgb2gray
    H, W = 48, 64
    frames = moving_frames(H, W, C_, 4, 21)
    kw = dict(step=8, max_tracks=52, min_eig=4.0)
    xy = st = start = None
    dropped_any = 0
    with optical_flow.PointTracker(frames[0].shape, "classic+nl-fast", **kw) as tr:
        for k, f in enumerate(frames):
            snap = tr.push(f, return_flows=True)
            gray = _rgb2gray(f)
            if k == 0:
                assert snap.forward is None and snap.occ_forward is None
                xy, st, start = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.int32)
            else:
                r = optical_flow.estimate_flow_bidirectional(frames[k - 1], f, "classic+nl-fast")
                np.testing.assert_array_equal(snap.forward, r.forward)
                np.testing.assert_array_equal(snap.backward, r.backward)
                np.testing.assert_array_equal(snap.occ_forward, r.occ_forward)
                np.testing.assert_array_equal(snap.occ_backward, r.occ_backward)
                xy, st = optical_flow.advance_points(xy, r.forward, r.backward, st)
            new, drop = optical_flow.seed_points(gray, xy, st, frame=k, return_dropped=True, **kw)
            xy = np.concatenate([xy, new])
            st = np.concatenate([st, np.zeros(len(new), np.uint8)])
            start = np.concatenate([start, np.full(len(new), k, np.int32)])
            dropped_any += drop
            assert (snap.n_new, snap.n_dropped) == (len(new), drop), k
            np.testing.assert_array_equal(snap.xy.view(np.uint32), xy.view(np.uint32))
            np.testing.assert_array_equal(snap.status, st)
            np.testing.assert_array_equal(snap.start, start)
    assert (start > 0).any() and dropped_any > 0  # it re-seeded later, and the table ran full
    print("tracks", len(xy), "status", np.bincount(st, minlength=4), "dropped", dropped_any)


# ---- lifecycle ---------------------------------------------------------------
def test_lifecycle_and_device_bytes():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    frames = moving_frames(H, W, 1, 3, 8)
    f0 = _native.f32(frames[0])
    n = C.c_int32(0)
    assert lib.of_tracks_push(h, _native.ptr(f0), None, None, None, None, C.byref(n), None, None, None,
                              None) == _abi.OF_EINVAL
    assert lib.of_tracks_read(h, 0, 0, None, None, None) == _abi.OF_EINVAL
    assert lib.of_tracks_close(h) == _abi.OF_EINVAL

    def run(between=None, watch=None):
        snaps = []
        with optical_flow.PointTracker((H, W), step=4, min_eig=1.0) as tr:
            if watch is not None:
                watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
            with pytest.raises(ValueError):
                optical_flow.PointTracker((H, W))  # one tracker per context
            for f in frames:
                snaps.append(tr.push(f))
                if between:
                    between()
                if watch is not None:
                    watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        return snaps

    base = run()  # also grows the arena to what these pairs need
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    watch = []
    again = run(watch=watch)
    # the tracker's own buffers are counted from open to close and nothing else moves
    assert watch[0] - b0 >= 2 * H * W * 4 and all(w == watch[0] for w in watch), (b0, watch)
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    other = moving_frames(40, 56, 3, 2, 9)
    mixed = run(between=lambda: optical_flow.estimate_flow(other[0], other[1], "classic+nl-fast"))
    for a in (again, mixed):
        for s, t in zip(base, a):
            np.testing.assert_array_equal(s.xy.view(np.uint32), t.xy.view(np.uint32))
            np.testing.assert_array_equal(s.status, t.status)
            np.testing.assert_array_equal(s.start, t.start)
            assert (s.n_new, s.n_dropped) == (t.n_new, t.n_dropped)
    assert len(base[-1].xy) > 0
    # the table can be read in parts; out-of-range reads are refused
    with optical_flow.PointTracker((H, W), step=4, min_eig=1.0) as tr:
        s = tr.push(frames[0])
        m = len(s.xy)
        part = np.empty((m - 3, 2), np.float32)
        assert lib.of_tracks_read(h, 3, m - 3, _native.ptr(part), None, None) == 0
        np.testing.assert_array_equal(part, s.xy[3:])
        assert lib.of_tracks_read(h, 3, m - 2, _native.ptr(part), None, None) == _abi.OF_EINVAL
        assert lib.of_tracks_read(h, -1, 1, None, None, None) == _abi.OF_EINVAL
    assert lib.of_tracks_close(h) == _abi.OF_EINVAL


# ---- it tracks ----------------------------------------------------------------
SHIFT = (1.5, -0.75)  # px per frame, (x, y)


def texture(x, y):
    """An analytic texture: evaluated at shifted coordinates it gives an
    exactly shifted frame with no resampling."""
    return (127.5 + 38.0 * np.sin(0.35 * x + 0.2 * y) + 33.0 * np.sin(-0.22 * x + 0.41 * y + 1.0)
            + 27.0 * np.sin(0.6 * x - 0.5 * y + 2.0) + 22.0 * np.sin(0.13 * x + 0.71 * y + 0.5))


def score(pts, xy, st, H, W, T):
    """Of the frame-0 tracks at least 12 px from the border: the share alive
    at the end and the largest distance of a survivor from its true place."""
    sel = (pts[:, 0] >= 12) & (pts[:, 0] <= W - 1 - 12) & (pts[:, 1] >= 12) & (pts[:, 1] <= H - 1 - 12)
    alive = sel & (st == tn.ALIVE)
    true = pts.astype(np.float64) + (T - 1) * np.array(SHIFT)
    d = np.sqrt(((xy.astype(np.float64) - true) ** 2).sum(1))
    return int(sel.sum()), alive.sum() / sel.sum(), float(d[alive].max())


def test_it_tracks_a_known_motion():
    """Five 64 x 96 frames of the texture moving by (1.5, -0.75) px per frame.
    Reference: the restatement driven by the fp64 oracle's flows (two
    estimate_flow calls per pair).  Measured reference (45 tracks scored):
    surviving share 1.0, largest drift 0.0578 px; the GPU measured the same
    (share 1.0, 0.0578 px).
    Gates: the GPU's largest drift <= 2 x the reference's (the drift is the
    method's flow error, common to both; the factor covers fp32 against fp64
    flows), its surviving share >= the reference's - 0.02; the sample counts
    only while the reference itself keeps >= 90 %."""
    import optical_flow
    import oracle
    H, W, T = 64, 96, 5
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = [texture(xx - SHIFT[0] * k, yy - SHIFT[1] * k) for k in range(T)]
    kw = dict(step=8, min_eig=25.0)
    pts, _ = tn.seed(frames[0], None, None, 8, 4 * 8 * 12, 25.0)
    xy, st = pts.copy(), np.zeros(len(pts), np.uint8)
    for k in range(1, T):
        fw = oracle.estimate_flow(frames[k - 1], frames[k], "classic+nl-fast")
        bw = oracle.estimate_flow(frames[k], frames[k - 1], "classic+nl-fast")
        xy, st = tn.advance(xy, st, fw, bw)
    n_ref, share_ref, drift_ref = score(pts, xy, st, H, W, T)
    tr = optical_flow.track_points(frames, "classic+nl-fast", **kw)
    first = tr.start == 0
    np.testing.assert_array_equal(tr.xy[0, first], pts)  # the same frame-0 seeds
    last = np.where(np.isnan(tr.xy[-1, first]), 0, tr.xy[-1, first])
    n_gpu, share_gpu, drift_gpu = score(pts, last, tr.status[first], H, W, T)
    print(f"scored {n_ref}: reference share {share_ref:.3f} drift {drift_ref:.4f} px; "
          f"GPU share {share_gpu:.3f} drift {drift_gpu:.4f} px")
    assert n_gpu == n_ref >= 40
    assert share_ref >= 0.90
    assert drift_gpu <= 2.0 * drift_ref
    assert share_gpu >= share_ref - 0.02
    assert tr.xy.shape == (T, len(tr), 2) and np.all(tr.length[first & (tr.status == 0)] == T)
