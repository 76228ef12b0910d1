"""Dense point trajectories across a frame sequence (Sundaram, Brox and
Keutzer, ECCV 2010): points carried from frame to frame by the forward flow,
ended where the forward-backward test, the frame border or a motion boundary
says so, and re-seeded on a grid wherever the picture has structure and no
live track covers the cell.  include/optflow.h ("Dense point trajectories")
states the arithmetic; the table, the frames and the flows stay on the GPU
(of_tracks_*), only point positions come back per frame.

A point is (x, y) = (column, row), pixel centres at integers, as for flows."""
import ctypes as C
from collections import namedtuple

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import Session, _clip, _frame_size, _int_in

# status of a track (of_track_advance, include/optflow.h)
TRACK_ALIVE = _abi.OF_TRACK_ALIVE
TRACK_OCCLUDED = _abi.OF_TRACK_OCCLUDED
TRACK_LEFT_FRAME = _abi.OF_TRACK_LEFT_FRAME
TRACK_MOTION_BOUNDARY = _abi.OF_TRACK_MOTION_BOUNDARY


def _cells(H, W, step):
    return -(-H // step) * -(-W // step)


def _track_opts(H, W, step=8, max_tracks=None, alpha1=0.01, alpha2=0.5, beta1=0.01, beta2=0.002, min_eig=25.0):
    """of_track_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    step = _int_in("step", step, 1, _abi.TRACK_MAX_STEP)
    if max_tracks is None:
        max_tracks = min(4 * _cells(H, W, step), _abi.TRACK_MAX_TRACKS)
    max_tracks = _int_in("max_tracks", max_tracks, 1, _abi.TRACK_MAX_TRACKS)
    vals = {"alpha1": alpha1, "alpha2": alpha2, "beta1": beta1, "beta2": beta2, "min_eig": min_eig}
    for k, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) \
                or not np.isfinite(v) or v < 0:
            raise ValueError(f"{k} must be a finite number >= 0, got {v!r}")
    return _abi.OfTrackOpts(step, max_tracks, float(alpha1), float(alpha2), float(beta1), float(beta2),
                            float(min_eig))


def _table(xy, status, allow_none):
    """The points as contiguous (N, 2) float32 and their status as (N,) uint8
    (all alive when None); (None, None) for no table at all."""
    if xy is None:
        if status is not None or not allow_none:
            raise ValueError("xy must be an (N, 2) array of points")
        return None, None
    xy = np.asarray(xy)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.dtype.kind not in "fiu":
        raise ValueError(f"xy must be an (N, 2) array of numbers, got {xy.dtype} {xy.shape}")
    n = xy.shape[0]
    if n > _abi.TRACK_MAX_TRACKS:
        raise ValueError(f"at most {_abi.TRACK_MAX_TRACKS} points")
    if status is None:
        st = np.zeros(n, dtype=np.uint8)
    else:
        st = np.asarray(status)
        if st.shape != (n,) or st.dtype.kind not in "iu" or (n and (st.min() < 0 or st.max() > 255)):
            raise ValueError(f"status must be ({n},) integers in 0..255, got {st.dtype} {st.shape}")
        st = np.ascontiguousarray(st, dtype=np.uint8)
    with np.errstate(over='ignore'):
        return nat.f32(xy), st


def advance_points(xy, fw, bw, status=None, alpha1=0.01, alpha2=0.5, beta1=0.01, beta2=0.002):
    """One step of the points `xy` (N, 2) along the forward flow `fw` (frame k
    -> k+1) with the backward flow `bw` (frame k+1 -> k), both (H, W, 2):
    returns (xy, status), (N, 2) float32 and (N,) uint8.  A point whose
    `status` is not TRACK_ALIVE (None: all alive) comes back as it is; an
    alive one moves by the bilinearly sampled flow, or ends with
    TRACK_LEFT_FRAME, TRACK_OCCLUDED (forward-backward test with alpha1,
    alpha2, as forward_backward_check) or TRACK_MOTION_BOUNDARY (flow gradient
    test with beta1, beta2), keeping its position (of_track_advance)."""
    fw, bw = np.asarray(fw), np.asarray(bw)
    if fw.ndim != 3 or fw.shape[2] != 2 or bw.shape != fw.shape or fw.dtype.kind not in "fiu" \
            or bw.dtype.kind not in "fiu":
        raise ValueError(f"flows must share one (H, W, 2) shape, got {fw.shape} / {bw.shape}")
    H, W = fw.shape[:2]
    _frame_size(H, W)
    pts, st = _table(xy, status, allow_none=False)
    opts = _track_opts(H, W, 1, 1, alpha1, alpha2, beta1, beta2, 0.0)
    n = pts.shape[0]
    if n == 0:
        return pts.copy(), st.copy()
    out_xy = np.empty((n, 2), dtype=np.float32)
    out_st = np.empty(n, dtype=np.uint8)
    ctx = nat.context()
    ctx.check(ctx.lib.of_track_advance(ctx.handle, nat.ptr(nat.planar(fw)), nat.ptr(nat.planar(bw)), H, W,
                                       C.byref(opts), n, nat.ptr(pts), nat.u8ptr(st), nat.ptr(out_xy),
                                       nat.u8ptr(out_st)))
    return out_xy, out_st


def seed_points(gray, xy=None, status=None, step=8, max_tracks=None, min_eig=25.0, frame=0, return_dropped=False):
    """New points on the (H, W) gray plane for a table `xy` (N, 2) / `status`
    (None: no table / all alive): one candidate per step x step cell (its
    centre pixel), taken where no alive point of the table occupies the cell
    and the smallest eigenvalue of the 3 x 3 structure tensor is >= min_eig
    (0 takes every free cell), in row-major cell order, while the table has
    room (max_tracks, default 4 x the number of cells).  Returns the new
    points, (M, 2) float32; with `return_dropped` also the number of accepted
    cells the table had no room for (of_track_seed).

    min_eig = 25 is nine window pixels at a gradient of 5/3 gray levels per
    pixel in the weaker direction: a default for 0..255 grays, not a gate.  It
    scales with the square of the image range (0..1 images: 25 / 255^2)."""
    gray = np.asarray(gray)
    if gray.ndim != 2 or gray.size == 0 or gray.dtype.kind not in "fiub":
        raise ValueError(f"gray must be a non-empty (H, W) plane of numbers, got {gray.dtype} {gray.shape}")
    H, W = gray.shape
    _frame_size(H, W)
    opts = _track_opts(H, W, step, max_tracks, min_eig=min_eig)
    frame = _int_in("frame", frame, 0, (1 << 31) - 1)
    pts, st = _table(xy, status, allow_none=True)
    n = 0 if pts is None else pts.shape[0]
    if n > opts.max_tracks:
        raise ValueError(f"the table holds {n} points, more than max_tracks = {opts.max_tracks}")
    room = min(opts.max_tracks - n, _cells(H, W, opts.step))
    out = np.empty((max(room, 1), 2), dtype=np.float32)
    n_new, n_drop = np.zeros(1, np.int32), np.zeros(1, np.int32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_track_seed(ctx.handle, nat.ptr(nat.f32(gray)), H, W, C.byref(opts), frame, n,
                                    nat.ptr(pts if n else None), nat.u8ptr(st if n else None), nat.i32ptr(n_new),
                                    nat.i32ptr(n_drop), nat.ptr(out)))
    new = out[:int(n_new[0])].copy()
    return (new, int(n_drop[0])) if return_dropped else new


TrackSnapshot = namedtuple('TrackSnapshot', ['xy', 'status', 'start', 'n_new', 'n_dropped', 'forward', 'backward',
                                             'occ_forward', 'occ_backward'])


class PointTracker(Session):
    """Dense point tracker over frames of one shape, (H, W) or (H, W, 3): the
    track table, the previous frame and both flows of every pair stay on the
    GPU (of_tracks_open / of_tracks_push, include/optflow.h).

        with PointTracker(frames[0].shape) as tr:
            for f in frames:
                snap = tr.push(f)       # snap.xy (N, 2), snap.status (N,), snap.start (N,)

    The flows of a pair are those of estimate_flow_bidirectional(prev, cur,
    method, params, alpha1, alpha2); step, max_tracks and min_eig as
    seed_points, the thresholds as advance_points.  A track's id is its row
    in the table and never changes; ended tracks keep their row.  One tracker
    per context: by default the calling thread's context (other calls of the
    package may run between pushes), or a `context` (_native.Context) of
    your own for a second tracker at the same time.

    `scale` = 2..4 estimates every pair's flows at 1/scale of the resolution
    and brings them back along the frames' edges, as estimate_flow_bidirectional
    with the same `scale` / `upsample_range` does (of_session_set_flow_scale);
    the table and everything else stay at full resolution.  1 is the
    full-resolution tracker."""

    _PREFIX, _NAME, _KIND = "of_tracks_", "tracker", _abi.OF_SESSION_TRACKS

    def __init__(self, shape, method='classic+nl-fast', params=None, step=8, max_tracks=None, min_eig=25.0,
                 alpha1=0.01, alpha2=0.5, beta1=0.01, beta2=0.002, context=None, scale=1, upsample_range=20.0):
        super().__init__(shape, method, params,
                         lambda H, W: _track_opts(H, W, step, max_tracks, alpha1, alpha2, beta1, beta2, min_eig),
                         context, scale, upsample_range)

    def push(self, frame, return_flows=False):
        """The next frame.  Returns a TrackSnapshot: xy (N, 2) float32, status
        (N,) uint8 and start (N,) int32 of every track so far, n_new and
        n_dropped of this frame's seeding; with `return_flows` also forward,
        backward (H, W, 2) float64 and occ_forward, occ_backward (H, W) uint8
        of the pair (previous frame, this frame), None on the first push."""
        H, W = self.H, self.W
        flows = return_flows and self.frames > 0
        out_f = np.empty((2, H, W), dtype=np.float32) if flows else None
        out_b = np.empty((2, H, W), dtype=np.float32) if flows else None
        occ_f = np.empty((H, W), dtype=np.uint8) if flows else None
        occ_b = np.empty((H, W), dtype=np.uint8) if flows else None
        cnt = np.zeros(3, dtype=np.int32)
        st_f, st_b = _abi.OfStats(), _abi.OfStats()
        self._push(frame, nat.ptr(out_f), nat.ptr(out_b), nat.u8ptr(occ_f), nat.u8ptr(occ_b), nat.i32ptr(cnt),
                   nat.i32ptr(cnt[1:]), nat.i32ptr(cnt[2:]), C.byref(st_f), C.byref(st_b))
        self.last_stats = (st_f.as_dict(), st_b.as_dict()) if self.frames > 1 else None
        n = int(cnt[0])
        xy = np.empty((n, 2), dtype=np.float32)
        status = np.empty(n, dtype=np.uint8)
        start = np.empty(n, dtype=np.int32)
        if n:
            self._call("read", 0, n, nat.ptr(xy), nat.u8ptr(status), nat.i32ptr(start))
        return TrackSnapshot(xy, status, start, int(cnt[1]), int(cnt[2]),
                             nat.interleaved(out_f) if flows else None, nat.interleaved(out_b) if flows else None,
                             occ_f, occ_b)


class Trajectories:
    """The tracks of a sequence of T frames: xy (T, N, 2) float32, NaN outside
    a track's life; per track start (the frame it was seeded in), length (the
    frames it was alive in, start .. start + length - 1) and the final status
    (TRACK_ALIVE: still tracked in the last frame).  len() is N."""

    def __init__(self, xy, start, length, status):
        self.xy, self.start, self.length, self.status = xy, start, length, status

    def __len__(self):
        return self.xy.shape[1]

    @classmethod
    def from_snapshots(cls, snaps):
        """Assemble from the per-frame snapshots (xy, status, start, ...) of a
        tracker: a track is present in the frames whose snapshot has it alive."""
        T = len(snaps)
        N = snaps[-1][0].shape[0] if T else 0
        xy = np.full((T, N, 2), np.nan, dtype=np.float32)
        length = np.zeros(N, dtype=np.int32)
        for t, s in enumerate(snaps):
            alive = np.flatnonzero(np.asarray(s[1]) == TRACK_ALIVE)
            xy[t, alive] = s[0][alive]
            length[alive] += 1
        if T:
            return cls(xy, np.array(snaps[-1][2], dtype=np.int32), length, np.array(snaps[-1][1], dtype=np.uint8))
        return cls(xy, np.zeros(0, np.int32), length, np.zeros(0, np.uint8))


def track_points(frames, method='classic+nl-fast', params=None, step=8, max_tracks=None, min_eig=25.0, alpha1=0.01,
                 alpha2=0.5, beta1=0.01, beta2=0.002, scale=1, upsample_range=20.0):
    """Track points through `frames` (a sequence of at least one (H, W) or
    (H, W, 3) frame of one shape) with a PointTracker; returns Trajectories.
    `scale` / `upsample_range` as PointTracker."""
    frames = _clip(frames)
    with PointTracker(frames[0].shape, method, params, step, max_tracks, min_eig, alpha1, alpha2, beta1,
                      beta2, None, scale, upsample_range) as tr:
        snaps = [tr.push(f) for f in frames]
    return Trajectories.from_snapshots(snaps)
