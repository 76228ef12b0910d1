"""Flow-guided video inpainting (object removal): a region is marked in every
frame of a clip (masks.propagate_masks makes those masks from one drawn mask),
and the region is filled with what the other frames show there, carried along
the motion.  Under the marks the flows are completed from
their surroundings by the solver (a data weight of 0, pair_weight); a marked
pixel then walks through the completed flows of the adjacent pairs, forward and
backward, until it lands on a pixel that some frame really saw
(propagate_fill).  include/optflow.h ("Flow-guided video inpainting") states
the arithmetic; in a session the frames, masks and flows stay on the GPU
(of_inpaint_*), only the filled frames come back.

Gradient-domain blending (blend_fill, `blend=True` in the session) runs a
Poisson solve over the hole on top of that fill: the propagated colours supply
the gradients and the frame's own pixels around the hole the boundary values,
so an exposure offset of a source frame is spread through the hole instead of
showing at its rim, and a pixel that no frame reveals gets a smooth membrane
fill (INPAINT_SPATIAL) instead of keeping the object's colour.  poisson_fill is
the solver on its own.

Masks are (H, W) arrays of a bool or integer dtype, nonzero where a pixel is to
be replaced.  Known limits: without blending a pixel that no frame within
`radius` reveals comes back INPAINT_UNFILLED and a source frame's exposure shows
as a patch; with it the spatial fill is smooth (no texture is synthesised), a
gain change is only partly corrected and the seams between colours from
different source frames stay; the forward-backward states are not used; a hole
bordered by two motions gets the smoothness term's blend of them; no `scale`,
batch or stream variant; the masks must cover shadows and reflections
themselves, `grow` only pads them."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import DelayedSession, _clip, _flow, _frame_size, _int_in, _planar32

INPAINT_KEPT, INPAINT_FILLED, INPAINT_UNFILLED = (_abi.OF_INPAINT_KEPT, _abi.OF_INPAINT_FILLED,
                                                  _abi.OF_INPAINT_UNFILLED)
INPAINT_SPATIAL = _abi.OF_INPAINT_SPATIAL


def _inpaint_opts(radius=8, grow=2, margin=4):
    """of_inpaint_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    return _abi.OfInpaintOpts(_int_in("radius", radius, 1, _abi.INPAINT_MAX_RADIUS),
                              _int_in("grow", grow, 0, _abi.INPAINT_MAX_GROW),
                              _int_in("margin", margin, 0, _abi.INPAINT_MAX_MARGIN), 0)


def _blend_opts(cycles=8, sweeps=2, coarse_sweeps=32):
    """of_blend_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    return _abi.OfBlendOpts(_int_in("cycles", cycles, 1, _abi.BLEND_MAX_CYCLES),
                            _int_in("sweeps", sweeps, 1, _abi.BLEND_MAX_SWEEPS),
                            _int_in("coarse_sweeps", coarse_sweeps, 1, _abi.BLEND_MAX_COARSE_SWEEPS), 0)


def _mask(name, m, shape=None):
    """A mask as contiguous (H, W) uint8 0 / 1."""
    m = np.asarray(m)
    if m.ndim != 2 or m.size == 0 or m.dtype.kind not in "iub" or (shape is not None and m.shape != shape):
        want = "(H, W)" if shape is None else f"{shape}"
        raise ValueError(f"{name} must be a non-empty {want} array of a bool or integer dtype, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def _finite_frame(name, f, shape=None):
    f = np.asarray(f)
    if f.dtype.kind not in "fiu" or (shape is not None and f.shape != shape):
        want = "arrays of numbers" if shape is None else f"{shape} arrays of numbers"
        raise ValueError(f"{name} must be {want}, got {f.dtype} {f.shape}")
    if not np.all(np.isfinite(f)):
        raise ValueError(f"{name} must be finite everywhere")
    return f


def grow_mask(mask, g):
    """`mask` grown by `g` (0..24) pixels per axis: (H, W) uint8, 1 where any
    pixel of `mask` within the (2 g + 1)-wide window is nonzero (positions
    outside the frame count as 0), else 0; g = 0 gives mask != 0
    (of_mask_grow)."""
    m = _mask("mask", mask)
    g = _int_in("g", g, 0, _abi.MASK_GROW_MAX)
    H, W = m.shape
    _frame_size(H, W)
    out = np.empty((H, W), dtype=np.uint8)
    ctx = nat.context()
    ctx.check(ctx.lib.of_mask_grow(ctx.handle, nat.u8ptr(m), None, H, W, g, nat.u8ptr(out), None))
    return out


def pair_weight(mask_a, mask_b, grow=2, margin=4):
    """The data weight the inpainter estimates the pair of two adjacent frames
    with, from their masks: (H, W) float32, 0 where either mask grown by
    `grow`, and then their union by `margin`, is set, else 1.  Pass it as
    estimate_flow(..., data_weight=...) in both directions: the data term is
    then off under the holes of either frame, `margin` pixels around them and
    where the other frame's hole may land, and the flow there is completed from
    its surroundings."""
    a = _mask("mask_a", mask_a)
    H, W = a.shape
    b = _mask("mask_b", mask_b, (H, W))
    o = _inpaint_opts(1, grow, margin)
    _frame_size(H, W)
    ctx = nat.context()
    da, db = np.empty((H, W), dtype=np.uint8), np.empty((H, W), dtype=np.uint8)
    ctx.check(ctx.lib.of_mask_grow(ctx.handle, nat.u8ptr(a), None, H, W, o.grow, nat.u8ptr(da), None))
    ctx.check(ctx.lib.of_mask_grow(ctx.handle, nat.u8ptr(b), None, H, W, o.grow, nat.u8ptr(db), None))
    w = np.empty((H, W), dtype=np.float32)
    ctx.check(ctx.lib.of_mask_grow(ctx.handle, nat.u8ptr(da), nat.u8ptr(db), H, W, o.margin, None, nat.ptr(w)))
    return w


def _clip_and_masks(frames, masks):
    """A clip and its masks, validated: (frames, masks, H, W, channels), the
    masks contiguous uint8 0 / 1."""
    frames = _clip(frames)
    f0 = frames[0]
    if f0.ndim not in (2, 3) or f0.size == 0:
        raise ValueError(f"frames must be non-empty (H, W) or (H, W, C) arrays, got {f0.shape}")
    frames = [_finite_frame("frames", f) for f in frames]
    H, W = f0.shape[:2]
    _frame_size(H, W)
    masks = list(masks)
    if len(masks) != len(frames):
        raise ValueError(f"{len(frames)} frames but {len(masks)} masks")
    masks = [_mask(f"masks[{k}]", m, (H, W)) for k, m in enumerate(masks)]
    return frames, masks, H, W, 1 if f0.ndim == 2 else f0.shape[2]


def _fill_inputs(frames, masks, fw, bw, t):
    """The clip, masks and flows of a fill of frame t, validated, as the C
    entries take them: ((frames, masks, fw, bw), T, H, W, channels, t,
    the frames' shape)."""
    frames, masks, H, W, Cc = _clip_and_masks(frames, masks)
    if not 1 <= Cc <= _abi.INPAINT_MAX_CHANNELS:
        raise ValueError(f"frames must have 1..{_abi.INPAINT_MAX_CHANNELS} channels, got {Cc}")
    T = len(frames)
    fw, bw = list(fw), list(bw)
    if len(fw) != T - 1 or len(bw) != T - 1:
        raise ValueError(f"{T} frames take {T - 1} forward and backward flows, got {len(fw)} and {len(bw)}")
    fw = [_flow(f"fw[{k}]", f, (H, W)) for k, f in enumerate(fw)]
    bw = [_flow(f"bw[{k}]", f, (H, W)) for k, f in enumerate(bw)]
    t = _int_in("t", t, 0, T - 1)
    fr32 = nat.f32(np.stack([np.asarray(f, dtype=float) for f in frames]))
    m8 = np.ascontiguousarray(np.stack(masks))
    fw32 = np.ascontiguousarray(np.stack([_planar32(f) for f in fw])) if T > 1 else None
    bw32 = np.ascontiguousarray(np.stack([_planar32(f) for f in bw])) if T > 1 else None
    return (fr32, m8, fw32, bw32), T, H, W, Cc, t, frames[0].shape


def _ptrs(a):
    return nat.ptr(a[0]), nat.u8ptr(a[1]), nat.ptr(a[2]), nat.ptr(a[3])


def propagate_fill(frames, masks, fw, bw, t, radius=8, grow=2, return_status=False, return_hops=False):
    """Frame `t` of the clip `frames` ((H, W) or (H, W, C) with C <= 4, one
    shape) with the pixels of its mask filled from the other frames: returns
    the filled frame, float64 in the frames' shape.  `masks` has one mask per
    frame, each grown by `grow` (0..8) first; `fw[s]` and `bw[s]` are the
    (H, W, 2) flows of the pair (s, s+1), s -> s+1 and s+1 -> s, len(frames) - 1
    of each (estimate them with pair_weight as the data weight).

    A pixel outside the grown mask comes back as it is.  A pixel inside walks
    forward along fw[t], fw[t+1], ... and backward along bw[t-1], bw[t-2], ...,
    at most `radius` (1..16) frames each way, until it lands on four pixels
    outside that frame's grown mask; the two colours found are blended, the
    nearer frame counting more (of_inpaint_fill).  With `return_status` also
    the (H, W) uint8 plane of INPAINT_KEPT / INPAINT_FILLED / INPAINT_UNFILLED;
    with `return_hops` also the (2, H, W) uint8 hop counts of the forward and
    the backward walk (0: no hit)."""
    a, T, H, W, Cc, t, shape = _fill_inputs(frames, masks, fw, bw, t)
    opts = _inpaint_opts(radius, grow)
    out = np.empty(shape, dtype=np.float32)
    status = np.empty((H, W), dtype=np.uint8) if return_status else None
    hops = np.empty((2, H, W), dtype=np.uint8) if return_hops else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_inpaint_fill(ctx.handle, *_ptrs(a), T, H, W, Cc, t, C.byref(opts), nat.ptr(out), nat.u8ptr(status),
                                      nat.u8ptr(hops)))
    res = (out.astype(np.float64),) + ((status,) if return_status else ()) + ((hops,) if return_hops else ())
    return res if len(res) > 1 else res[0]


def blend_fill(frames, masks, fw, bw, t, radius=8, grow=2, cycles=8, sweeps=2, coarse_sweeps=32, return_status=False):
    """propagate_fill with gradient-domain blending and a spatial fallback
    (of_inpaint_blend): arguments as propagate_fill's.  The frame is filled
    along the flows with the masks grown by one more pixel; over the hole a
    Poisson problem is then solved whose gradients are those of the propagated
    colours and whose boundary values are the frame's own pixels around the
    hole, so a source frame's exposure offset is spread through the hole; the
    pixels that no frame reveals are filled from that result by a second solve
    without gradients (a smooth membrane).  `cycles` (1..64), `sweeps` (1..2)
    and `coarse_sweeps` (1..64) are the multigrid solver's fixed schedule.
    With `return_status` also the (H, W) uint8 plane of INPAINT_KEPT /
    INPAINT_FILLED / INPAINT_SPATIAL; INPAINT_UNFILLED does not occur."""
    a, T, H, W, Cc, t, shape = _fill_inputs(frames, masks, fw, bw, t)
    opts, bopts = _inpaint_opts(radius, grow), _blend_opts(cycles, sweeps, coarse_sweeps)
    out = np.empty(shape, dtype=np.float32)
    status = np.empty((H, W), dtype=np.uint8) if return_status else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_inpaint_blend(ctx.handle, *_ptrs(a), T, H, W, Cc, t, C.byref(opts), C.byref(bopts), nat.ptr(out),
                                       nat.u8ptr(status)))
    return (out.astype(np.float64), status) if return_status else out.astype(np.float64)


def poisson_fill(values, unknown, source=None, has_source=None, excluded=None, cycles=8, sweeps=2, coarse_sweeps=32):
    """The Poisson solver of the blended fill on its own (of_poisson_solve):
    `values`, (H, W) or (H, W, C) with C <= 4, with the pixels of the mask
    `unknown` replaced by the solution of the discrete Poisson equation whose
    boundary values are the other pixels of `values`; float64 in the shape of
    `values`.  The pixels of the mask `excluded` take no part (their
    neighbours see a free boundary there) and come back as they are.  With
    `source` (the shape of `values`) and the mask `has_source` the solution
    takes the differences of `source` between neighbouring pixels that both
    have a source as its gradients; without them it is the smooth membrane.
    The unknown pixels of `values` are the start of the fixed multigrid
    schedule (`cycles` W-cycles): a region of unknowns that touches no other
    pixel is singular, and what the schedule makes of its start is returned."""
    v = _finite_frame("values", values)
    if v.ndim not in (2, 3) or v.size == 0 or (v.ndim == 3 and not 1 <= v.shape[2] <= _abi.BLEND_MAX_CHANNELS):
        raise ValueError(f"values must be a non-empty (H, W) or (H, W, C) array with C <= 4, got {v.shape}")
    H, W = v.shape[:2]
    _frame_size(H, W)
    label = _mask("unknown", unknown, (H, W)) * np.uint8(_abi.OF_PSN_UNKNOWN)
    if excluded is not None:
        ex = _mask("excluded", excluded, (H, W))
        if np.any(ex & label):
            raise ValueError("a pixel cannot be both unknown and excluded")
        label = label + ex * np.uint8(_abi.OF_PSN_EXCLUDED)
    if (source is None) != (has_source is None):
        raise ValueError("source and has_source come together")
    s32 = h8 = None
    if source is not None:
        s32 = nat.f32(np.asarray(_finite_frame("source", source, v.shape), dtype=float))
        h8 = _mask("has_source", has_source, (H, W))
    opts = _blend_opts(cycles, sweeps, coarse_sweeps)
    v32 = nat.f32(np.asarray(v, dtype=float))
    out = np.empty(v.shape, dtype=np.float64)
    ctx = nat.context()
    ctx.check(ctx.lib.of_poisson_solve(ctx.handle, nat.u8ptr(np.ascontiguousarray(label)), nat.ptr(v32), nat.ptr(s32),
                                       nat.u8ptr(h8), H, W, 1 if v.ndim == 2 else v.shape[2], C.byref(opts),
                                       nat.dptr(out)))
    return out


class VideoInpainter(DelayedSession):
    """Inpainter over frames of H x W with `channels` 1 ((H, W) frames) or 3
    ((H, W, 3)): the last 2 radius + 1 frames and grown masks and both flows of
    the pairs between them stay on the GPU (of_inpaint_open / _push / _flush).

        with VideoInpainter(H, W, 3, radius=8) as vi:
            for f, m in zip(frames, masks):
                r = vi.push(f, m)       # None for the first `radius` frames,
                ...                     # then (index, filled frame)
            for index, frame in vi.flush():
                ...                     # the last `radius` frames

    Every pair of adjacent frames is estimated in both directions with
    pair_weight(mask, next mask, grow, margin) as estimate_flow's data weight;
    frame t is filled (propagate_fill; with `blend`, blend_fill with `cycles`,
    `sweeps` and `coarse_sweeps`) from frames t - radius .. t + radius that
    exist.  Frames come back as float64 in the frames' shape; `last_status`
    holds the status plane of the frame returned last.  One inpainter per
    context, beside the other sessions.  Methods that take no data weight
    ('classic-c-a', a general spatial_filters list) raise
    NotImplementedError."""

    _PREFIX, _NAME, _KIND = "of_inpaint_", "inpainter", None

    def __init__(self, H, W, channels=3, method='classic+nl-fast', params=None, radius=8, grow=2, margin=4,
                 context=None, blend=False, cycles=8, sweeps=2, coarse_sweeps=32):
        for name, v in (("H", H), ("W", W)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if isinstance(channels, bool) or channels not in (1, 3):
            raise ValueError(f"channels must be 1 or 3, got {channels!r}")
        shape = (int(H), int(W)) if channels == 1 else (int(H), int(W), 3)
        if not isinstance(blend, (bool, np.bool_)):
            raise ValueError(f"blend must be True or False, got {blend!r}")
        bopts = _blend_opts(cycles, sweeps, coarse_sweeps)
        super().__init__(shape, method, params, lambda h, w: _inpaint_opts(radius, grow, margin), context)
        self.radius, self.grow, self.margin = self._opts.radius, self._opts.grow, self._opts.margin
        self.blend = bool(blend)
        self.last_status = None
        if self.blend:
            try:
                self._call("set_blend", C.byref(bopts))
            except Exception:
                self.close()
                raise

    def _step(self, call, *args):
        out = np.empty(self.shape, dtype=np.float32)
        status = np.empty((self.H, self.W), dtype=np.uint8)
        idx = np.full(1, -1, dtype=np.int32)
        call(*args, nat.ptr(out), nat.u8ptr(status), nat.i32ptr(idx))
        if idx[0] < 0:
            return None
        self.last_status = status
        return int(idx[0]), out.astype(np.float64)

    def push(self, frame, mask):
        """The next frame and its mask.  Returns (index, frame) of the filled
        frame that became complete, or None while fewer than radius + 1 frames
        have been pushed."""
        self._live()
        _finite_frame("frames", frame, self.shape)
        m = _mask("mask", mask, (self.H, self.W))
        return self._step(self._push, frame, nat.u8ptr(m))

    def _flush_step(self):
        return self._step(self._call, "flush")


def inpaint_frames(frames, masks, method='classic+nl-fast', radius=8, grow=2, margin=4, return_status=False,
                   params=None, blend=False, cycles=8, sweeps=2, coarse_sweeps=32):
    """Fill the masked regions of `frames` (a sequence of at least one (H, W)
    or (H, W, 3) frame of one shape) with a VideoInpainter; `masks` has one
    mask per frame.  Returns (T,) + the frames' shape, float64; with
    `return_status` also the (T, H, W) uint8 status planes.  `blend`: every
    frame is the blended fill (blend_fill) instead of the plain one."""
    frames, masks, H, W, Cc = _clip_and_masks(frames, masks)
    out = np.empty((len(frames),) + frames[0].shape, dtype=np.float64)
    status = np.empty((len(frames), H, W), dtype=np.uint8)
    with VideoInpainter(H, W, Cc, method, params, radius, grow, margin, None, blend, cycles, sweeps,
                        coarse_sweeps) as vi:
        def take(r):
            if r is not None:
                out[r[0]] = r[1]
                status[r[0]] = vi.last_status
        for f, m in zip(frames, masks):
            take(vi.push(f, m))
        for r in vi.flush():
            take(r)
    return (out, status) if return_status else out
