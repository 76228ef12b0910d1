"""Global (camera) motion from a dense flow, and video stabilisation: the
dominant motion of a flow field is fitted on the GPU as a translation, a
similarity or an affine map by iteratively reweighted least squares with a
decreasing Tukey cutoff; a stabiliser smooths the chain of those motions over
a clip and warps every frame onto the smoothed camera path; segment_motion
splits a flow into several such motions with a label per pixel
("Layered motion segmentation" there).
include/optflow.h ("Global motion estimation and video stabilisation") states
the arithmetic; in a session the frames and flows stay on the GPU
(of_stab_*), only the six numbers of each motion visit the host.

Flows are (H, W, 2) with u along columns, as everywhere in the package; masks
are forward_backward_check's (0 consistent, anything else left out).  A motion
is a (2, 3) matrix acting on points (column, row, 1)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import DelayedSession, _flow, _frame_size, _int_in, _number, _planar32, _state

MotionFit = namedtuple("MotionFit", "matrix theta cutoff support rms passes degenerate inliers")
MotionFit.__doc__ = """Result of fit_motion: `matrix` (2, 3) maps a point (column, row) of the
flow's first frame to the second; `theta` the six parameters in normalised
coordinates; `cutoff` the final Tukey cutoff in pixels; `support` the sum of
the final weights; `rms` the weighted rms residual in pixels; `passes` the
solving passes run; `degenerate` bit flags (1 a pass lost rank and solved the
translation, 2 no support); `inliers` the (H, W) float64 final weights, or
None."""


def _motion_opts(model='affine', iters=10, kappa=2.0, decay=0.5, c_min=0.5):
    """of_motion_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    if not isinstance(model, str) or model not in _abi.MOTION_MODEL:
        raise ValueError(f"model must be one of {sorted(_abi.MOTION_MODEL)}, got {model!r}")
    decay = _number("decay", decay, True)
    if decay > 1.0:
        raise ValueError(f"decay must be in (0, 1], got {decay!r}")
    return _abi.OfMotionOpts(_abi.MOTION_MODEL[model], _int_in("iters", iters, 0, _abi.MOTION_MAX_ITERS),
                             _number("kappa", kappa, True), decay, _number("c_min", c_min, True))


def _matrix(name, m):
    m = np.asarray(m)
    if m.shape != (2, 3) or m.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be a (2, 3) array of numbers, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m, dtype=np.float64)


def fit_motion(flow, model='affine', weight=None, state=None, iters=10, kappa=2.0, decay=0.5, c_min=0.5,
               return_inliers=False):
    """The dominant motion of `flow` (H, W, 2) as a MotionFit: `model` is
    'translation', 'similarity' or 'affine'.  Pixels whose flow is not finite
    or whose `state` (an (H, W) forward-backward mask, or None) is not 0 are
    left out; `weight` (an (H, W) array, finite and >= 0, or None) weighs the
    rest.  Pass 0 is plain least squares; `iters` Tukey-weighted passes follow,
    the cutoff starting at `kappa` times the flow's rms and shrinking by
    `decay` (on its square) per pass down to `c_min` pixels (of_fit_motion).
    With `return_inliers` the final weights come back as `inliers`: near 1 on
    the camera motion, 0 on what moves otherwise."""
    flow = _flow("flow", flow)
    H, W = flow.shape[:2]
    _frame_size(H, W)
    opts = _motion_opts(model, iters, kappa, decay, c_min)
    w = nat.data_weight(weight, H, W)
    st = _state("state", state, H, W)
    fit = _abi.OfMotionFit()
    inl = np.empty((H, W), dtype=np.float32) if return_inliers else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_fit_motion(ctx.handle, nat.ptr(_planar32(flow)), H, W, nat.ptr(w), nat.u8ptr(st),
                                    C.byref(opts), C.byref(fit), nat.ptr(inl)))
    return MotionFit(np.array(fit.matrix, dtype=np.float64).reshape(2, 3), np.array(fit.theta, dtype=np.float64),
                     fit.cutoff, fit.support, fit.rms, fit.passes, fit.degenerate,
                     inl.astype(np.float64) if return_inliers else None)


def warp_affine(im, matrix, return_valid=False):
    """`im`, (H, W) or (H, W, C) with C <= 4, sampled bilinearly through the
    (2, 3) `matrix`, which maps an output pixel (column, row) to its source
    position: float64 in im's shape, 0 where the source lies outside the frame
    or is not finite; with `return_valid` also the (H, W) uint8 mask of the
    pixels that have a source (of_warp_affine)."""
    im = np.asarray(im)
    if im.ndim not in (2, 3) or im.size == 0 or im.dtype.kind not in "fiu":
        raise ValueError(f"im must be a non-empty (H, W) or (H, W, C) array of numbers, got {im.dtype} {im.shape}")
    Cc = 1 if im.ndim == 2 else im.shape[2]
    if not 1 <= Cc <= _abi.FUSE_MAX_CHANNELS:
        raise ValueError(f"im must have 1..{_abi.FUSE_MAX_CHANNELS} channels, got {Cc}")
    H, W = im.shape[:2]
    _frame_size(H, W)
    A = _matrix("matrix", matrix)
    out = np.empty(im.shape, dtype=np.float32)
    valid = np.empty((H, W), dtype=np.uint8) if return_valid else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_warp_affine(ctx.handle, nat.ptr(nat.f32(np.asarray(im, dtype=float))), H, W, Cc,
                                     nat.dptr(A), nat.ptr(out), nat.u8ptr(valid)))
    out = out.astype(np.float64)
    return (out, valid) if return_valid else out


LAYER_NONE = _abi.OF_LAYER_NONE

MotionLayer = namedtuple("MotionLayer", "theta matrix support rms pixels degenerate")
MotionLayer.__doc__ = """One layer of segment_motion: `theta`, `matrix` (2, 3), `support` and `rms` as
in MotionFit, from the closing pass over the layer's pixels; `pixels` the
pixels that carry the layer's label; `degenerate` 1 when a solve of the layer
lost rank and solved the translation."""

MotionLayers = namedtuple("MotionLayers", "labels layers n labels_raw")
MotionLayers.__doc__ = """Result of segment_motion: `labels` (H, W) uint8, the index into `layers` or
LAYER_NONE (255) where no layer explains the pixel; `layers` the `n`
MotionLayer fits in extraction order; `labels_raw` the labels before the mode
filter, or None."""


def segment_motion(flow, model='affine', max_layers=4, grid=8, passes=4, rounds=3, smooth=2, cutoff=1.0,
                   min_support=0.03, weight=None, state=None, return_raw=False):
    """`flow` (H, W, 2) split into up to `max_layers` motions of `model` as a
    MotionLayers (of_segment_motion).  Every cell of a `grid` x `grid`
    partition of the frame proposes the least-squares motion of its own
    pixels; the proposal that explains most of the pixels not yet claimed to
    within `cutoff` pixels is refitted on them by `passes` Tukey passes and
    claims its inliers, until a layer would explain less than `min_support` of
    the usable pixels.  `rounds` rounds of assigning every pixel to its best
    layer and refitting follow, and a mode filter of radius `smooth` cleans
    the labels up.  `weight` and `state` as in fit_motion: they decide what
    enters the fits; every pixel with a finite flow gets a label."""
    flow = _flow("flow", flow)
    H, W = flow.shape[:2]
    _frame_size(H, W)
    if not isinstance(model, str) or model not in _abi.MOTION_MODEL:
        raise ValueError(f"model must be one of {sorted(_abi.MOTION_MODEL)}, got {model!r}")
    min_support = _number("min_support", min_support, True)
    if min_support > 1.0:
        raise ValueError(f"min_support must be in (0, 1], got {min_support!r}")
    opts = _abi.OfLayersOpts(_abi.MOTION_MODEL[model], _int_in("max_layers", max_layers, 1, _abi.LAYERS_MAX),
                             _int_in("grid", grid, 1, _abi.LAYERS_MAX_GRID),
                             _int_in("passes", passes, 0, _abi.LAYERS_MAX_PASSES),
                             _int_in("rounds", rounds, 0, _abi.LAYERS_MAX_ROUNDS),
                             _int_in("smooth", smooth, 0, _abi.LAYERS_MAX_SMOOTH), _number("cutoff", cutoff, True),
                             min_support)
    w = nat.data_weight(weight, H, W)
    st = _state("state", state, H, W)
    fits = (_abi.OfMotionLayer * opts.max_layers)()
    n = C.c_int32(0)
    labels = np.empty((H, W), dtype=np.uint8)
    raw = np.empty((H, W), dtype=np.uint8) if return_raw else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_segment_motion(ctx.handle, nat.ptr(_planar32(flow)), H, W, nat.ptr(w), nat.u8ptr(st),
                                        C.byref(opts), fits, C.byref(n), nat.u8ptr(labels), nat.u8ptr(raw)))
    layers = [MotionLayer(np.array(f.theta, dtype=np.float64), np.array(f.matrix, dtype=np.float64).reshape(2, 3),
                          f.support, f.rms, int(f.pixels), f.degenerate) for f in fits[:n.value]]
    return MotionLayers(labels, layers, n.value, raw)


class Stabilizer(DelayedSession):
    """Video stabiliser over frames of one shape, (H, W) or (H, W, 3): the last
    radius + 1 frames stay on the GPU (of_stab_open / _push / _flush).

        with Stabilizer(frames[0].shape) as st:
            for f in frames:
                r = st.push(f)          # None for the first `radius` frames,
                ...                     # then (index, frame) of frame index
            for index, frame in st.flush():
                ...                     # the last `radius` frames

    Every push after the first estimates estimate_flow_bidirectional(previous
    frame, frame, method, params, alpha1, alpha2) and fits the motion between
    the two (fit_motion on the forward flow with its mask as `state`, `model`
    and the fit options).  Frame t comes back warped onto the camera path
    smoothed over frames t - radius .. t + radius with a Gaussian window of
    `sigma_t` frames, float64 in the input's shape.  After a push or a flush
    step `last_motion` holds the (2, 3) motion fitted in that push (None for
    the first frame and in flush), `last_transform` the (2, 3) S_t of the
    frame returned, `last_valid` its (H, W) uint8 mask of pixels that have a
    source and `last_degenerate` the flags (fit_motion's, | 4 where a motion
    could not be inverted and the identity took its place).  One stabiliser per
    context: by default the calling thread's context (other calls of the
    package may run between pushes), or a `context` (_native.Context) of your
    own.

    `scale` = 2..4 estimates every pair's flows at 1/scale of the resolution
    and brings them back along the frames' edges, as estimate_flow_bidirectional
    with the same `scale` / `upsample_range` does (of_session_set_flow_scale);
    the fit and the warp stay at full resolution.  1 is the full-resolution
    stabiliser."""

    _PREFIX, _NAME, _KIND = "of_stab_", "stabiliser", _abi.OF_SESSION_STAB

    def __init__(self, shape, method='classic+nl-fast', params=None, model='similarity', radius=8, sigma_t=3.0,
                 iters=10, kappa=2.0, decay=0.5, c_min=0.5, alpha1=0.01, alpha2=0.5, context=None, scale=1,
                 upsample_range=20.0):
        super().__init__(shape, method, params, lambda H, W: _abi.OfStabOpts(
            _motion_opts(model, iters, kappa, decay, c_min), _int_in("radius", radius, 1, _abi.STAB_MAX_RADIUS), 0,
            _number("sigma_t", sigma_t, True), _number("alpha1", alpha1, False), _number("alpha2", alpha2, False)),
            context, scale, upsample_range)
        self.radius = self._opts.radius
        self.last_motion = self.last_transform = self.last_valid = None
        self.last_degenerate = 0

    def _step(self, call, *args, motion=None):
        out = np.empty(self.shape, dtype=np.float32)
        valid = np.empty((self.H, self.W), dtype=np.uint8)
        S = np.empty(6, dtype=np.float64)
        deg, idx = np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        call(*args, nat.ptr(out), nat.u8ptr(valid), nat.dptr(S), *([] if motion is None else [nat.dptr(motion)]),
             nat.i32ptr(deg), nat.i32ptr(idx))
        self.last_motion = None if motion is None else motion.reshape(2, 3)
        self.last_degenerate = int(deg[0])
        if idx[0] < 0:
            return None
        self.last_transform, self.last_valid = S.reshape(2, 3).copy(), valid
        return int(idx[0]), out.astype(np.float64)

    def push(self, frame):
        """The next frame.  Returns (index, frame) of the stabilised frame that
        became complete, float64 in the input's shape, or None while fewer
        than radius + 1 frames have been pushed."""
        r = self._step(self._push, frame, motion=np.empty(6, dtype=np.float64))
        if self.frames == 1:
            self.last_motion = None
        return r

    def _flush_step(self):
        return self._step(self._call, "flush")


def stabilize_frames(frames, method='classic+nl-fast', model='similarity', radius=8, sigma_t=3.0, params=None,
                     iters=10, kappa=2.0, decay=0.5, c_min=0.5, alpha1=0.01, alpha2=0.5, return_transforms=False,
                     scale=1, upsample_range=20.0):
    """Stabilise `frames` (a sequence of at least one (H, W) or (H, W, 3)
    frame of one shape) with a Stabilizer: returns (T, H, W[, 3]) float64; with
    `return_transforms` also the (T, 2, 3) float64 S_t each frame was moved
    by (a point of frame t lies at S_t^-1 of it in the output).  `scale` /
    `upsample_range` estimate the flows at reduced resolution (Stabilizer)."""
    out, tr = Stabilizer.run_clip(frames, "last_transform", method, params, model, radius, sigma_t, iters, kappa,
                                  decay, c_min, alpha1, alpha2, None, scale, upsample_range)
    return (out, tr) if return_transforms else out
