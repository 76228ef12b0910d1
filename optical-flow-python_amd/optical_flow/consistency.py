"""Blind temporal consistency: the flicker of a per-frame operator removed.
Beside a clip there is a second one, the same frames after an operator that
knows nothing about time (tone mapping, grading, dehazing, colourisation,
stylisation, inpaint_frames with differing sources per frame): every frame of
it looks right, the clip flickers.  Every output frame keeps the gradients of
its processed frame and leans, where the original frames show the same
surface, on the previous output warped along the backward flow: a screened
Poisson problem per frame (consistency_step; screened_poisson is the solver on
its own).  include/optflow.h ("Blind temporal consistency") states the
arithmetic; in a session the previous frame and output stay on the GPU
(of_consist_*).

Known limits: the first frame's look is the anchor and errors accumulate
along a long clip (`lam` trades flicker against drift; there is no long-term
keyframe); where the forward-backward mask or the weight rejects the past a
pixel follows the processed frame alone, so newly revealed regions can still
flicker; causal, no look-ahead; no `scale`, batch or stream variant."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import Session, _clip, _flow, _frame_size, _int_in, _number, _planar32, _state
from optical_flow.inpaint import _blend_opts, _finite_frame
from optical_flow.temporal import _fuse_opts


def _consist_opts(sigma, lam=1.0, strength=4.0, patch=1, alpha1=0.01, alpha2=0.5, cycles=_abi.CONSIST_CYCLES, sweeps=2,
                  coarse_sweeps=32):
    """of_consist_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    return _abi.OfConsistOpts(_fuse_opts(sigma, 1, strength, patch, alpha1, alpha2),
                              _blend_opts(cycles, sweeps, coarse_sweeps), _number("lam", lam, False))


def _channels(name, a, shape2=None):
    """A finite (H, W) or (H, W, C <= 4) array of numbers and its channel count."""
    a = _finite_frame(name, a)
    if a.ndim not in (2, 3) or a.size == 0 or (a.ndim == 3 and not 1 <= a.shape[2] <= _abi.CONSIST_MAX_CHANNELS) or \
            (shape2 is not None and a.shape[:2] != shape2):
        want = "(H, W) or (H, W, C)" if shape2 is None else f"{shape2} or {shape2 + ('C',)}"
        raise ValueError(f"{name} must be a non-empty {want} array with C <= {_abi.CONSIST_MAX_CHANNELS}, "
                         f"got {a.shape}")
    return a, 1 if a.ndim == 2 else a.shape[2]


def screened_poisson(target, anchor, weight, cycles=_abi.CONSIST_CYCLES, sweeps=2, coarse_sweeps=32):
    """The screened Poisson solver on its own (of_screened_solve): the x that
    has the gradients of `target`, (H, W) or (H, W, C) with C <= 4, and stays
    near `anchor` (the shape of `target`) where the (H, W) plane `weight` >= 0
    is large,
        (deg + weight) x - sum of x over the 4-neighbours in the frame
            = sum of (target - its neighbour) + weight * anchor,
    by `cycles` W-cycles of the fixed multigrid schedule from x = target;
    float64 in the shape of `target`.  Where `weight` is 0 everywhere the
    result is `target` (as float32)."""
    t, Cc = _channels("target", target)
    H, W = t.shape[:2]
    _frame_size(H, W)
    a = _finite_frame("anchor", anchor, t.shape)
    w = np.asarray(weight)
    if w.shape != (H, W) or w.dtype.kind not in "fiu" or not np.all(np.isfinite(w) & (w >= 0)):
        raise ValueError(f"weight must be a ({H}, {W}) array of finite numbers >= 0, got {w.dtype} {w.shape}")
    opts = _blend_opts(cycles, sweeps, coarse_sweeps)
    t32 = nat.f32(np.asarray(t, dtype=float))
    a64 = np.ascontiguousarray(a, dtype=np.float64)
    w64 = np.ascontiguousarray(w, dtype=np.float64)
    out = np.empty(t.shape, dtype=np.float64)
    ctx = nat.context()
    ctx.check(ctx.lib.of_screened_solve(ctx.handle, nat.ptr(t32), nat.dptr(a64), nat.dptr(w64), H, W, Cc, C.byref(opts),
                                        nat.dptr(out)))
    return out


def consistency_step(frame, prev_frame, processed, prev_out, flow, state=None, lam=1.0, sigma=None, strength=4.0,
                     patch=1, cycles=_abi.CONSIST_CYCLES, sweeps=2, coarse_sweeps=32, return_weight=False):
    """One frame made consistent with its predecessor (of_consist_step):
    `processed`, (H, W) or (H, W, Cp) with Cp <= 4, keeps its gradients and
    leans on `prev_out` (its shape), the previous output, warped along `flow`,
    the (H, W, 2) flow from `frame` to `prev_frame` (the original frames, (H, W)
    or (H, W, C) with C <= 4), with `state` its forward-backward mask ((H, W),
    nonzero = not trusted) or None.  Returns float64 in the shape of
    `processed`; with `return_weight` also the (H, W) float64 weight of the
    past, fuse_weights(frame, [prev_frame], [flow], sigma, [state], strength,
    patch)[0].

    `sigma` is required: what the original frames may differ by where they
    show the same surface.  `lam` >= 0 weighs the past: 0 returns `processed`,
    a large value the warped previous output where it is visible."""
    v, Cc = _channels("frame", frame)
    H, W = v.shape[:2]
    _frame_size(H, W)
    pv = _finite_frame("prev_frame", prev_frame, v.shape)
    p, Cp = _channels("processed", processed, (H, W))
    po = _finite_frame("prev_out", prev_out, p.shape)
    f = _flow("flow", flow, (H, W))
    s = _state("state", state, H, W)
    opts = _consist_opts(sigma, lam, strength, patch, cycles=cycles, sweeps=sweeps, coarse_sweeps=coarse_sweeps)
    a32 = [nat.f32(np.asarray(x, dtype=float)) for x in (v, pv, p, po)]
    f32 = _planar32(f)
    out = np.empty(p.shape, dtype=np.float32)
    wgt = np.empty((H, W), dtype=np.float32) if return_weight else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_consist_step(ctx.handle, nat.ptr(a32[0]), nat.ptr(a32[1]), H, W, Cc, nat.ptr(a32[2]),
                                      nat.ptr(a32[3]), Cp, nat.ptr(f32), nat.u8ptr(s), C.byref(opts), nat.ptr(out),
                                      nat.ptr(wgt)))
    out = out.astype(np.float64)
    return (out, wgt.astype(np.float64)) if return_weight else out


class TemporalConsistency(Session):
    """Temporal consistency over frames of one `shape`, (H, W) or (H, W, 3),
    and processed frames of `processed_channels` channels (None: as the
    frames; 1 means (H, W) processed frames, 2..4 (H, W, Cp)): the previous
    frame and the previous output stay on the GPU (of_consist_open / _push /
    _close).

        with TemporalConsistency(frames[0].shape, sigma=4.0) as tc:
            for f, p in zip(frames, processed):
                out = tc.push(f, p)     # the output of this frame

    The first push returns its processed frame; every later one estimates the
    pair (previous, this) in both directions (estimate_flow_bidirectional with
    `alpha1`, `alpha2`) and runs consistency_step along the backward flow with
    its mask.  Frames come back as float64 in the processed frames' shape;
    `last_weight` holds the (H, W) float64 weight of the past in the frame
    returned last (0 after the first push).  `sigma` is required.  One such
    session per context, beside the other kinds; no `scale`."""

    _PREFIX, _NAME, _KIND = "of_consist_", "temporal consistency session", None

    def __init__(self, shape, processed_channels=None, method='classic+nl-fast', params=None, sigma=None, lam=1.0,
                 strength=4.0, patch=1, alpha1=0.01, alpha2=0.5, cycles=_abi.CONSIST_CYCLES, sweeps=2, coarse_sweeps=32,
                 context=None):
        if processed_channels is not None:
            processed_channels = _int_in("processed_channels", processed_channels, 1, _abi.CONSIST_MAX_CHANNELS)
        self._cp = processed_channels
        super().__init__(shape, method, params,
                         lambda h, w: _consist_opts(sigma, lam, strength, patch, alpha1, alpha2, cycles, sweeps,
                                                    coarse_sweeps), context)
        self.processed_shape = (self.H, self.W) if self._cp == 1 else (self.H, self.W, self._cp)
        self.lam, self.sigma = self._opts.lambda_, self._opts.fuse.sigma
        self.last_weight = None

    def _open(self, ctx, P):
        if self._cp is None:
            self._cp = self.channels
        return ctx.lib.of_consist_open(ctx.handle, C.byref(P), self.H, self.W, self.channels, self._cp,
                                       C.byref(self._opts))

    def push(self, frame, processed):
        """The next frame and its processed version.  Returns the consistent
        frame, float64 in the processed frames' shape."""
        self._live()
        _finite_frame("frames", frame, self.shape)
        p = _finite_frame("processed", processed, self.processed_shape)
        p32 = nat.f32(np.asarray(p, dtype=float))
        out = np.empty(self.processed_shape, dtype=np.float32)
        wgt = np.empty((self.H, self.W), dtype=np.float32)
        self._push(frame, nat.ptr(p32), nat.ptr(out), nat.ptr(wgt))
        self.last_weight = wgt.astype(np.float64)
        return out.astype(np.float64)


def consistent_frames(frames, processed, method='classic+nl-fast', sigma=None, lam=1.0, strength=4.0, patch=1,
                      alpha1=0.01, alpha2=0.5, cycles=_abi.CONSIST_CYCLES, sweeps=2, coarse_sweeps=32,
                      return_weight=False, params=None):
    """`processed`, a clip of (H, W) or (H, W, Cp) frames with Cp <= 4, made
    temporally consistent along the motion of `frames`, the original clip of as
    many (H, W) or (H, W, 3) frames: (T, H, W[, Cp]) float64, by a
    TemporalConsistency session over the clip.  With `return_weight` also the
    (T, H, W) float64 weights of the past (0 for the first frame)."""
    frames = _clip(frames)
    f0 = frames[0]
    if f0.size == 0 or not (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3)):
        raise ValueError(f"frames must be non-empty (H, W) or (H, W, 3) arrays, got {f0.shape}")
    frames = [_finite_frame("frames", f) for f in frames]
    H, W = f0.shape[:2]
    _frame_size(H, W)
    try:
        processed = _clip(processed)
    except ValueError:
        raise ValueError("processed must be a non-empty sequence of frames of one shape") from None
    if len(processed) != len(frames):
        raise ValueError(f"{len(frames)} frames but {len(processed)} processed frames")
    Cp = _channels("processed", processed[0], (H, W))[1]
    processed = [_finite_frame("processed", p) for p in processed]
    _consist_opts(sigma, lam, strength, patch, alpha1, alpha2, cycles, sweeps, coarse_sweeps)
    out = np.empty((len(frames),) + processed[0].shape, dtype=np.float64)
    wgt = np.empty((len(frames), H, W), dtype=np.float64)
    with TemporalConsistency(f0.shape, Cp, method, params, sigma, lam, strength, patch, alpha1, alpha2, cycles, sweeps,
                             coarse_sweeps) as tc:
        for t, (f, p) in enumerate(zip(frames, processed)):
            out[t] = tc.push(f, p)
            wgt[t] = tc.last_weight
    return (out, wgt) if return_weight else out
