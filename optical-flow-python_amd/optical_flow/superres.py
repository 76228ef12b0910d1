"""Multi-frame super-resolution along the flow: a frame and its neighbours in
time are resampled onto a grid `factor` times finer, every neighbour's pixels
placed where its flow says they belong and weighted as fuse_frames weights
them, so the sub-pixel phases between the frames add detail.
include/optflow.h ("Multi-frame super-resolution along the flow") states the
arithmetic; in a session the frames, flows and masks stay on the GPU
(of_sr_*), only the enlarged frames come back.

The upscale factor is `factor`; `scale` means flow reduction in this package.
`sigma` has to cover the aliasing between the frames as well as the noise: a
neighbour whose warped patch differs from the frame's by more than sigma
explains gets no weight, and the result is then the single-frame one.  `reach`
0.75 was the best of {0.6, 0.75, 1.0, 1.5} in a numpy prototype on one texture,
not a measured optimum."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import DelayedSession, _int_in, _number
from optical_flow.temporal import _fuse_inputs


def _sr_opts(factor, sigma, radius=1, strength=4.0, patch=2, reach=0.75, back=0.0, alpha1=0.01, alpha2=0.5):
    """of_sr_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    if sigma is None:
        raise ValueError("sigma (what the frames may differ by where they show the same surface: the noise and the "
                         "aliasing between them, in image units) is required")
    reach = _number("reach", reach, True)
    back = _number("back", back, False)
    if not _abi.SR_MIN_REACH <= reach <= _abi.SR_MAX_REACH:
        raise ValueError(f"reach must be in {_abi.SR_MIN_REACH}..{_abi.SR_MAX_REACH}, got {reach!r}")
    if back > 1.0:
        raise ValueError(f"back must be in 0..1, got {back!r}")
    return _abi.OfSrOpts(_int_in("factor", factor, _abi.SR_MIN_FACTOR, _abi.SR_MAX_FACTOR),
                         _int_in("radius", radius, 1, _abi.FUSE_MAX_RADIUS),
                         _int_in("patch", patch, 0, _abi.FUSE_MAX_PATCH), 0, _number("sigma", sigma, True),
                         _number("strength", strength, True), reach, back, _number("alpha1", alpha1, False),
                         _number("alpha2", alpha2, False))


def _out_size(H, W, s):
    if s * s * H * W >= 1 << 31:
        raise ValueError(f"the enlarged frame must stay below 2^31 pixels, got {s * H} x {s * W}")


def super_resolve(center, neighbours, flows, factor, sigma=None, states=None, strength=4.0, patch=2, reach=0.75,
                  back=0.0, return_support=False):
    """`center`, (H, W) or (H, W, C) with C <= 4, enlarged `factor` (2..4)
    times with the help of 0..8 `neighbours` of the same shape along `flows`
    (one (H, W, 2) flow centre -> neighbour each, in the frames' own pixels)
    and, optionally, their forward-backward masks `states`: returns the
    (factor H, factor W[, C]) float64 frame; with `return_support` also the
    (factor H, factor W) float64 weight every output pixel rests on.

    Every output pixel averages the pixels of the centre frame and of the
    neighbours that land within `reach` (0.75..1.5) low-resolution pixels of
    it, closer ones counting more; a neighbour counts with its fuse_weights
    weight (`sigma`, `strength`, `patch`) at the low-resolution pixel the
    output pixel lies in.  `back` (0..1) adds one back-projection step: the
    difference between `center` and the box reduction of the result
    (reduce_frame) is added back, `back` = 1 in full, which sharpens a clean
    frame and brings the noise of a noisy one back (of_super_resolve).
    `sigma` is required."""
    H, W, Cc, n, c32, n32, f32, st = _fuse_inputs(center, neighbours, flows, states, 0)
    opts = _sr_opts(factor, sigma, 1, strength, patch, reach, back)
    s = opts.factor
    _out_size(H, W, s)
    out = np.empty((s * H, s * W) + c32.shape[2:], dtype=np.float32)
    sup = np.empty((s * H, s * W), dtype=np.float32) if return_support else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_super_resolve(ctx.handle, nat.ptr(c32), H, W, Cc, n, nat.ptr(n32), nat.ptr(f32),
                                       nat.u8ptr(st), C.byref(opts), nat.ptr(out), nat.ptr(sup)))
    out = out.astype(np.float64)
    return (out, sup.astype(np.float64)) if return_support else out


class SuperResolver(DelayedSession):
    """Super-resolver over frames of one shape, (H, W) or (H, W, 3): the last
    2 radius + 1 frames and both flows and masks of the pairs between them
    stay on the GPU (of_sr_open / _push / _flush), as in a TemporalDenoiser.

        with SuperResolver(frames[0].shape, factor=2, sigma=8.0) as sr:
            for f in frames:
                r = sr.push(f)          # None for the first `radius` frames,
                ...                     # then (index, enlarged frame)
            for index, frame in sr.flush():
                ...                     # the last `radius` frames

    Frame t is enlarged (super_resolve) with frames t - radius .. t + radius
    that exist, along the flows of estimate_flow_bidirectional on the adjacent
    pairs and their masks; two frames apart the flows are chained
    (compose_flows).  Frames come back as float64, (factor H, factor W[, 3]);
    `last_support` holds the support plane of the frame returned last.  One
    super-resolver per context, beside the other sessions.  `sigma` is
    required and is a number."""

    _PREFIX, _NAME, _KIND = "of_sr_", "super-resolver", None

    def __init__(self, shape, method='classic+nl-fast', params=None, factor=2, sigma=None, radius=2, strength=4.0,
                 patch=2, reach=0.75, back=0.0, alpha1=0.01, alpha2=0.5, context=None):
        def make_opts(H, W):
            opts = _sr_opts(factor, sigma, radius, strength, patch, reach, back, alpha1, alpha2)
            _out_size(H, W, opts.factor)
            return opts

        super().__init__(shape, method, params, make_opts, context)
        self.factor, self.radius = self._opts.factor, self._opts.radius
        self.out_shape = (self.factor * self.H, self.factor * self.W) + self.shape[2:]
        self.last_support = None

    def _step(self, call, *args):
        out = np.empty(self.out_shape, dtype=np.float32)
        sup = np.empty(self.out_shape[:2], dtype=np.float32)
        idx = np.full(1, -1, dtype=np.int32)
        call(*args, nat.ptr(out), nat.ptr(sup), nat.i32ptr(idx))
        if idx[0] < 0:
            return None
        self.last_support = sup.astype(np.float64)
        return int(idx[0]), out.astype(np.float64)

    def push(self, frame):
        """The next frame.  Returns (index, frame) of the enlarged frame that
        became complete, or None while fewer than radius + 1 frames have been
        pushed."""
        return self._step(self._push, frame)

    def _flush_step(self):
        return self._step(self._call, "flush")


def super_resolve_frames(frames, method='classic+nl-fast', factor=2, sigma=None, radius=2, strength=4.0, patch=2,
                         reach=0.75, back=0.0, alpha1=0.01, alpha2=0.5, params=None, return_support=False):
    """Enlarge `frames` (a sequence of at least one (H, W) or (H, W, 3) frame
    of one shape) with a SuperResolver: returns (T, factor H, factor W[, 3])
    float64; with `return_support` also the (T, factor H, factor W) float64
    support planes.  `sigma` is required."""
    out, sup = SuperResolver.run_clip(frames, "last_support", method, params, factor, sigma, radius, strength, patch,
                                      reach, back, alpha1, alpha2)
    return (out, sup) if return_support else out
