"""Motion-compensated temporal denoising of a frame sequence: a frame is
averaged with its neighbours in time, each warped onto it along a flow and
weighted per pixel by how well its warped patch matches the frame's; what the
forward-backward masks, the frame border or the photometric difference say
does not match is left out.  include/optflow.h ("Motion-compensated temporal
denoising") states the arithmetic; in a session the frames, flows and masks
stay on the GPU (of_denoise_*), only the denoised frames come back.

Flows are (H, W, 2) with u along columns, as everywhere in the package; masks
are forward_backward_check's (0 consistent, 1 occluded, 2 out of frame)."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import DelayedSession, _flow, _frame_size, _int_in, _number, _planar32, _state


AUTO = "auto"  # sigma=AUTO: the session estimates the noise level itself (of_denoise_open_auto)


def _is_auto(sigma):
    return isinstance(sigma, str) and sigma == AUTO


def _fuse_opts(sigma, radius=1, strength=4.0, patch=2, alpha1=0.01, alpha2=0.5):
    """of_fuse_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    if sigma is None:
        raise ValueError("sigma (the noise standard deviation in image units, or 'auto' in a session) is required")
    return _abi.OfFuseOpts(_int_in("radius", radius, 1, _abi.FUSE_MAX_RADIUS),
                           _int_in("patch", patch, 0, _abi.FUSE_MAX_PATCH), _number("sigma", sigma, True),
                           _number("strength", strength, True), _number("alpha1", alpha1, False),
                           _number("alpha2", alpha2, False))


def compose_flows(f, g, state_f=None, state_g=None, return_state=False):
    """Chain the flow `f` (frame a -> b) with `g` (b -> c), both (H, W, 2):
    returns the flow a -> c, (H, W, 2) float64: f plus g sampled bilinearly
    where f lands.  Where f is not finite or leaves the frame the result is f
    itself.  With `return_state` also the (H, W) uint8 mask of the result: 2
    where f leaves the frame, else the larger of `state_f` at the pixel and
    `state_g` at the pixel nearest to where f lands (None: all consistent), in
    forward_backward_check's encoding (of_flow_compose)."""
    f = _flow("f", f)
    H, W = f.shape[:2]
    g = _flow("g", g, (H, W))
    _frame_size(H, W)
    sf, sg = _state("state_f", state_f, H, W), _state("state_g", state_g, H, W)
    out = np.empty((2, H, W), dtype=np.float32)
    so = np.empty((H, W), dtype=np.uint8) if return_state else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_flow_compose(ctx.handle, nat.ptr(_planar32(f)), nat.ptr(_planar32(g)), H, W, nat.u8ptr(sf),
                                      nat.u8ptr(sg), nat.ptr(out), nat.u8ptr(so)))
    return (nat.interleaved(out), so) if return_state else nat.interleaved(out)


def _frame_stack(center, neighbours, least=1):
    center = np.asarray(center)
    if center.ndim not in (2, 3) or center.size == 0 or center.dtype.kind not in "fiu":
        raise ValueError(f"center must be a non-empty (H, W) or (H, W, C) array of numbers, got {center.dtype} "
                         f"{center.shape}")
    Cc = 1 if center.ndim == 2 else center.shape[2]
    if not 1 <= Cc <= _abi.FUSE_MAX_CHANNELS:
        raise ValueError(f"frames must have 1..{_abi.FUSE_MAX_CHANNELS} channels, got {Cc}")
    neighbours = [np.asarray(x) for x in neighbours]
    if not least <= len(neighbours) <= _abi.FUSE_MAX_NEIGHBOURS:
        raise ValueError(f"{least}..{_abi.FUSE_MAX_NEIGHBOURS} neighbours, got {len(neighbours)}")
    for x in neighbours:
        if x.shape != center.shape or x.dtype.kind not in "fiu":
            raise ValueError(f"every neighbour must be a {center.shape} array of numbers, got {x.dtype} {x.shape}")
    return center, neighbours, Cc


def _fuse_inputs(center, neighbours, flows, states, least=1):
    """The arguments a fusion shares, validated and as the C entries take
    them: (H, W, channels, n, center, neighbours, flows, states), the arrays
    contiguous float32 / uint8, or None for what is absent."""
    center, neighbours, Cc = _frame_stack(center, neighbours, least)
    H, W = center.shape[:2]
    _frame_size(H, W)
    n = len(neighbours)
    flows = list(flows)
    if len(flows) != n:
        raise ValueError(f"{n} neighbours but {len(flows)} flows")
    flows = [_flow(f"flows[{k}]", f, (H, W)) for k, f in enumerate(flows)]
    st = None
    if states is not None:
        states = list(states)
        if len(states) != n:
            raise ValueError(f"{n} neighbours but {len(states)} states")
        if any(s is not None for s in states):
            st = np.zeros((n, H, W), dtype=np.uint8)
            for k, s in enumerate(states):
                if s is not None:
                    st[k] = _state(f"states[{k}]", s, H, W)
    c32 = nat.f32(np.asarray(center, dtype=float))
    n32 = nat.f32(np.stack([np.asarray(x, dtype=float) for x in neighbours])) if n else None
    f32 = np.ascontiguousarray(np.stack([_planar32(f) for f in flows])) if n else None
    return H, W, Cc, n, c32, n32, f32, st


def fuse_frames(center, neighbours, flows, sigma=None, states=None, strength=4.0, patch=2, return_weight=False):
    """`center`, (H, W) or (H, W, C) with C <= 4, fused with 1..8 `neighbours`
    of the same shape along `flows` (one (H, W, 2) flow centre -> neighbour
    each) and, optionally, their forward-backward masks `states` (None, or one
    (H, W) mask or None per neighbour): returns the fused frame, float64 in
    center's shape; with `return_weight` also the (H, W) float64 effective
    number of frames averaged per pixel, 1 .. len(neighbours) + 1.

    A neighbour counts at a pixel where its flow is finite, stays in the frame
    and its mask is 0; its weight is 1 while the mean squared difference of the
    (2 patch + 1)^2 window to the warped neighbour is at most 2 sigma^2 (what
    noise of standard deviation `sigma` explains) and falls to exactly 0 at
    2 sigma^2 + (strength sigma)^2 (of_fuse_frames).  `sigma` is required."""
    H, W, Cc, n, c32, n32, f32, st = _fuse_inputs(center, neighbours, flows, states)
    opts = _fuse_opts(sigma, 1, strength, patch)
    out = np.empty(c32.shape, dtype=np.float32)
    wgt = np.empty((H, W), dtype=np.float32) if return_weight else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_fuse_frames(ctx.handle, nat.ptr(c32), H, W, Cc, n, nat.ptr(n32), nat.ptr(f32), nat.u8ptr(st),
                                     C.byref(opts), nat.ptr(out), nat.ptr(wgt)))
    out = out.astype(np.float64)
    return (out, wgt.astype(np.float64)) if return_weight else out


def fuse_weights(center, neighbours, flows, sigma=None, states=None, strength=4.0, patch=2):
    """The weight every neighbour gets in fuse_frames with the same arguments:
    (n, H, W) float64 in 0..1, 0 where the neighbour does not count at the
    pixel (of_fuse_weights)."""
    H, W, Cc, n, c32, n32, f32, st = _fuse_inputs(center, neighbours, flows, states)
    opts = _fuse_opts(sigma, 1, strength, patch)
    wgt = np.empty((n, H, W), dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_fuse_weights(ctx.handle, nat.ptr(c32), H, W, Cc, n, nat.ptr(n32), nat.ptr(f32),
                                      nat.u8ptr(st), C.byref(opts), nat.ptr(wgt)))
    return wgt.astype(np.float64)


class TemporalDenoiser(DelayedSession):
    """Temporal denoiser over frames of one shape, (H, W) or (H, W, 3): the
    last 2 radius + 1 frames and both flows and masks of the pairs between
    them stay on the GPU (of_denoise_open / _push / _flush).

        with TemporalDenoiser(frames[0].shape, sigma=10.0) as dn:
            for f in frames:
                r = dn.push(f)          # None for the first `radius` frames,
                ...                     # then (index, frame) of frame index
            for index, frame in dn.flush():
                ...                     # the last `radius` frames

    Frame t is fused (fuse_frames) with frames t - radius .. t + radius that
    exist, along the flows of estimate_flow_bidirectional(frame k, frame k+1,
    method, params, alpha1, alpha2) on the adjacent pairs and their masks;
    two frames apart the flows are chained (compose_flows).  Frames come back
    as float64 in the input's shape; `last_weight` holds the (H, W) float64
    effective number of frames averaged in the frame returned last.  One
    denoiser per context: by default the calling thread's context (other
    calls of the package may run between pushes), or a `context`
    (_native.Context) of your own.

    `sigma` is required: the noise standard deviation in image units, or
    'auto'.  With 'auto' every frame is fused with a sigma of its own, the
    root mean square of estimate_noise(frame k, frame k+1, flow, mask) over
    its adjacent pairs (t-1, t) and (t, t+1) that rest on at least a quarter
    of the pixels, else estimate_noise(frame t), never below `noise_floor`
    (0.25 on a 0..255 scale, below the 1/sqrt(12) of 8-bit quantisation: scale
    it with your value range; of_denoise_open_auto).  `last_sigma` holds the
    sigma of the frame returned last, in either mode.

    `scale` = 2..4 estimates every pair's flows at 1/scale of the resolution
    and brings them back along the frames' edges, as estimate_flow_bidirectional
    with the same `scale` / `upsample_range` does (of_session_set_flow_scale);
    the fusion stays at full resolution.  1 is the full-resolution denoiser."""

    _PREFIX, _NAME, _KIND = "of_denoise_", "denoiser", _abi.OF_SESSION_DENOISE

    def __init__(self, shape, method='classic+nl-fast', params=None, sigma=None, radius=1, strength=4.0, patch=2,
                 alpha1=0.01, alpha2=0.5, context=None, noise_floor=0.25, scale=1, upsample_range=20.0):
        self._auto = _is_auto(sigma)
        self._floor = _number("noise_floor", noise_floor, True)
        fixed = self._floor if self._auto else sigma  # the automatic session does not read the field
        super().__init__(shape, method, params,
                         lambda H, W: _fuse_opts(fixed, radius, strength, patch, alpha1, alpha2), context, scale,
                         upsample_range)
        self.radius = self._opts.radius
        self.last_weight = None
        self.last_sigma = None

    def _open(self, ctx, P):
        if not self._auto:
            return super()._open(ctx, P)
        return ctx.lib.of_denoise_open_auto(ctx.handle, C.byref(P), self.H, self.W, self.channels,
                                            C.byref(self._opts), self._floor)

    def _step(self, call, *args):
        out = np.empty(self.shape, dtype=np.float32)
        wgt = np.empty((self.H, self.W), dtype=np.float32)
        idx = np.full(1, -1, dtype=np.int32)
        call(*args, nat.ptr(out), nat.ptr(wgt), nat.i32ptr(idx))
        if idx[0] < 0:
            return None
        self.last_weight = wgt.astype(np.float64)
        sigma = C.c_double(0.0)
        self._call("last_sigma", C.byref(sigma))
        self.last_sigma = sigma.value
        return int(idx[0]), out.astype(np.float64)

    def push(self, frame):
        """The next frame.  Returns (index, frame) of the denoised frame that
        became complete, float64 in the input's shape, or None while fewer
        than radius + 1 frames have been pushed."""
        return self._step(self._push, frame)

    def _flush_step(self):
        return self._step(self._call, "flush")


def denoise_frames(frames, method='classic+nl-fast', sigma=None, radius=1, strength=4.0, patch=2, alpha1=0.01,
                   alpha2=0.5, params=None, return_weight=False, noise_floor=0.25, return_sigma=False, scale=1,
                   upsample_range=20.0):
    """Denoise `frames` (a sequence of at least one (H, W) or (H, W, 3) frame
    of one shape) with a TemporalDenoiser: returns (T, H, W[, 3]) float64;
    with `return_weight` also the (T, H, W) float64 effective number of frames
    averaged per pixel, with `return_sigma` also the (T,) float64 sigma every
    frame was fused with, in that order.  `sigma` is required: a number, or
    'auto' with its `noise_floor`; `scale` / `upsample_range` estimate the
    flows at reduced resolution (TemporalDenoiser)."""
    out, (wgt, sig) = TemporalDenoiser.run_clip(frames, ("last_weight", "last_sigma"), method, params, sigma, radius,
                                                strength, patch, alpha1, alpha2, None, noise_floor, scale,
                                                upsample_range)
    res = (out,) + ((wgt,) if return_weight else ()) + ((sig,) if return_sigma else ())
    return res if len(res) > 1 else out
