"""Mask propagation: a marked object followed through a clip.  The mask of the
previous frame is carried to the current one along the backward flow (current
-> previous); a pixel whose flow cannot be trusted (forward-backward state,
a non-finite flow, a flow that leaves the frame) is decided by a colour-guided
vote of its decided neighbours; a pixel with no decided neighbour stays
unmarked and comes back MASK_UNKNOWN; a small mode filter cleans the result
(advance_mask).  include/optflow.h ("Mask propagation") states the arithmetic;
in a session the previous frame and the mask stay on the GPU (of_masks_*).
propagate_masks followed by inpaint_frames removes an object from one drawn
mask.

Masks are (H, W) arrays of a bool or integer dtype, nonzero where a pixel is
marked; they come back as uint8 0 / 1.  Known limits: the vote needs colour
contrast between the object and its surroundings, and an object whose whole
area is untrusted in one pair is lost from then on; the labels are thresholded
at every step, so the outline drifts over long clips (re-anchor with another
keyframe); `smooth` 1 rounds corners (a 14 x 18 rectangle loses its 4 corner
pixels); one object per call; no `scale`, batch or stream variant."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import Session, _clip, _flow, _frame_size, _int_in, _number, _planar32, _state
from optical_flow.inpaint import _finite_frame, _mask

MASK_CARRIED, MASK_VOTED, MASK_UNKNOWN, MASK_GIVEN = (_abi.OF_MASK_CARRIED, _abi.OF_MASK_VOTED,
                                                      _abi.OF_MASK_UNKNOWN, _abi.OF_MASK_GIVEN)


def _mask_opts(vote_radius=8, vote_range=20.0, smooth=1, alpha1=0.01, alpha2=0.5):
    """of_mask_opts from the keyword arguments; ValueError for anything the
    library would refuse (ranges of include/optflow.h)."""
    return _abi.OfMaskOpts(_int_in("vote_radius", vote_radius, 1, _abi.MASK_MAX_VOTE_RADIUS),
                           _int_in("smooth", smooth, 0, _abi.MASK_MAX_SMOOTH), _number("vote_range", vote_range, True),
                           _number("alpha1", alpha1, False), _number("alpha2", alpha2, False))


def advance_mask(mask, frame, flow, state=None, vote_radius=8, vote_range=20.0, smooth=1, return_status=False):
    """The mask of the previous frame carried to the current frame `frame`
    ((H, W) or (H, W, C) with C <= 4, the vote's guide) along `flow`, the
    (H, W, 2) flow current -> previous: (H, W) uint8 0 / 1.  `state` is the
    forward-backward state of `flow` ((H, W) integers, nonzero = not trusted)
    or None.

    A pixel whose flow is finite, lands inside the frame and has state 0 takes
    the bilinear sample of the mask there, thresholded at 0.5 (MASK_CARRIED).
    Every other pixel is voted by the decided pixels within `vote_radius`
    (1..12), each weighted by (1 - z)^2 with z = the mean squared colour
    difference / vote_range^2 where z < 1, by their plain count where no
    neighbour is that close in colour (MASK_VOTED), and stays unmarked where
    there is none (MASK_UNKNOWN).  A mode filter of radius `smooth` (0..2)
    follows (of_mask_advance).  A guide value that is not finite gives its
    pixel weight 0.  With `return_status` also the (H, W) uint8 status plane."""
    m = _mask("mask", mask)
    H, W = m.shape
    _frame_size(H, W)
    g = np.asarray(frame)
    if g.dtype.kind not in "fiu" or g.ndim not in (2, 3) or g.shape[:2] != (H, W) or \
            (g.ndim == 3 and not 1 <= g.shape[2] <= _abi.MASK_MAX_CHANNELS):
        raise ValueError(f"frame must be a ({H}, {W}) or ({H}, {W}, C) array of numbers with C <= "
                         f"{_abi.MASK_MAX_CHANNELS}, got {g.dtype} {g.shape}")
    f = _flow("flow", flow, (H, W))
    s = _state("state", state, H, W)
    opts = _mask_opts(vote_radius, vote_range, smooth)
    with np.errstate(over='ignore'):
        g32 = nat.f32(np.asarray(g, dtype=float))
    f32 = _planar32(f)
    out = np.empty((H, W), dtype=np.uint8)
    status = np.empty((H, W), dtype=np.uint8) if return_status else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_mask_advance(ctx.handle, nat.u8ptr(m), nat.ptr(g32), H, W, 1 if g.ndim == 2 else g.shape[2],
                                      nat.ptr(f32), nat.u8ptr(s), C.byref(opts), nat.u8ptr(out), nat.u8ptr(status)))
    return (out, status) if return_status else out


class MaskPropagator(Session):
    """Mask propagator over frames of H x W with `channels` 1 ((H, W) frames)
    or 3 ((H, W, 3)): the previous frame and the current mask stay on the GPU
    (of_masks_open / _push / _close).

        with MaskPropagator(H, W, 3) as mp:
            m = mp.push(frames[0], drawn)   # a keyframe: comes back as drawn != 0
            for f in frames[1:]:
                m = mp.push(f)              # the mask followed into f

    A push with a mask stores it (the first frame, or a re-anchor later) and
    estimates nothing; a push without one estimates the pair (previous, this)
    in both directions (estimate_flow_bidirectional with `alpha1`, `alpha2`)
    and advances the stored mask along the backward flow (advance_mask with its
    state).  `last_status` holds the status plane of the mask returned last
    (MASK_GIVEN everywhere after a keyframe).  One mask propagator per context,
    beside the other sessions."""

    _PREFIX, _NAME, _KIND = "of_masks_", "mask propagator", None

    def __init__(self, H, W, channels=3, method='classic+nl-fast', params=None, vote_radius=8, vote_range=20.0,
                 smooth=1, alpha1=0.01, alpha2=0.5, context=None):
        for name, v in (("H", H), ("W", W)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if isinstance(channels, bool) or channels not in (1, 3):
            raise ValueError(f"channels must be 1 or 3, got {channels!r}")
        shape = (int(H), int(W)) if channels == 1 else (int(H), int(W), 3)
        super().__init__(shape, method, params,
                         lambda h, w: _mask_opts(vote_radius, vote_range, smooth, alpha1, alpha2), context)
        self.vote_radius, self.vote_range, self.smooth = self._opts.vote_radius, self._opts.range, self._opts.smooth
        self.last_status = None

    def push(self, frame, mask=None):
        """The next frame, with its mask when it is a keyframe.  Returns the
        frame's mask, (H, W) uint8 0 / 1."""
        self._live()
        _finite_frame("frames", frame, self.shape)
        m = None if mask is None else _mask("mask", mask, (self.H, self.W))
        if m is None and self.frames == 0:
            raise ValueError("the first push of the mask propagator takes a mask")
        out = np.empty((self.H, self.W), dtype=np.uint8)
        status = np.empty((self.H, self.W), dtype=np.uint8)
        self._push(frame, nat.u8ptr(m), nat.u8ptr(out), nat.u8ptr(status))
        self.last_status = status
        return out


def _keyframe_runs(T, keys):
    """The runs that give every frame of 0 .. T-1 its mask from the nearest of
    the keyframes `keys` (sorted, distinct), a tie going to the earlier one: a
    list of lists of frame indices, each starting at its keyframe and running
    forward (ascending) or backward (descending) from it; a keyframe no other
    frame takes its mask from stands alone in its list."""
    runs = []
    for n, k in enumerate(keys):
        lo = 0 if n == 0 else (keys[n - 1] + k) // 2 + 1          # the earlier keyframe keeps the tie
        hi = T - 1 if n == len(keys) - 1 else (k + keys[n + 1]) // 2
        if hi > k:
            runs.append(list(range(k, hi + 1)))
        if lo < k:
            runs.append(list(range(k, lo - 1, -1)))
        if lo == k == hi:
            runs.append([k])
    return runs


def propagate_masks(frames, keyframes, method='classic+nl-fast', vote_radius=8, vote_range=20.0, smooth=1,
                    alpha1=0.01, alpha2=0.5, return_status=False, params=None):
    """A mask for every frame of `frames` (a sequence of at least one (H, W) or
    (H, W, 3) frame of one shape) from the masks drawn on a few of them:
    (T, H, W) uint8 0 / 1, as inpaint_frames takes it.  `keyframes` is a dict
    {frame index: mask}, or a single mask, meaning {0: mask}.

    Frame t takes its mask from the nearest keyframe, the earlier one on a tie:
    propagated forward when the keyframe lies before t, and backward, by a
    MaskPropagator over the frames in reverse order from the keyframe, when it
    lies after t.  The runs are sequential, one session each.  With
    `return_status` also the (T, H, W) uint8 status planes (MASK_GIVEN on the
    keyframes)."""
    frames = _clip(frames)
    f0 = frames[0]
    if f0.size == 0 or not (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3)):
        raise ValueError(f"frames must be non-empty (H, W) or (H, W, 3) arrays, got {f0.shape}")
    frames = [_finite_frame("frames", f) for f in frames]
    H, W = f0.shape[:2]
    _frame_size(H, W)
    T = len(frames)
    if not isinstance(keyframes, dict):
        keyframes = {0: keyframes}
    if not keyframes:
        raise ValueError("keyframes must hold at least one mask")
    given = {_int_in("a keyframe's index", k, 0, T - 1): _mask(f"keyframes[{k}]", m, (H, W))
             for k, m in keyframes.items()}
    _mask_opts(vote_radius, vote_range, smooth, alpha1, alpha2)
    out = np.empty((T, H, W), dtype=np.uint8)
    status = np.empty((T, H, W), dtype=np.uint8)
    for run in _keyframe_runs(T, sorted(given)):
        with MaskPropagator(H, W, 1 if f0.ndim == 2 else 3, method, params, vote_radius, vote_range, smooth, alpha1,
                            alpha2) as mp:
            for n, t in enumerate(run):
                out[t] = mp.push(frames[t], given[t] if n == 0 else None)
                status[t] = mp.last_status
    return (out, status) if return_status else out
