"""Reduced-resolution flow: the box reduction of a frame and the edge-aware
upsampling of a low-resolution flow along a full-resolution guide, the two
stages behind the `scale` keyword of estimate_flow, estimate_flow_bidirectional,
interpolate_frames and the sessions.  include/optflow.h ("Reduced-resolution
flow with edge-aware upsampling") states the arithmetic."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import _flow, _flow_scale, _frame_size, _planar32


def _low_shape(H, W, scale):
    return -(-H // scale), -(-W // scale)


def _stage_scale(scale, rng=20.0):
    """of_upsample_opts of a stage call: scale 2..4 (1 has nothing to do)."""
    up = _flow_scale(scale, rng, "range")
    if up is None:
        raise ValueError(f"scale must be an integer in {_abi.UPSAMPLE_MIN_SCALE}..{_abi.UPSAMPLE_MAX_SCALE}, got 1")
    return up


def _frame(name, im, shape=None):
    """A frame as (float32 contiguous, H, W, channels): (H, W) or (H, W, C), C <= 4."""
    im = np.asarray(im)
    if im.ndim not in (2, 3) or im.size == 0 or im.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be a non-empty (H, W) or (H, W, C) array of numbers, got {im.dtype} {im.shape}")
    Cc = 1 if im.ndim == 2 else im.shape[2]
    if not 1 <= Cc <= _abi.UPSAMPLE_MAX_CHANNELS:
        raise ValueError(f"{name} must have 1..{_abi.UPSAMPLE_MAX_CHANNELS} channels, got {Cc}")
    if shape is not None and im.shape != shape:
        raise ValueError(f"{name} must be {shape}, got {im.shape}")
    H, W = im.shape[:2]
    _frame_size(H, W)
    with np.errstate(over='ignore'):
        return nat.f32(np.asarray(im, dtype=float)), H, W, Cc


def reduce_frame(im, scale):
    """`im`, (H, W) or (H, W, C) with C <= 4, reduced by the integer `scale`
    (2..4): every output pixel is the mean of its scale x scale block, cut at
    the frame's edge, so the result is (ceil(H/scale), ceil(W/scale)[, C])
    float64 (of_reduce_frame)."""
    a, H, W, Cc = _frame("im", im)
    s = _stage_scale(scale).scale
    hs, ws = _low_shape(H, W, s)
    out = np.empty((hs, ws) + a.shape[2:], dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_reduce_frame(ctx.handle, nat.ptr(a), H, W, Cc, s, nat.ptr(out)))
    return out.astype(np.float64)


def upsample_flow(flow_lo, guide, scale, range=20.0, guide_lo=None, return_info=False):
    """The low-resolution flow `flow_lo`, (ceil(H/scale), ceil(W/scale), 2) in
    low-resolution pixels, brought to the size of `guide`, (H, W) or (H, W, C)
    with C <= 4, in full-resolution pixels: (H, W, 2) float64.  Every output
    pixel averages the 4 x 4 low-resolution neighbours around it, each weighted
    by its distance and by how much the guide at the pixel looks like the low
    guide at the neighbour, so motion boundaries follow the guide's edges
    instead of being smeared over `scale` pixels (of_flow_upsample).
    `guide_lo` is the low guide (default: reduce_frame(guide, scale)); low
    flows that are not finite are left out.

    `range` is the photometric difference (root mean square over the channels)
    at which a neighbour's weight reaches 0.  It is on the frames' own value
    scale, 20 for 0..255 frames, and scales with the value range like min_eig
    and noise_floor do (0..1 frames: 20 / 255).  The default is the best
    all-round value of a numpy prototype on synthetic two-layer scenes, not a
    measured optimum.

    With `return_info` also the (H, W) uint8 plane: 0 the edge-aware average,
    1 no neighbour looked like the pixel and the distance weights alone
    decided, 2 no neighbour had a finite flow (the flow is NaN there)."""
    g, H, W, Cc = _frame("guide", guide)
    up = _stage_scale(scale, range)
    hs, ws = _low_shape(H, W, up.scale)
    f = _flow("flow_lo", flow_lo, (hs, ws))
    if guide_lo is None:
        lo = nat.f32(reduce_frame(guide, up.scale))
    else:
        lo = _frame("guide_lo", guide_lo, (hs, ws) + g.shape[2:])[0]
    out = np.empty((2, H, W), dtype=np.float32)
    info = np.empty((H, W), dtype=np.uint8) if return_info else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_flow_upsample(ctx.handle, nat.ptr(_planar32(f)), nat.ptr(lo), nat.ptr(g), H, W, Cc,
                                       C.byref(up), nat.ptr(out), nat.u8ptr(info)))
    return (nat.interleaved(out), info) if return_info else nat.interleaved(out)
