"""Noise-level estimation: the standard deviation of additive Gaussian noise
in a frame, from the frame alone or, better, from a pair of frames and the
flow between them.  include/optflow.h ("Noise-level estimation") states the
arithmetic; both estimators run on the GPU (of_estimate_noise[_pair])."""
import collections
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow._session import _flow, _frame_size, _planar32, _state

NoiseEstimate = collections.namedtuple("NoiseEstimate", ["sigma", "per_channel", "used"])
NoiseEstimate.__doc__ = """estimate_noise's result: `sigma`, the noise standard deviation in image units pooled
over the channels (the root mean square of `per_channel`, a tuple of one float per channel), and `used`, the
number of samples behind each channel's figure (pixels of the pair estimator, 2 x 2 blocks of the single-frame
one).  With used == 0 every sigma is NaN."""


def _image(name, im, shape=None):
    im = np.asarray(im)
    if im.ndim not in (2, 3) or im.size == 0 or im.dtype.kind not in "fiu" \
            or (im.ndim == 3 and not 1 <= im.shape[2] <= _abi.NOISE_MAX_CHANNELS) \
            or (shape is not None and im.shape != shape):
        want = f"(H, W) or (H, W, C) with C <= {_abi.NOISE_MAX_CHANNELS}" if shape is None else f"{shape}"
        raise ValueError(f"{name} must be a non-empty {want} array of numbers, got {im.dtype} {im.shape}")
    return im


def estimate_noise(im, im2=None, flow=None, state=None):
    """The noise standard deviation of `im`, (H, W) or (H, W, C) with C <= 4,
    as a NoiseEstimate(sigma, per_channel, used), in the image's units.

    With `im` alone: the median absolute diagonal Haar detail of the frame's
    2 x 2 blocks (H, W >= 2).  Texture counts as noise: on a textured frame at
    low noise the figure is high, by a factor of two and more.

    With `im2` (of im's shape) and `flow` ((H, W, 2), im -> im2): the median
    absolute difference between a pixel and its bilinear sample in im2 where
    the flow lands, over the pixels whose flow is finite, stays in the frame
    and, with `state` (the flow's forward_backward_check mask, optional), is
    consistent.  The median ignores a minority of wrong flows, and each
    residual is scaled by the variance factor of its four interpolation
    weights, so the figure does not depend on the sub-pixel phase.  The
    sample interpolates the picture too: while the noise is below the
    picture's interpolation error (sigma 2 on a strongly textured frame moving
    by a fraction of a pixel read 2.2) the estimate is high.

    Pixels or blocks with a non-finite value are left out.  Exact: the median
    is selected, not approximated, and equals a numpy float64 restatement
    bitwise (of_estimate_noise, of_estimate_noise_pair)."""
    im = _image("im", im)
    H, W = im.shape[:2]
    Cc = 1 if im.ndim == 2 else im.shape[2]
    _frame_size(H, W)
    if (im2 is None) != (flow is None):
        raise ValueError("im2 and flow go together: give both (the pair estimator) or neither (the single frame)")
    if im2 is None:
        if state is not None:
            raise ValueError("state belongs to the pair estimator: give im2 and flow too")
        if H < 2 or W < 2:
            raise ValueError(f"the single-frame estimate takes H and W >= 2, got {H} x {W}")
    else:
        im2 = _image("im2", im2, im.shape)
        flow = _flow("flow", flow, (H, W))
        state = _state("state", state, H, W)
    est = _abi.OfNoiseEstimate()
    with np.errstate(over='ignore'):
        a = nat.f32(im)
        b = None if im2 is None else nat.f32(im2)
    ctx = nat.context()
    if im2 is None:
        ctx.check(ctx.lib.of_estimate_noise(ctx.handle, nat.ptr(a), H, W, Cc, C.byref(est)))
    else:
        ctx.check(ctx.lib.of_estimate_noise_pair(ctx.handle, nat.ptr(a), nat.ptr(b), H, W, Cc, nat.ptr(_planar32(flow)),
                                                 nat.u8ptr(state), C.byref(est)))
    return NoiseEstimate(est.sigma, tuple(est.sigma_c[c] for c in range(Cc)), int(est.n))
