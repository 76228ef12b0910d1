"""estimate_flow (reference: optical_flow/interface.py:11-141).

RGB -> gray (uint8 round trip) and RGB -> Lab (+ per-channel [0,255]
scaling) run on the GPU inside of_estimate_flow, followed by the whole
coarse-to-fine schedule; one C call per pair."""
import ctypes as C
from collections import namedtuple

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow.methods.base import progress_printer
from optical_flow._session import Closing, _flow_scale, method_params


def estimate_flow(im1, im2, method='classic+nl-fast', params=None, gt=None, data_weight=None, scale=1,
                  upsample_range=20.0):
    """Flow (H, W, 2) float64 from im1 to im2; (H, W) or (H, W, >=3) inputs.
    Prints what the reference's compute_flow prints.  `gt` (an extension:
    the reference's estimate_flow has no such argument) is handed to the
    per-GNC-stage report as compute_flow(init, gt) would get it.

    `data_weight` (an extension too): an (H, W) plane, finite and >= 0 (not
    limited to <= 1; a bool mask works), that multiplies the data term of
    every pixel of im1 (include/optflow.h, "Per-pixel data-term weights").
    Where it is 0 -- a dead sensor region, a letterbox bar, a burnt-in
    overlay, a masked boundary, pixels a forward-backward check flagged -- the
    pixel's brightness constancy is switched off and the smoothness term
    inpaints the flow from the surroundings; the coarse pyramid levels use
    the weight's own pyramid.  The masked pixels' content still enters the
    global min / max of the preprocessing and the blurred coarse frames, so
    fill them with plausible values rather than extremes.  None is the
    unweighted flow, bitwise.  A wrong shape or a NaN, Inf or negative value
    raises ValueError; a general spatial_filters list or 'classic-c-a' with a
    weight raises NotImplementedError.

    `scale` (an extension too) = 2..4 trades accuracy for speed: both frames
    are reduced by that integer factor (reduce_frame), the flow is estimated
    on the reduced pair, whose pyramid is as many levels shorter, and brought
    back to full size along im1's edges (upsample_flow with `upsample_range`
    as its `range`: on the frames' value scale, 20 for 0..255), all in one C
    call (of_estimate_flow_scaled).  1 is the full-resolution estimate, the
    same C call as without the keyword.  (H, W) and (H, W, >=3) frames only,
    and not together with `data_weight`: NotImplementedError."""
    up = _flow_scale(scale, upsample_range)
    im1 = np.asarray(im1, dtype=float)
    im2 = np.asarray(im2, dtype=float)
    ope, P = method_params(method, params)
    H, W = im1.shape[:2]
    wgt = nat.data_weight(data_weight, H, W)
    if up is not None and (wgt is not None or (im1.ndim == 3 and im1.shape[2] < 3)):
        raise NotImplementedError("scale > 1 takes (H, W) or (H, W, >=3) frames and no data_weight")
    if im1.ndim == 3 and im1.shape[2] < 3:
        # interface.py:47: channels are concatenated, no colour conversion
        ope.images = np.concatenate([im1, im2], axis=2)
        if ope.color_images is not None:
            ope.color_images = im1.copy()
        return ope.compute_flow(np.zeros((H, W, 2)), gt, data_weight=wgt)
    if im1.ndim == 3:
        a = nat.f32(im1[:, :, :3])
        b = nat.f32(im2[:, :, :3])
        Cc = 3
    else:
        a, b, Cc = nat.f32(im1), nat.f32(im2), 1
    out = np.empty((2, H, W), dtype=np.float32)
    st = _abi.OfStats()
    ctx = nat.context()
    fn, flags = progress_printer(ope, gt)  # the reference's compute_flow prints (interface.py:66)
    with ctx.progress(fn, flags):
        if up is None:
            ctx.check(ctx.lib.of_estimate_flow_weighted(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc, None,
                                                        nat.ptr(wgt), nat.ptr(out), C.byref(st)))
        else:
            ctx.check(ctx.lib.of_estimate_flow_scaled(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc,
                                                      C.byref(up), nat.ptr(out), C.byref(st)))
    ope.alpha = P.alpha
    ope.last_stats = st.as_dict()
    return nat.interleaved(out)

BidirectionalFlow = namedtuple('BidirectionalFlow', ['forward', 'backward', 'occ_forward', 'occ_backward'])


def estimate_flow_bidirectional(im1, im2, method='classic+nl-fast', params=None, alpha1=0.01, alpha2=0.5, scale=1,
                                upsample_range=20.0):
    """Flow im1 -> im2, flow im2 -> im1 and where each can be trusted.

    Returns BidirectionalFlow(forward, backward, occ_forward, occ_backward):
    the flows (H, W, 2) float64, equal to estimate_flow(im1, im2, method,
    params) and estimate_flow(im2, im1, method, params); the masks (H, W)
    uint8, equal to forward_backward_check(forward, backward, alpha1, alpha2)
    and the same with the flows exchanged (utils/occlusion.py: FB_CONSISTENT,
    FB_OCCLUDED, FB_OUT_OF_FRAME).  (H, W) and (H, W, >=3) frames take one C
    call (of_estimate_flow_bidir) that runs the gray conversion, the
    structure-texture split and the image pyramids once for both directions.

    `scale` = 2..4 estimates both flows on the frames reduced by that factor
    and upsamples each along its own first frame (im1 for forward, im2 for
    backward; `upsample_range` as upsample_flow's `range`); the masks are the
    check of the full-resolution flows (of_estimate_flow_bidir_scaled, one C
    call; see estimate_flow).  1 is the full-resolution estimate, the same C
    call as without the keyword."""
    up = _flow_scale(scale, upsample_range)
    im1 = np.asarray(im1, dtype=float)
    im2 = np.asarray(im2, dtype=float)
    if im1.shape != im2.shape or im1.ndim not in (2, 3):
        raise ValueError(f"frames must share one (H, W) or (H, W, C) shape, got {im1.shape} / {im2.shape}")
    H, W = im1.shape[:2]
    if up is not None and im1.ndim == 3 and im1.shape[2] < 3:
        raise NotImplementedError("scale > 1 takes (H, W) or (H, W, >=3) frames")
    if im1.ndim == 3 and im1.shape[2] < 3:
        # estimate_flow's compute_flow route (interface.py:47), once per direction
        from optical_flow.utils.occlusion import forward_backward_check
        fw = estimate_flow(im1, im2, method, params)
        bw = estimate_flow(im2, im1, method, params)
        return BidirectionalFlow(fw, bw, forward_backward_check(fw, bw, alpha1, alpha2),
                                 forward_backward_check(bw, fw, alpha1, alpha2))
    ope, P = method_params(method, params)
    if im1.ndim == 3:
        a, b, Cc = nat.f32(im1[:, :, :3]), nat.f32(im2[:, :, :3]), 3
    else:
        a, b, Cc = nat.f32(im1), nat.f32(im2), 1
    out_f = np.empty((2, H, W), dtype=np.float32)
    out_b = np.empty((2, H, W), dtype=np.float32)
    occ_f = np.empty((H, W), dtype=np.uint8)
    occ_b = np.empty((H, W), dtype=np.uint8)
    st_f, st_b = _abi.OfStats(), _abi.OfStats()
    ctx = nat.context()
    fn, flags = progress_printer(ope, None)
    with ctx.progress(fn, flags):
        if up is None:
            ctx.check(ctx.lib.of_estimate_flow_bidir(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc, None,
                                                     None, nat.ptr(out_f), nat.ptr(out_b), float(alpha1),
                                                     float(alpha2), nat.u8ptr(occ_f), nat.u8ptr(occ_b),
                                                     C.byref(st_f), C.byref(st_b)))
        else:
            ctx.check(ctx.lib.of_estimate_flow_bidir_scaled(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc,
                                                            C.byref(up), float(alpha1), float(alpha2),
                                                            nat.ptr(out_f), nat.ptr(out_b), nat.u8ptr(occ_f),
                                                            nat.u8ptr(occ_b), C.byref(st_f), C.byref(st_b)))
    return BidirectionalFlow(nat.interleaved(out_f), nat.interleaved(out_b), occ_f, occ_b)


# info byte of interpolate_frames (of_interp_frames, include/optflow.h)
INTERP_BLEND = 0
INTERP_FRAME1_ONLY = 1
INTERP_FRAME2_ONLY = 2
INTERP_NEITHER = 3
INTERP_FILLED = 4


def interpolate_frames(im1, im2, t=0.5, method='classic+nl-fast', params=None, flows=None, alpha1=0.01, alpha2=0.5,
                       return_info=False, scale=1, upsample_range=20.0):
    """The frame(s) at time(s) `t`, strictly between im1 (t = 0) and im2
    (t = 1), by occlusion-aware interpolation along the flows of both
    directions (Baker et al. 2011 sec. 3.3.2; include/optflow.h states the
    arithmetic).  A scalar `t` gives one float64 frame of im1's shape, a
    sequence a list of them.

    `flows` = (forward, backward), each (H, W, 2), or a BidirectionalFlow
    interpolates along flows you already have (of_interp_frames; frames of 1
    to 4 channels).  Without it the flows are estimated with `method` /
    `params` as estimate_flow_bidirectional does, and (H, W) and (H, W, 3)
    frames take one C call (of_estimate_interp) that keeps the frames, flows
    and forward-backward masks on the device; the frames equal those of
    estimate_flow_bidirectional followed by interpolate_frames(flows=...).
    alpha1 / alpha2 are the thresholds of forward_backward_check.

    With `return_info` the result is (frames, ut, info): per frame also the
    motion at time t, (H, W, 2) float64, and the (H, W) uint8 info byte
    (INTERP_BLEND, INTERP_FRAME1_ONLY, INTERP_FRAME2_ONLY or INTERP_NEITHER,
    plus INTERP_FILLED where the motion came from hole filling); estimated
    flows then make the round trip of estimate_flow_bidirectional.

    `scale` / `upsample_range` apply where the flows are estimated, as in
    estimate_flow_bidirectional, whose round trip the flows then make; with
    `flows` given a `scale` other than 1 is a ValueError."""
    up = _flow_scale(scale, upsample_range)
    if up is not None and flows is not None:
        raise ValueError("scale applies to estimated flows only: leave it at 1 when `flows` is given")
    im1 = np.asarray(im1, dtype=float)
    im2 = np.asarray(im2, dtype=float)
    if im1.shape != im2.shape or im1.ndim not in (2, 3) or im1.size == 0:
        raise ValueError(f"frames must share one non-empty (H, W) or (H, W, C) shape, got {im1.shape} / {im2.shape}")
    H, W = im1.shape[:2]
    Cc = im1.shape[2] if im1.ndim == 3 else 1
    if not 1 <= Cc <= 4:
        raise ValueError(f"frames must have 1 to 4 channels, got {Cc}")
    scalar = np.ndim(t) == 0
    ts = np.atleast_1d(np.asarray(t, dtype=np.float64))
    if ts.ndim != 1 or ts.size == 0 or not np.all(np.isfinite(ts) & (ts > 0) & (ts < 1)):
        raise ValueError(f"t must be one or more times strictly inside (0, 1), got {t!r}")
    ts = np.ascontiguousarray(ts)
    n = ts.size
    if flows is not None:
        fw, bw = (flows.forward, flows.backward) if isinstance(flows, BidirectionalFlow) else flows
        fw, bw = np.asarray(fw), np.asarray(bw)
        if fw.shape != (H, W, 2) or bw.shape != (H, W, 2):
            raise ValueError(f"flows must both be ({H}, {W}, 2), got {fw.shape} / {bw.shape}")
    elif return_info or (im1.ndim == 3 and Cc != 3) or up is not None:
        r = estimate_flow_bidirectional(im1, im2, method, params, alpha1, alpha2, scale, upsample_range)
        fw, bw = r.forward, r.backward
    a, b = nat.f32(im1), nat.f32(im2)
    out = np.empty((n, H, W, Cc), dtype=np.float32)
    ut = np.empty((n, 2, H, W), dtype=np.float32) if return_info else None
    info = np.empty((n, H, W), dtype=np.uint8) if return_info else None
    if flows is not None or return_info or (im1.ndim == 3 and Cc != 3) or up is not None:
        ctx = nat.context()
        ctx.check(ctx.lib.of_interp_frames(ctx.handle, nat.ptr(a), nat.ptr(b), H, W, Cc, nat.ptr(nat.planar(fw)),
                                           nat.ptr(nat.planar(bw)), float(alpha1), float(alpha2), n, nat.dptr(ts),
                                           nat.ptr(out), nat.ptr(ut), nat.u8ptr(info)))
    else:
        ope, P = method_params(method, params)
        st_f, st_b = _abi.OfStats(), _abi.OfStats()
        ctx = nat.context()
        fn, flags = progress_printer(ope, None)
        with ctx.progress(fn, flags):
            ctx.check(ctx.lib.of_estimate_interp(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc,
                                                 float(alpha1), float(alpha2), n, nat.dptr(ts), nat.ptr(out), None,
                                                 None, None, C.byref(st_f), C.byref(st_b)))
    frames = [out[k].reshape(im1.shape).astype(np.float64) for k in range(n)]
    if not return_info:
        return frames[0] if scalar else frames
    uts = [nat.interleaved(ut[k]) for k in range(n)]
    infos = [info[k] for k in range(n)]
    return (frames[0], uts[0], infos[0]) if scalar else (frames, uts, infos)


def _as_u8(im):
    a = np.asarray(im)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    f = np.asarray(a, dtype=float)
    if not (np.all(f == np.floor(f)) and f.min() >= 0 and f.max() <= 255):
        raise ValueError("estimate_flow_batch takes uint8 frames (or integer-valued 0..255)")
    return np.ascontiguousarray(f.astype(np.uint8))


def estimate_flow_batch(im1s, im2s, method='classic+nl-fast', params=None, lanes=4):
    """estimate_flow over a batch of uint8 frame pairs, host to host: one C
    call (of_pairs_run_host) keeps `lanes` pairs in flight on the GPU with
    their uploads and downloads overlapped.  Returns a list of (H, W, 2)
    float64 flows equal to [estimate_flow(a, b, method, params) ...]:
    bitwise with lanes=1 or below 2^20 px; at >= 2^20 px with lanes >= 2 the
    fine CG solves of two pairs run side by side in another block geometry
    and the flows differ by CG rounding only (include/optflow.h)."""
    a = [_as_u8(x) for x in im1s]
    b = [_as_u8(x) for x in im2s]
    if not a or len(a) != len(b):
        raise ValueError("im1s and im2s must be non-empty and of equal length")
    H, W = a[0].shape[:2]
    # every frame of both lists: (H, W) or (H, W, >=3), checked before the
    # [:, :, :3] slice (a 1- or 2-channel frame would otherwise pass as 3)
    for x in a + b:
        if not (x.ndim == 2 or (x.ndim == 3 and x.shape[2] >= 3)):
            raise ValueError("estimate_flow_batch takes (H, W) or (H, W, >=3) frames")
    Cc = 3 if a[0].ndim == 3 else 1
    want = (H, W, 3) if Cc == 3 else (H, W)
    a = [x[:, :, :3] if x.ndim == 3 else x for x in a]
    b = [x[:, :, :3] if x.ndim == 3 else x for x in b]
    for x in a + b:
        if x.shape != want:
            raise ValueError("all frames of a batch must share one shape")
    a = [np.ascontiguousarray(x) for x in a]
    b = [np.ascontiguousarray(x) for x in b]
    P = method_params(method, params)[1]
    n = len(a)
    outs = [np.empty((2, H, W), dtype=np.float32) for _ in range(n)]
    vp = C.c_void_p
    p1 = (vp * n)(*[x.ctypes.data for x in a])
    p2 = (vp * n)(*[x.ctypes.data for x in b])
    po = (vp * n)(*[o.ctypes.data for o in outs])
    ctx = nat.context()
    ctx.check(ctx.lib.of_pairs_run_host(ctx.handle, n, p1, p2, H, W, Cc, C.byref(P), int(lanes), po, None))
    return [nat.interleaved(o) for o in outs]


class PairStream(Closing):
    """Streaming estimate_flow over uint8 frame pairs of one shape: a pool of
    `lanes` GPU pipelines (of_pairs_open, include/optflow.h) on a context of
    its own takes pairs as they are submitted, so host work between
    submissions (decoding, writing) never drains the GPU.  Flows equal
    estimate_flow_batch(..., lanes=lanes) bitwise.

        with PairStream(H, W, 3, 'classic+nl-fast') as s:
            t = s.submit(im1, im2)      # returns at once
            uv = s.wait(t)              # (H, W, 2) float64
    """

    def __init__(self, H, W, channels=3, method='classic+nl-fast', params=None, lanes=4, device=0):
        if channels not in (1, 3):
            raise ValueError("channels must be 1 (gray) or 3 (RGB)")
        P = method_params(method, params)[1]
        self.shape = (H, W, 3) if channels == 3 else (H, W)
        self.H, self.W, self.channels = H, W, channels
        self._ctx = nat.Context(device)
        self._live = {}
        try:
            self._ctx.check(self._ctx.lib.of_pairs_open(self._ctx.handle, H, W, channels, C.byref(P), int(lanes)))
        except Exception:
            self._ctx.close()
            raise

    def submit(self, im1, im2):
        """Queue one pair; returns its ticket.  The frames are copied into the
        stream's pinned buffers by a lane thread later, so they are kept
        referenced here until wait()."""
        a = _as_u8(im1)
        b = _as_u8(im2)
        if a.ndim == 3:
            a, b = np.ascontiguousarray(a[:, :, :3]), np.ascontiguousarray(b[:, :, :3])
        if a.shape != self.shape or b.shape != self.shape:
            raise ValueError(f"frames must be {self.shape}, got {a.shape} / {b.shape}")
        out = np.empty((2, self.H, self.W), dtype=np.float32)
        vp = C.c_void_p
        t = C.c_int64(0)
        self._ctx.check(self._ctx.lib.of_pairs_submit(self._ctx.handle, 1, (vp * 1)(a.ctypes.data),
                                                      (vp * 1)(b.ctypes.data), (vp * 1)(out.ctypes.data),
                                                      C.byref(t)))
        self._live[t.value] = (a, b, out)
        return t.value

    def wait(self, ticket, planar=False):
        """Block until the pair's flow is ready; (H, W, 2) float64, or with
        `planar` the library's (2, H, W) float32 planes as they came back (the
        conversion can then run on another thread)."""
        if ticket not in self._live:
            raise ValueError(f"unknown or already waited ticket {ticket}")
        self._ctx.check(self._ctx.lib.of_pairs_wait(self._ctx.handle, int(ticket)))
        out = self._live.pop(ticket)[2]
        return out if planar else nat.interleaved(out)

    def close(self):
        if self._ctx is not None:
            try:
                self._ctx.check(self._ctx.lib.of_pairs_close(self._ctx.handle))
            finally:
                self._ctx.close()
                self._ctx = None
                self._live.clear()


def _preprocess(im1, im2):
    a = nat.f32(np.asarray(im1, dtype=float)[:, :, :3])
    b = nat.f32(np.asarray(im2, dtype=float)[:, :, :3])
    H, W = a.shape[:2]
    gray = np.empty((2, H, W), dtype=np.float32)
    lab = np.empty((3, H, W), dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_preprocess(ctx.handle, nat.ptr(a), nat.ptr(b), H, W, nat.ptr(gray), nat.ptr(lab)))
    return gray, lab


def _rgb2gray(im):
    """MATLAB double(rgb2gray(uint8(im))) on the GPU (interface.py:74-88)."""
    im = np.asarray(im, dtype=float)
    if im.ndim == 2:
        return im
    return _preprocess(im, im)[0][0].astype(float)


def _rgb2lab_scaled(im):
    """_rgb2lab (interface.py:91-141) followed by the per-channel scale_image
    to [0, 255] that estimate_flow applies (interface.py:58-61)."""
    return nat.interleaved(_preprocess(im, im)[1])
