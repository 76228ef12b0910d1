"""Occlusion confidence on the GPU (reference: optical_flow/utils/occlusion.py:6-56)."""
import numpy as np

from optical_flow import _native as nat


def detect_occlusion(uv, images, sigma_d=0.3, sigma_i=20.0):
    """exp(-div^2/2sd^2) * exp(-|I2(x+u)-I1|^2/2si^2)."""
    if sigma_d != 0.3 or sigma_i != 20.0:
        raise NotImplementedError("detect_occlusion runs with the reference defaults sigma_d=0.3, sigma_i=20")
    uv = np.asarray(uv, dtype=float)
    images = np.asarray(images, dtype=float)
    H, W = uv.shape[:2]
    nc = images.shape[2] // 2
    out = np.empty((H, W), dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_detect_occlusion(ctx.handle, nat.ptr(nat.planar(uv)), nat.ptr(nat.planar(images)),
                                          H, W, nc, nat.ptr(out)))
    return out.astype(float)


def flow_update(uv, x, clip=True, images=None):
    """The update of an IRLS warp as one level runs it (of_flow_update):
    uv + clip(x, -1, 1) in float32 (clip=False: uv + x), and with `images`
    also detect_occlusion of that field from the same launch.  Returns uv1,
    or (uv1, occ) when images are given."""
    uv = np.asarray(uv, dtype=float)
    x = np.asarray(x, dtype=float)
    if uv.ndim != 3 or uv.shape[2] != 2 or x.shape != uv.shape:
        raise ValueError(f"uv and x must both be (H, W, 2), got {uv.shape} / {x.shape}")
    H, W = uv.shape[:2]
    out = np.empty((2, H, W), dtype=np.float32)
    occ, im, nc = None, None, 0
    if images is not None:
        images = np.asarray(images, dtype=float)
        if images.ndim != 3 or images.shape[:2] != (H, W) or images.shape[2] % 2:
            raise ValueError(f"images must be ({H}, {W}, 2*nc), got {images.shape}")
        im, nc = nat.planar(images), images.shape[2] // 2
        occ = np.empty((H, W), dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_flow_update(ctx.handle, nat.ptr(nat.planar(uv)), nat.ptr(nat.planar(x)), int(bool(clip)),
                                     nat.ptr(im), H, W, nc, nat.ptr(out), nat.ptr(occ)))
    uv1 = nat.interleaved(out)
    return uv1 if occ is None else (uv1, occ.astype(float))


# states of forward_backward_check (of_fb_consistency, include/optflow.h)
FB_CONSISTENT = 0
FB_OCCLUDED = 1
FB_OUT_OF_FRAME = 2


def forward_backward_check(fw, bw, alpha1=0.01, alpha2=0.5, return_error=False):
    """Where the flow `fw` (frame 1 -> 2) can be trusted, given `bw` (frame
    2 -> 1), both (H, W, 2): follow fw, sample bw there bilinearly and test
    |fw + bw|^2 <= alpha1 (|fw|^2 + |bw|^2) + alpha2 (Sundaram et al. 2010).
    Returns the (H, W) uint8 state: FB_CONSISTENT, FB_OCCLUDED (inconsistent
    or occluded) or FB_OUT_OF_FRAME (the target leaves the frame); with
    `return_error` also |fw + bw|^2 as (H, W) float32 (+inf out of frame).
    Swap the arguments for the backward mask."""
    fw = np.asarray(fw)
    bw = np.asarray(bw)
    if fw.ndim != 3 or fw.shape[2] != 2 or fw.shape != bw.shape:
        raise ValueError(f"flows must both be (H, W, 2), got {fw.shape} / {bw.shape}")
    H, W = fw.shape[:2]
    state = np.empty((H, W), dtype=np.uint8)
    err = np.empty((H, W), dtype=np.float32) if return_error else None
    ctx = nat.context()
    ctx.check(ctx.lib.of_fb_consistency(ctx.handle, nat.ptr(nat.planar(fw)), nat.ptr(nat.planar(bw)), H, W,
                                        float(alpha1), float(alpha2), nat.u8ptr(state), nat.ptr(err)))
    return (state, err) if return_error else state
