"""Flow resampling on the GPU (reference: optical_flow/utils/warping.py:6-45)."""
import numpy as np

from optical_flow import _native as nat


def resample_flow(uv, target_sz, method='bilinear'):
    """Bilinear resize; BOTH components scale by the height ratio (warping.py:25-26)."""
    uv = np.asarray(uv, dtype=float)
    H, W = uv.shape[:2]
    nH, nW = int(target_sz[0]), int(target_sz[1])
    if (H, W) == (nH, nW):
        return uv.copy()
    out = np.empty((2, nH, nW), dtype=np.float32)
    ctx = nat.context()
    ctx.check(ctx.lib.of_resample_flow(ctx.handle, nat.ptr(nat.planar(uv)), H, W, nH, nW, nat.ptr(out)))
    return nat.interleaved(out)


def warp_image(im, uv):
    """`im` (H, W) or (H, W, C <= 4) sampled bilinearly at (x + u, y + v) for
    the flow `uv` (H, W, 2), coordinates clamped to the frame (of_warp_image,
    include/optflow.h).  Returns (warped, valid): the float64 image of im's
    shape and the (H, W) bool mask of the pixels whose sample point lies
    inside the frame; a NaN / Inf flow gives 0 and False."""
    im = np.asarray(im, dtype=float)
    uv = np.asarray(uv)
    if im.ndim not in (2, 3) or uv.shape != im.shape[:2] + (2,):
        raise ValueError(f"need an (H, W[, C]) image and an (H, W, 2) flow, got {im.shape} / {uv.shape}")
    H, W = im.shape[:2]
    Cc = im.shape[2] if im.ndim == 3 else 1
    if not 1 <= Cc <= 4 or H < 1 or W < 1:
        raise ValueError(f"warp_image takes non-empty images of 1 to 4 channels, got {im.shape}")
    a = nat.f32(im)
    out = np.empty((H, W, Cc), dtype=np.float32)
    valid = np.empty((H, W), dtype=np.uint8)
    ctx = nat.context()
    ctx.check(ctx.lib.of_warp_image(ctx.handle, nat.ptr(a), H, W, Cc, nat.ptr(nat.planar(uv)), nat.ptr(out),
                                    nat.u8ptr(valid)))
    return out.reshape(im.shape).astype(np.float64), valid.astype(bool)
