"""numpy float64 restatement of the noise-level estimation (include/optflow.h,
"Noise-level estimation"): the keys of of_estimate_noise_pair and
of_estimate_noise operation for operation, in the order the header writes
them, the lower-median rule, and the automatic session's sigma rule built
from them.  Also a forward-backward test for flows made without a GPU.  Test
helper, not a conftest."""
import collections

import numpy as np

from fuse_numpy import _landing

Estimate = collections.namedtuple("Estimate", ["sigma", "per_channel", "used"])
MAD_TO_SIGMA = 0.6744897501960817  # the median of |N(0, 1)|


def _frame(im):
    a = np.asarray(im)
    with np.errstate(over="ignore"):
        a = a.astype(np.float32).astype(np.float64)
    return a[..., None] if a.ndim == 2 else a


def pair_keys(im1, im2, flow, state=None):
    """of_estimate_noise_pair's keys: (n, C) float32, the usable pixels in
    row-major order."""
    A, B = _frame(im1), _frame(im2)
    H, W, C = A.shape
    with np.errstate(over="ignore"):
        f32 = np.asarray(flow).astype(np.float32)
    _, _, r, q, ok = _landing(f32)
    if state is not None:
        ok = ok & (np.asarray(state) == 0)
    # bil's taps (r, q are 0 where the flow does not land inside)
    qc = np.minimum(np.maximum(q, 0.0), float(W - 1))
    rc = np.minimum(np.maximum(r, 0.0), float(H - 1))
    qf, rf = np.floor(qc), np.floor(rc)
    j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
    fc, fr = qc - qf, rc - rf
    j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
    a00, a01, a10, a11 = B[i0, j0], B[i0, j1], B[i1, j0], B[i1, j1]
    fin = np.isfinite(A) & np.isfinite(a00) & np.isfinite(a01) & np.isfinite(a10) & np.isfinite(a11)
    ok = ok & fin.all(-1)
    w00, w01 = (1.0 - fr) * (1.0 - fc), (1.0 - fr) * fc
    w10, w11 = fr * (1.0 - fc), fr * fc
    g = 1.0 + (((w00 * w00 + w01 * w01) + w10 * w10) + w11 * w11)
    fc3, fr3 = fc[..., None], fr[..., None]
    with np.errstate(all="ignore"):
        s = (1.0 - fr3) * ((1.0 - fc3) * a00 + fc3 * a01) + fr3 * ((1.0 - fc3) * a10 + fc3 * a11)
        e = A - s
        k = (e * e / g[..., None]).astype(np.float32)
    return k[ok]


def single_keys(im):
    """of_estimate_noise's keys: (n, C) float32, the usable 2 x 2 blocks in
    row-major order."""
    A = _frame(im)
    H, W, C = A.shape
    Hb, Wb = H // 2, W // 2
    a, b = A[0:2 * Hb:2, 0:2 * Wb:2], A[0:2 * Hb:2, 1:2 * Wb:2]
    p, q = A[1:2 * Hb:2, 0:2 * Wb:2], A[1:2 * Hb:2, 1:2 * Wb:2]
    ok = (np.isfinite(a) & np.isfinite(b) & np.isfinite(p) & np.isfinite(q)).all(-1)
    with np.errstate(all="ignore"):
        d = ((a - b) - (p - q)) / 2.0
        k = (d * d).astype(np.float32)
    return k[ok]


def lower_median(keys):
    """The key of rank (n - 1) // 2, 0-based, ascending, of a 1-D float32
    array of n >= 1 non-negative keys (+Inf allowed)."""
    k = np.sort(np.asarray(keys, dtype=np.float32))
    return k[(k.size - 1) // 2]


def from_keys(keys):
    """The estimate from (n, C) keys."""
    n, C = keys.shape
    if n == 0:
        return Estimate(float("nan"), (float("nan"),) * C, 0)
    per = [float(np.sqrt(np.float64(lower_median(keys[:, c]))) / MAD_TO_SIGMA) for c in range(C)]
    s = 0.0
    for x in per:
        s = s + x * x
    return Estimate(float(np.sqrt(s / C)), tuple(per), n)


def estimate_pair(im1, im2, flow, state=None):
    return from_keys(pair_keys(im1, im2, flow, state))


def estimate_single(im):
    return from_keys(single_keys(im))


def session_sigma(t, T, H, W, pair_estimates, single_fn, floor):
    """The sigma frame t of a T-frame clip is fused with in the automatic
    session: pair_estimates[j] of pair (j, j + 1), single_fn(t) the
    single-frame estimate of frame t, computed only where it is needed."""
    s, m = 0.0, 0
    for j in (t - 1, t):
        if j < 0 or j + 1 >= T:
            continue
        e = pair_estimates[j]
        if 4 * e.used < H * W:
            continue
        s = s + e.sigma * e.sigma
        m += 1
    if m > 0:
        sigma = float(np.sqrt(s / m))
    elif H >= 2 and W >= 2:
        sigma = single_fn(t).sigma
    else:
        sigma = floor
    return sigma if sigma >= floor else floor


def fb_state(fw, bw, alpha1=0.01, alpha2=0.5):
    """of_fb_consistency's state of fw given bw, both (H, W, 2)."""
    fw = np.asarray(fw).astype(np.float32)
    B = np.asarray(bw).astype(np.float32).astype(np.float64)
    H, W = fw.shape[:2]
    u, v, r, q, ok = _landing(fw)
    j0, i0 = np.floor(q).astype(np.int64), np.floor(r).astype(np.int64)
    fc, fr = q - np.floor(q), r - np.floor(r)
    j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
    with np.errstate(all="ignore"):
        def samp(P):
            return (1 - fr) * ((1 - fc) * P[i0, j0] + fc * P[i0, j1]) + fr * ((1 - fc) * P[i1, j0] + fc * P[i1, j1])
        bu, bv = samp(B[..., 0]), samp(B[..., 1])
        du, dv = u + bu, v + bv
        err = du * du + dv * dv
        thr = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2
        st = np.where(err > thr, 1, 0)
    return np.where(ok, st, 2).astype(np.uint8)
