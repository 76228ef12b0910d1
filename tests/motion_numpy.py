"""numpy float64 restatement of the global motion estimation and the
stabiliser (include/optflow.h, "Global motion estimation and video
stabilisation"): the fixed-order sums, the robust fit, both warps' sampling
and the path smoothing, operation for operation, in the order the header
writes them.  Plain numpy and Python floats, no library.  Test helper, not a
conftest."""
import math
from types import SimpleNamespace

import numpy as np

from fuse_numpy import bil
from track_numpy import inside

TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
MODELS = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE}
I6 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ---- the order of every sum ---------------------------------------------------
def tree64(s):
    """The halving tree over the last axis (64 long): s[l] = s[l] + s[l + d]
    for l < d, d = 32 .. 1; returns s[..., 0]."""
    s = np.array(s, dtype=np.float64)
    d = 32
    while d >= 1:
        s[..., :d] = s[..., :d] + s[..., d:2 * d]
        d //= 2
    return s[..., 0]


def group_tree(v):
    """Values in order, zero-padded to a multiple of 64, every group of 64
    reduced by the tree; repeated until one value is left."""
    v = np.asarray(v, dtype=np.float64).ravel()
    while v.size > 1:
        pad = np.zeros(-(-v.size // 64) * 64)
        pad[:v.size] = v
        v = tree64(pad.reshape(-1, 64))
    return float(v[0])


def tile_values(a):
    """The 8 x 64 tiles of an (H, W) plane in row-major tile order: each
    column adds its 8 rows ascending from +0.0 (positions outside the plane
    are +0.0), the 64 columns go through the tree."""
    H, W = a.shape
    nty, ntx = -(-H // 8), -(-W // 64)
    p = np.zeros((nty * 8, ntx * 64))
    p[:H, :W] = a
    p = p.reshape(nty, 8, ntx, 64)
    acc = np.zeros((nty, ntx, 64))
    for r in range(8):
        acc = acc + p[:, r]
    return tree64(acc).ravel()


def ordered_sum(a):
    return group_tree(tile_values(a))


# ---- the fit --------------------------------------------------------------------
def frame_coords(H, W):
    s, cx, cy = 0.5 * max(H, W), 0.5 * (W - 1), 0.5 * (H - 1)
    ii, jj = np.mgrid[0:H, 0:W]
    return s, cx, cy, (jj - cx) / s, (ii - cy) / s


def matrix_of(th, H, W):
    s, cx, cy = 0.5 * max(H, W), 0.5 * (W - 1), 0.5 * (H - 1)
    return np.array([[1.0 + th[1] / s, th[2] / s, th[0] - (th[1] * cx + th[2] * cy) / s],
                     [th[4] / s, 1.0 + th[5] / s, th[3] - (th[4] * cx + th[5] * cy) / s]])


def _div(a, b):
    """IEEE division of two Python floats (no ZeroDivisionError)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def solve(S, model):
    """(th, lost_rank) of one pass from its 13 sums; Sw > 0."""
    Sw, Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv, _ = S
    th = [_div(Su, Sw), 0.0, 0.0, _div(Sv, Sw), 0.0, 0.0]
    with np.errstate(all="ignore"):
        if model == SIMILARITY:
            q = Sxx + Syy
            D = q - _div(Sx * Sx + Sy * Sy, Sw)
            if not D > 1e-9 * Sw:
                return th, True
            a = _div((Sxu + Syv) - _div(Sx * Su + Sy * Sv, Sw), D)
            b = _div((Sxv - Syu) - _div(Sx * Sv - Sy * Su, Sw), D)
            return [_div(Su - a * Sx + b * Sy, Sw), a, -b, _div(Sv - b * Sx - a * Sy, Sw), b, a], False
        if model == AFFINE:
            m, n = _div(Sx, Sw), _div(Sy, Sw)
            A, B, Cc = Sxx - m * Sx, Sxy - m * Sy, Syy - n * Sy
            l = _div(B, A)
            E = Cc - l * B
            if not A > 1e-9 * Sw or not E > 1e-9 * Sw:
                return th, True
            th = []
            for Sf, Sxf, Syf in ((Su, Sxu, Syu), (Sv, Sxv, Syv)):
                gx, gy = Sxf - m * Sf, Syf - n * Sf
                p2 = _div(gy - l * gx, E)
                p1 = _div(gx - B * p2, A)
                th += [_div(Sf - Sx * p1 - Sy * p2, Sw), p1, p2]
            return th, False
    return th, False


def fit(flow, model="affine", weight=None, state=None, iters=10, kappa=2.0, decay=0.5, c_min=0.5):
    """of_fit_motion.  Returns a namespace: theta (6,), matrix (2, 3), cutoff,
    support, rms, passes, degenerate, inliers (H, W) float32, masked (H, W)
    bool (w0 forced to 0)."""
    model = MODELS.get(model, model)
    f = np.asarray(flow).astype(np.float32)
    H, W = f.shape[:2]
    ok = np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
    if state is not None:
        ok &= np.asarray(state) == 0
    u = np.where(ok, f[..., 0], np.float32(0)).astype(np.float64)
    v = np.where(ok, f[..., 1], np.float32(0)).astype(np.float64)
    w0 = np.ones((H, W)) if weight is None else np.asarray(weight).astype(np.float32).astype(np.float64)
    w0 = np.where(ok, w0, 0.0)
    s, cx, cy, x, y = frame_coords(H, W)
    cmin2 = c_min * c_min
    kappa2 = kappa * kappa

    def one_pass(th, c2, first):
        with np.errstate(all="ignore"):
            uh = th[0] + th[1] * x + th[2] * y
            vh = th[3] + th[4] * x + th[5] * y
            ru, rv = u - uh, v - vh
            r2 = ru * ru + rv * rv
            if first:
                w = w0
            else:
                z = r2 / c2
                t = np.where(z < 1.0, z, 1.0)
                w = w0 * ((1.0 - t) * (1.0 - t))
            wx, wy = w * x, w * y
            planes = (w, wx, wy, wx * x, wx * y, wy * y, w * u, wx * u, wy * u, w * v, wx * v, wy * v, w * r2)
            return [ordered_sum(p) for p in planes], w

    th, c2 = [0.0] * 6, cmin2
    passes = degenerate = 0
    for k in range(iters + 1):
        S, _ = one_pass(th, c2, k == 0)
        passes += 1
        if not S[0] > 0.0:
            degenerate |= 2
            break
        th, lost = solve(S, model)
        degenerate |= int(lost)
        with np.errstate(all="ignore"):
            c = kappa2 * _div(S[12], S[0]) if k == 0 else c2 * decay
        c2 = c if c > cmin2 else cmin2
    S, w = one_pass(th, c2, False)
    with np.errstate(all="ignore"):
        rms = float(np.sqrt(np.float64(_div(S[12], S[0]))))
    return SimpleNamespace(theta=np.array(th, dtype=np.float64), matrix=matrix_of(th, H, W), cutoff=math.sqrt(c2),
                           support=S[0], rms=rms, passes=passes, degenerate=degenerate,
                           inliers=w.astype(np.float32), masked=~ok)


# ---- the affine warp ---------------------------------------------------------------
def warp_affine(im, A):
    """of_warp_affine: (out float32 in im's shape, valid (H, W) uint8)."""
    I = np.asarray(im).astype(np.float32).astype(np.float64)
    H, W = I.shape[:2]
    A = np.asarray(A, dtype=np.float64).ravel()
    ii, jj = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        q = (A[0] * jj + A[1] * ii) + A[2]
        r = (A[3] * jj + A[4] * ii) + A[5]
        ok = np.isfinite(q) & np.isfinite(r) & inside(r, q, H, W)
    smp = bil(I, np.where(ok, r, 0.0), np.where(ok, q, 0.0))
    out = np.where(ok if I.ndim == 2 else ok[..., None], smp, 0.0).astype(np.float32)
    return out, ok.astype(np.uint8)


# ---- path smoothing -------------------------------------------------------------------
def invertible(m):
    m = [float(e) for e in np.asarray(m).ravel()]
    if not all(math.isfinite(e) for e in m):
        return False
    return abs(m[0] * m[4] - m[1] * m[3]) >= 1e-12


def inv(m):
    a, b, tx, c, d, ty = [float(e) for e in np.asarray(m).ravel()]
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return (ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty))


def compose(X, Y):
    """X o Y: Y first."""
    x = [float(e) for e in np.asarray(X).ravel()]
    y = [float(e) for e in np.asarray(Y).ravel()]
    return (x[0] * y[0] + x[1] * y[3], x[0] * y[1] + x[1] * y[4], (x[0] * y[2] + x[1] * y[5]) + x[2],
            x[3] * y[0] + x[4] * y[3], x[3] * y[1] + x[4] * y[4], (x[3] * y[2] + x[4] * y[5]) + x[5])


def keep(m):
    """(the motion as the session keeps it, 4 if it was replaced else 0)."""
    return (tuple(float(e) for e in np.asarray(m).ravel()), 0) if invertible(m) else (I6, 4)


def smooth(motions, t, frames, radius, sigma_t):
    """S_t, (2, 3): motions[k] links frames k and k + 1 (invertible, as kept),
    `frames` = the frames of the clip so far."""
    two_s2 = (2.0 * sigma_t) * sigma_t
    num, den = [0.0] * 6, 0.0

    def add(P, d):
        nonlocal den
        g = math.exp(-(float(d) * float(d)) / two_s2)
        for e in range(6):
            num[e] = num[e] + g * P[e]
        den = den + g

    back = fwd = I6
    add(I6, 0)
    for d in range(1, radius + 1):
        if t - d >= 0:
            back = compose(inv(motions[t - d]), back)
            add(back, d)
        if t + d <= frames - 1:
            fwd = compose(motions[t + d - 1], fwd)
            add(fwd, d)
    return np.array([e / den for e in num]).reshape(2, 3)


def session_schedule(n, radius):
    """[(out_index, frames pushed so far)] for n pushes, then the flush."""
    pushes = [(k - radius if k >= radius else -1, k + 1) for k in range(n)]
    first = max(n - radius, 0)
    return pushes, [(t, n) for t in range(first, n)]
