"""numpy float64 restatement of the multi-frame super-resolution
(include/optflow.h, "Multi-frame super-resolution along the flow"):
of_super_resolve operation for operation, in the order the header writes
them, vectorised over the output pixels (the frames and the 3 x 3 taps stay
loops: their order is part of the arithmetic), and the prototype scene the
tests measure it on.  Test helper, not a conftest."""
import numpy as np

import fuse_numpy as fn
import upsample_numpy as un
from track_numpy import inside


def _chan(a):
    a = np.asarray(a).astype(np.float32).astype(np.float64)
    return a[..., None] if a.ndim == 2 else a


def grid(H, W, s):
    """(r, q, ic, jc) of every output pixel, each (sH, sW)."""
    Y, X = np.mgrid[0:s * H, 0:s * W]
    return (Y - 0.5 * (s - 1)) / s, (X - 0.5 * (s - 1)) / s, Y // s, X // s


def _taps(acc, S, N, zr, zq, R, ok, rho2, seen=None):
    """One frame's 3 x 3 taps around (zr, zq) where `ok`, added to acc and S."""
    H, W = N.shape[:2]
    zr, zq = np.where(ok, zr, 0.0), np.where(ok, zq, 0.0)
    a0, b0 = np.floor(zr + 0.5).astype(np.int64), np.floor(zq + 0.5).astype(np.int64)
    for ta in (-1, 0, 1):
        a = a0 + ta
        for tb in (-1, 0, 1):
            b = b0 + tb
            inb = ok & (a >= 0) & (a < H) & (b >= 0) & (b < W)
            dy, dx = a - zr, b - zq
            x = (dy * dy + dx * dx) / rho2
            use = inb & (x < 1.0)
            K = (1.0 - x) * (1.0 - x)
            w = K * R
            v = N[np.clip(a, 0, H - 1), np.clip(b, 0, W - 1)]
            acc = np.where(use[..., None], acc + w[..., None] * v, acc)
            S = np.where(use, S + w, S)
            if seen is not None:
                seen |= {"edge"} if (ok & ~inb).any() else set()
                seen |= {"far"} if (inb & ~use).any() else set()
    return acc, S


def super_resolve(center, neighbours, flows, factor, sigma, states=None, strength=4.0, patch=2, reach=0.75, back=0.0,
                  weights=None, seen=None):
    """of_super_resolve: (out float32 (sH, sW[, C]), out_support float32
    (sH, sW)).  `weights` replaces of_fuse_weights' (n, H, W) planes (the tests'
    "every weight forced to 1"); `seen` (a set) collects which branches
    occurred: "zero" a frame skipped for R == 0, "left" a frame skipped for
    leaving the frame, "far" a tap skipped for x >= 1, "edge" a tap skipped at
    the frame's edge."""
    I = _chan(center)
    H, W, C = I.shape
    s = int(factor)
    n = len(neighbours)
    if weights is None and n:
        weights = [w.astype(np.float32) for _, _, w in fn.weights(center, neighbours, flows, sigma, states, strength,
                                                                  patch)]
    rho2 = reach * reach
    r, q, ic, jc = grid(H, W, s)
    acc, S = np.zeros((s * H, s * W, C)), np.zeros((s * H, s * W))
    always = np.ones((s * H, s * W), bool)
    acc, S = _taps(acc, S, I, r, q, np.ones((s * H, s * W)), always, rho2, seen)
    for k in range(n):
        R = np.asarray(weights[k]).astype(np.float32).astype(np.float64)[ic, jc]
        F = np.asarray(flows[k]).astype(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            u, v = fn.bil(F[..., 0], r, q), fn.bil(F[..., 1], r, q)
            zr, zq = r + v, q + u
            ok = (R != 0.0) & inside(zr, zq, H, W)
        if seen is not None:
            seen |= {"zero"} if (R == 0.0).any() else set()
            seen |= {"left"} if ((R != 0.0) & ~ok).any() else set()
        acc, S = _taps(acc, S, _chan(neighbours[k]), zr, zq, R, ok, rho2, seen)
    out = (acc / S[..., None]).astype(np.float32)
    if back > 0:
        L = _chan(un.reduce_frame(out, s))
        e = I - L
        out = (out.astype(np.float64) + back * e[ic, jc]).astype(np.float32)
    return out.reshape((s * H, s * W) + np.asarray(center).shape[2:]), S.astype(np.float32)


def bilinear_upsample(center, factor):
    """The bilinear upsample of one frame on the same output grid, float64."""
    I = _chan(center)
    r, q, _, _ = grid(I.shape[0], I.shape[1], factor)
    return fn.bil(I, r, q).reshape(r.shape + np.asarray(center).shape[2:])


# ---- the prototype scene ----------------------------------------------------
OFFSETS = [(1, 2), (-2, 1), (3, -1), (-1, -3)]  # (dy, dx) of the four neighbours in high-resolution pixels


def tex(s, y, x):
    return 128 + 60 * np.sin(0.37 * x + 0.21 * y + s) * np.cos(0.29 * y - 0.17 * x + 2 * s)


def scene(factor, noise=0.0, H=48, W=64, seed=5):
    """(truth (sH, sW) float64, centre, [4 neighbours], [4 known flows centre
    -> neighbour, (H, W, 2)]): tex(1, y, x) on the high-resolution grid, seen by
    a camera that box-integrates factor x factor pixels; neighbour k sees the
    scene moved by OFFSETS[k] high-resolution pixels.  Gaussian noise of
    `noise` from a fixed seed on every low-resolution frame."""
    s = factor
    Y, X = np.mgrid[0:s * H, 0:s * W].astype(np.float64)
    rng = np.random.default_rng(seed)

    def shot(dy, dx):
        lo = un.reduce_frame(tex(1, Y + dy, X + dx), s).astype(np.float64)
        return lo + rng.normal(0.0, noise, lo.shape) if noise > 0 else lo

    center = shot(0, 0)
    neigh = [shot(dy, dx) for dy, dx in OFFSETS]
    flows = []
    for dy, dx in OFFSETS:  # the point at (y, x) of the centre is at (y - dy/s, x - dx/s) of the neighbour
        f = np.empty((H, W, 2))
        f[..., 0], f[..., 1] = -dx / s, -dy / s
        flows.append(f)
    return tex(1, Y, X), center, neigh, flows


def interior_mse(out, truth, factor):
    b = 4 * factor
    return float(((np.asarray(out, dtype=np.float64) - truth) ** 2)[b:-b, b:-b].mean())
