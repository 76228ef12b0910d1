"""numpy float64 restatement of the reduced-resolution flow (include/optflow.h,
"Reduced-resolution flow with edge-aware upsampling"): of_reduce_frame and
of_flow_upsample operation for operation, in the order the header writes them,
vectorised over the pixels (the 16 taps stay a loop: their order is part of
the arithmetic).  Test helper, not a conftest."""
import numpy as np


def low_shape(H, W, s):
    return -(-H // s), -(-W // s)


def _chan(a):
    a = np.asarray(a).astype(np.float32).astype(np.float64)
    return a[..., None] if a.ndim == 2 else a


def reduce_frame(im, s):
    """of_reduce_frame: float32, (hs, ws) or (hs, ws, C) like im."""
    im = np.asarray(im)
    I = _chan(im)
    H, W, C = I.shape
    hs, ws = low_shape(H, W, s)
    aa, bb = np.mgrid[0:hs, 0:ws]
    S = np.zeros((hs, ws, C))
    m = np.zeros((hs, ws), dtype=np.int64)
    for di in range(s):          # row-major over the block, from +0.0
        for dj in range(s):
            i, j = aa * s + di, bb * s + dj
            ok = (i < H) & (j < W)
            v = I[np.minimum(i, H - 1), np.minimum(j, W - 1)]
            S = np.where(ok[..., None], S + v, S)
            m = m + ok
    out = (S / m[..., None]).astype(np.float32)
    return out.reshape((hs, ws) + im.shape[2:])


def upsample(flow_lo, guide_lo, guide, s, rng=20.0, spatial_only=False):
    """of_flow_upsample: (out (H, W, 2) float32, info (H, W) uint8).  flow_lo
    (hs, ws, 2), guide_lo (hs, ws[, C]), guide (H, W[, C]).  `spatial_only`
    drops the photometric weight (wr = 1): what plain spatial weights give."""
    f = np.asarray(flow_lo).astype(np.float32)
    L, G = _chan(guide_lo), _chan(guide)
    H, W, C = G.shape
    hs, ws = low_shape(H, W, s)
    assert f.shape == (hs, ws, 2) and L.shape == (hs, ws, C)
    h2 = rng * rng
    ii, jj = np.mgrid[0:H, 0:W]
    r = (ii - 0.5 * (s - 1)) / s
    q = (jj - 0.5 * (s - 1)) / s
    a0 = np.floor(r).astype(np.int64)
    b0 = np.floor(q).astype(np.int64)
    fin = np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
    f64 = np.where(fin[..., None], f, np.float32(0)).astype(np.float64)
    U, V, Sw = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    Us, Vs, Ss = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(all="ignore"):
        for ta in range(-1, 3):
            a = a0 + ta
            wa = np.maximum(1.0 - np.abs(a - r) / 2.0, 0.0)
            for tb in range(-1, 3):
                b = b0 + tb
                ac, bc = np.clip(a, 0, hs - 1), np.clip(b, 0, ws - 1)
                ok = (a >= 0) & (a < hs) & (b >= 0) & (b < ws) & fin[ac, bc]
                wb = np.maximum(1.0 - np.abs(b - q) / 2.0, 0.0)
                wsp = wa * wb
                D = np.zeros((H, W))
                for c in range(C):
                    d = G[..., c] - L[ac, bc, c]
                    D = D + d * d
                z = D / (C * h2)
                x = np.where(z < 1.0, z, 1.0)
                wr = np.ones((H, W)) if spatial_only else (1.0 - x) * (1.0 - x)
                w = wsp * wr
                fx, fy = f64[ac, bc, 0], f64[ac, bc, 1]
                U = np.where(ok, U + w * fx, U)
                V = np.where(ok, V + w * fy, V)
                Sw = np.where(ok, Sw + w, Sw)
                Us = np.where(ok, Us + wsp * fx, Us)
                Vs = np.where(ok, Vs + wsp * fy, Vs)
                Ss = np.where(ok, Ss + wsp, Ss)
        e0, e1 = Sw > 0, ~(Sw > 0) & (Ss > 0)
        u = np.where(e0, s * (U / Sw), np.where(e1, s * (Us / Ss), np.nan))
        v = np.where(e0, s * (V / Sw), np.where(e1, s * (Vs / Ss), np.nan))
        out = np.stack([u, v], -1).astype(np.float32)
    info = np.where(e0, 0, np.where(e1, 1, 2)).astype(np.uint8)
    return out, info


def two_layer_scene(H, W, sigma, seed=0):
    """The sharpness scene: a 3-channel frame (background 90 + 25 sin(x/5)
    cos(y/7), a foreground rectangle 170 + 25 cos(x/4 + y/6) on rows H//4+1 ..
    3H//4-1 and columns W//3+1 .. 2W//3+1, Gaussian noise of `sigma` from a
    fixed seed), its true flow ((0.5, 0) outside, (3, -2) inside) and the
    rectangle's mask."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = (y >= H // 4 + 1) & (y <= 3 * H // 4 - 1) & (x >= W // 3 + 1) & (x <= 2 * W // 3 + 1)
    base = np.where(inside, 170.0 + 25.0 * np.cos(x / 4.0 + y / 6.0), 90.0 + 25.0 * np.sin(x / 5.0) * np.cos(y / 7.0))
    im = np.repeat(base[..., None], 3, axis=2)
    if sigma > 0:
        im = im + np.random.default_rng(seed).normal(0.0, sigma, im.shape)
    flow = np.where(inside[..., None], np.array([3.0, -2.0]), np.array([0.5, 0.0]))
    return im.astype(np.float32), flow.astype(np.float32), inside


def outline_band(inside, s):
    """The pixels within s pixels (Chebyshev) of the mask's outline: those
    whose (2s+1)^2 window holds both classes."""
    H, W = inside.shape
    p = np.pad(inside, s, mode="edge")
    any_in, any_out = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for a in range(2 * s + 1):
        for b in range(2 * s + 1):
            v = p[a:a + H, b:b + W]
            any_in |= v
            any_out |= ~v
    return any_in & any_out
