"""numpy float64 restatement of the temporal denoising (include/optflow.h,
"Motion-compensated temporal denoising"): of_flow_compose and of_fuse_frames
operation for operation, in the order the header writes them, and the
session's schedule built from them.  Test helper, not a conftest."""
import numpy as np

from track_numpy import inside, near


def bil(A, r, q):
    """The clamped bilinear sample of A (H, W) or (H, W, C) float64 at finite
    (r, q) arrays of one shape; channels, if any, come last."""
    H, W = A.shape[:2]
    qc = np.minimum(np.maximum(q, 0.0), float(W - 1))
    rc = np.minimum(np.maximum(r, 0.0), float(H - 1))
    qf, rf = np.floor(qc), np.floor(rc)
    j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
    fc, fr = qc - qf, rc - rf
    if A.ndim == 3:
        fc, fr = fc[..., None], fr[..., None]
    j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
    return (1.0 - fr) * ((1.0 - fc) * A[i0, j0] + fc * A[i0, j1]) + fr * ((1.0 - fc) * A[i1, j0] + fc * A[i1, j1])


def _landing(flow):
    """(u, v, r, q, ok): the float64 flow, where it lands, and whether it is
    finite and lands inside the frame (r, q zeroed where not)."""
    H, W = flow.shape[:2]
    ii, jj = np.mgrid[0:H, 0:W]
    fin = np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
    with np.errstate(all="ignore"):
        u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
        r, q = ii + v, jj + u
        ok = fin & inside(r, q, H, W)
    return u, v, np.where(ok, r, 0.0), np.where(ok, q, 0.0), ok


def compose(f, g, state_f=None, state_g=None):
    """of_flow_compose: (out (H, W, 2) float32, out_state (H, W) uint8)."""
    f = np.asarray(f).astype(np.float32)
    G = np.asarray(g).astype(np.float32).astype(np.float64)
    H, W = f.shape[:2]
    sf = np.zeros((H, W), np.uint8) if state_f is None else np.asarray(state_f, dtype=np.uint8)
    sg = np.zeros((H, W), np.uint8) if state_g is None else np.asarray(state_g, dtype=np.uint8)
    u, v, r, q, ok = _landing(f)
    with np.errstate(all="ignore"):
        gu, gv = bil(G[..., 0], r, q), bil(G[..., 1], r, q)
        chained = np.stack([(u + gu).astype(np.float32), (v + gv).astype(np.float32)], -1)
    out = np.where(ok[..., None], chained, f)
    state = np.where(ok, np.maximum(sf, sg[near(r, H), near(q, W)]), np.uint8(2)).astype(np.uint8)
    return out, state


def weights(center, neighbours, flows, sigma, states=None, strength=4.0, patch=2):
    """Per neighbour (vis (H, W) bool, Wk (H, W, C) float64 warped sample, w
    (H, W) float64 weight) of of_fuse_frames."""
    I = np.asarray(center).astype(np.float32).astype(np.float64)
    I = I[..., None] if I.ndim == 2 else I
    H, W, C = I.shape
    r_ = int(patch)
    two_s2 = 2.0 * (sigma * sigma)
    h2 = (strength * sigma) * (strength * sigma)
    res = []
    for k, (Nk, fk) in enumerate(zip(neighbours, flows)):
        N = np.asarray(Nk).astype(np.float32).astype(np.float64)
        N = N[..., None] if N.ndim == 2 else N
        _, _, r, q, ok = _landing(np.asarray(fk).astype(np.float32))
        sk = None if states is None else states[k]
        vis = ok if sk is None else ok & (np.asarray(sk) == 0)
        Wk = bil(N, r, q)
        D = np.zeros((H, W))
        for c in range(C):
            dd = I[..., c] - Wk[..., c]
            D = D + dd * dd
        pv = np.pad(vis, r_)
        pD = np.pad(np.where(vis, D, 0.0), r_)
        S, m = np.zeros((H, W)), np.zeros((H, W))
        for a in range(2 * r_ + 1):
            for b in range(2 * r_ + 1):
                sl = (slice(a, a + H), slice(b, b + W))
                S = np.where(pv[sl], S + pD[sl], S)
                m = m + pv[sl]
        with np.errstate(all="ignore"):
            d = S / (m * C)
            t = d - two_s2
            e = np.where(t > 0.0, t, 0.0)
            z = e / h2
            x = np.where(z < 1.0, z, 1.0)
            w = np.where(vis, (1.0 - x) * (1.0 - x), 0.0)
        res.append((vis, Wk, w))
    return res


def fuse(center, neighbours, flows, sigma, states=None, strength=4.0, patch=2):
    """of_fuse_frames: (out float32 in center's shape, out_weight (H, W) float32)."""
    I = np.asarray(center).astype(np.float32).astype(np.float64)
    I3 = I[..., None] if I.ndim == 2 else I
    acc = I3.copy()
    wsum = np.ones(I3.shape[:2])
    for vis, Wk, w in weights(center, neighbours, flows, sigma, states, strength, patch):
        acc = np.where(vis[..., None], acc + w[..., None] * Wk, acc)
        wsum = np.where(vis, wsum + w, wsum)
    out = (acc / wsum[..., None]).astype(np.float32)
    return out.reshape(I.shape), wsum.astype(np.float32)


def session(frames, pairs, sigma, radius=1, strength=4.0, patch=2, compose_fn=compose, fuse_fn=fuse):
    """The session's output for every frame of a clip: pairs[j] = (fw, bw, sf,
    sb) of frames (j, j+1); neighbours at offsets -1, +1, -2, +2 that exist.
    compose_fn / fuse_fn as compose / fuse above (or the package's, wrapped)."""
    T = len(frames)
    outs = []
    for t in range(T):
        nb, fl, st = [], [], []
        for a in range(1, radius + 1):
            for sgn in (-1, 1):
                s = t + sgn * a
                if s < 0 or s >= T:
                    continue
                k = 0 if sgn > 0 else 1  # forward flows of pairs t, t+1; backward flows of pairs t-1, t-2
                p0, p1 = (t, t + 1) if sgn > 0 else (t - 1, t - 2)
                if a == 1:
                    f, m = pairs[p0][k], pairs[p0][2 + k]
                else:
                    f, m = compose_fn(pairs[p0][k], pairs[p1][k], pairs[p0][2 + k], pairs[p1][2 + k])
                nb.append(frames[s])
                fl.append(f)
                st.append(m)
        if not nb:
            c = np.asarray(frames[t]).astype(np.float32)
            outs.append((c, np.ones(c.shape[:2], np.float32)))
        else:
            outs.append(fuse_fn(frames[t], nb, fl, sigma, st, strength, patch))
    return outs
