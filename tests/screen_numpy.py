"""numpy float64 restatement of the blind temporal consistency
(include/optflow.h, "Blind temporal consistency"): the screened Poisson solve
of of_screened_solve operation for operation, in the order the header writes
it, on the levels and integer operators of poisson_numpy, and the consistency
step built on fuse_numpy's weights; an exact sparse solve of the same system
and the two measures of the quality tests.  Test helper, not a conftest."""
import numpy as np

import fuse_numpy as fn
import poisson_numpy as pn

OMEGA = 1.5        # the coarse correction's factor (measured for this operator too: DESIGN.md)
CYCLES, SWEEPS, COARSE = 5, 2, 32   # 5: the smallest count within half an 8-bit level (test_screen_cpu.py)
LAMBDA = 1.0


class _SLevel:
    """A level of the screened problem: poisson_numpy's level (integer d and
    w of the all-unknown Neumann Laplacian) and the plane q; a cell is solved
    for where (double)d + q > 0."""

    def __init__(self, lv, q):
        self.lv, self.q = lv, q
        self.dg = lv.d.astype(np.float64) + q
        self.solved = self.dg > 0.0
        self.dgs = np.where(self.solved, self.dg, 1.0)
        ii, jj = np.mgrid[lv.r0:lv.r0 + lv.h, lv.c0:lv.c0 + lv.w_]
        self.colour = [self.solved & (((ii + jj) & 1) == k) for k in (0, 1)]

    def coarsen(self):
        q = self.q
        return _SLevel(self.lv.coarsen(), ((q[0::2, 0::2] + q[0::2, 1::2]) + q[1::2, 0::2]) + q[1::2, 1::2])


def _relax(sl, x, b, k):
    P = pn._pad(x, 0.0)
    t = b.copy()
    for n, u, w in zip(pn._nb(P), sl.lv.nbu, sl.lv.wd):
        t = np.where(u, t + w * n, t)
    return np.where(sl.colour[k], t / sl.dgs, x)


def _residual(sl, x, b):
    P = pn._pad(x, 0.0)
    r = b - sl.dg * x
    for n, u, w in zip(pn._nb(P), sl.lv.nbu, sl.lv.wd):
        r = np.where(u, r + w * n, r)
    return np.where(sl.solved, r, 0.0)


def _restrict(sl, x, b):
    r = _residual(sl, x, b)
    r = r.reshape(r.shape[0], sl.lv.h // 2, 2, sl.lv.w_ // 2, 2)
    return ((r[:, :, 0, :, 0] + r[:, :, 0, :, 1]) + r[:, :, 1, :, 0]) + r[:, :, 1, :, 1]


def _cycle(sls, l, x, b, sweeps, coarse, omega):
    sl = sls[l]
    if l == len(sls) - 1:
        for _ in range(coarse):
            x = _relax(sl, x, b, 0)
            x = _relax(sl, x, b, 1)
        return x
    for _ in range(sweeps):
        x = _relax(sl, x, b, 0)
        x = _relax(sl, x, b, 1)
    nx = sls[l + 1]
    rc = np.where(nx.solved, _restrict(sl, x, b), 0.0)
    e = np.zeros_like(rc)
    e = _cycle(sls, l + 1, e, rc, sweeps, coarse, omega)
    if l + 1 < len(sls) - 1:
        e = _cycle(sls, l + 1, e, rc, sweeps, coarse, omega)
    up = np.repeat(np.repeat(e, 2, axis=1), 2, axis=2)
    x = np.where(sl.lv.unk, x + omega * up, x)
    for _ in range(sweeps):
        x = _relax(sl, x, b, 0)
        x = _relax(sl, x, b, 1)
    return x


def levels(H, W):
    """(L, the windows' (r0, c0, h, w) of levels 0 .. L): every level's whole
    grid plus a one-cell apron of the coarsest level's cells."""
    L = pn.n_levels(H, W)
    hL, wL = -(-H >> L) + 2, -(-W >> L) + 2
    return L, [(-(1 << (L - l)), -(1 << (L - l)), hL << (L - l), wL << (L - l)) for l in range(L + 1)]


def solve(P, A, q, cycles=CYCLES, sweeps=SWEEPS, coarse=COARSE, omega=OMEGA, trace=None):
    """of_screened_solve: P (C, H, W) the target (fp32 values as float64), A
    (C, H, W) the anchor, q (H, W) >= 0 the screening plane.  Returns x
    (C, H, W) float64.  trace(k, x) after every cycle."""
    P = np.asarray(P, np.float64)
    A = np.asarray(A, np.float64)
    q = np.asarray(q, np.float64)
    _, H, W = P.shape
    L, wins = levels(H, W)
    r0, c0, h, w = wins[0]
    win = (slice(-r0, H - r0), slice(-c0, W - c0))

    def window(a, fill, dtype):
        o = np.full(a.shape[:-2] + (h, w), fill, dtype)
        o[(Ellipsis,) + win] = a
        return o

    lab = window(np.full((H, W), pn.UNKNOWN, np.uint8), pn.EXCLUDED, np.uint8)
    sls = [_SLevel(pn._Level.finest(lab, r0, c0), window(q, 0.0, np.float64))]
    for _ in range(L):
        sls.append(sls[-1].coarsen())
    x = window(P, 0.0, np.float64)
    inside = lab == pn.UNKNOWN
    g = np.zeros_like(x)
    for n, cn in zip(pn._nb(pn._pad(x, 0.0)), pn._nb(pn._pad(lab, pn.EXCLUDED))):
        g = np.where(inside & (cn != pn.EXCLUDED), g + (x - n), g)
    b = np.where(inside, g + sls[0].q * window(A, 0.0, np.float64), 0.0)
    for k in range(cycles):
        x = _cycle(sls, 0, x, b, sweeps, coarse, omega)
        if trace is not None:
            trace(k, x[(Ellipsis,) + win].copy())
    return x[(Ellipsis,) + win].copy()


def exact(P, A, q):
    """The same linear system solved by scipy.sparse; q == 0 everywhere is
    singular (callers avoid it), a 1 x 1 frame is x = A."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    P = np.asarray(P, np.float64)
    A = np.asarray(A, np.float64)
    q = np.asarray(q, np.float64)
    Cn, H, W = P.shape
    idx = np.arange(H * W).reshape(H, W)
    deg = np.zeros((H, W))
    g = np.zeros((Cn, H, W))
    rows, cols = [], []
    for a, b_ in (((slice(1, None), slice(None)), (slice(None, -1), slice(None))),      # up
                  ((slice(None, -1), slice(None)), (slice(1, None), slice(None))),      # down
                  ((slice(None), slice(1, None)), (slice(None), slice(None, -1))),      # left
                  ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):     # right
        deg[a] += 1
        g[(slice(None),) + a] += P[(slice(None),) + a] - P[(slice(None),) + b_]
        rows.append(idx[a].ravel())
        cols.append(idx[b_].ravel())
    n = H * W
    off = sp.csc_matrix((-np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))),
                        shape=(n, n))
    M = (off + sp.diags((deg + q).ravel())).tocsc()
    rhs = (g + q * A).reshape(Cn, n).T
    return spl.splu(M).solve(rhs).T.reshape(Cn, H, W)


def _chan(a):
    a = np.asarray(a)
    return a[..., None] if a.ndim == 2 else a


def step(frame, prev_frame, processed, prev_out, flow, state=None, lam=LAMBDA, sigma=None, strength=4.0, patch=1,
         cycles=CYCLES, sweeps=SWEEPS, coarse=COARSE, solver=solve):
    """of_consist_step: (out float32 in processed's shape, out_weight (H, W)
    float32)."""
    flow32 = np.asarray(flow).astype(np.float32)
    vis, _, w = fn.weights(frame, [prev_frame], [flow32], sigma, None if state is None else [state], strength,
                           patch)[0]
    w32 = w.astype(np.float32)
    P32 = np.asarray(processed).astype(np.float32)
    O = _chan(np.asarray(prev_out).astype(np.float32)).astype(np.float64)
    _, _, r, qq, _ = fn._landing(flow32)
    q = lam * w32.astype(np.float64)
    A = np.where(vis[..., None], fn.bil(O, r, qq), 0.0)
    x = solver(np.moveaxis(_chan(P32).astype(np.float64), 2, 0), np.moveaxis(A, 2, 0), q, cycles=cycles,
               sweeps=sweeps, coarse=coarse)
    return np.moveaxis(x, 0, 2).astype(np.float32).reshape(P32.shape), w32


def clip(frames, processed, flows, states=None, **kw):
    """The session along given backward flows: flows[k] = frame k+1 -> frame k.
    Returns the outputs, float32."""
    outs = [np.asarray(processed[0]).astype(np.float32)]
    for k in range(1, len(frames)):
        st = None if states is None else states[k - 1]
        outs.append(step(frames[k], frames[k - 1], processed[k], outs[-1], flows[k - 1], st, **kw)[0])
    return outs


# ---- the measures of the quality tests --------------------------------------
def instability(outs, true_bw, true_vis):
    """The mean of (O_t - warp(O_{t-1}))^2 along the true backward flows over
    the pixels the true masks say are visible in both frames."""
    num, den = 0.0, 0
    for t in range(1, len(outs)):
        O, Op = _chan(np.asarray(outs[t], np.float64)), _chan(np.asarray(outs[t - 1], np.float64))
        _, _, r, q, ok = fn._landing(np.asarray(true_bw[t - 1], np.float32))
        m = ok & true_vis[t - 1]
        d = (O - fn.bil(Op, r, q)) ** 2
        num += float(d[m].sum())
        den += int(m.sum()) * O.shape[2]
    return num / max(den, 1)


def fidelity(outs, processed):
    """The mean of |grad O_t - grad P_t|^2 (forward differences, both axes)."""
    num, den = 0.0, 0
    for O, P in zip(outs, processed):
        D = _chan(np.asarray(O, np.float64)) - _chan(np.asarray(P, np.float64))
        gy, gx = D[1:] - D[:-1], D[:, 1:] - D[:, :-1]
        num += float((gy ** 2).sum() + (gx ** 2).sum())
        den += gy.size + gx.size
    return num / max(den, 1)


def flicker_clip(frames, seed=5, gain=0.08, offset=6.0):
    """The processed clip of the quality tests: frame t times a gain of
    1 +- `gain` plus an offset of +- `offset`, drawn per frame from a seeded
    generator."""
    rng = np.random.default_rng(seed)
    return [(np.asarray(f, np.float64) * (1.0 + rng.uniform(-gain, gain)) + rng.uniform(-offset, offset)).astype(
        np.float32) for f in frames]


def patch_weights(H, W, seed):
    """The convergence tests' screening plane: patches of 0, 1e-3, 1 and 1e3."""
    rng = np.random.default_rng(seed)
    ph, pw = max(H // 4, 1), max(W // 4, 1)
    k = rng.integers(0, 4, (-(-H // ph), -(-W // pw)))
    k.flat[0] = 2  # never singular: one patch of 1 at least
    return np.repeat(np.repeat(np.array([0.0, 1e-3, 1.0, 1e3])[k], ph, axis=0), pw, axis=1)[:H, :W]


def convergence_case(H, W):
    """(P, A, q) of the convergence tests: P a textured image on 0..255 (fp32
    values), A that image off by 10 % gain + 12 with sigma = 3 noise, q
    patch_weights."""
    import inpaint_numpy as ip
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    tr = ip._texture(np.random.default_rng(3), xx, yy)[None]
    A = 1.1 * tr + 12.0 + np.random.default_rng(1).normal(0.0, 3.0, tr.shape)
    return tr.astype(np.float32).astype(np.float64), A, patch_weights(H, W, H * W)


def _truth(masks, bg, obj_step):
    """True backward flows and visibility of a clip whose background moves by
    the (H, W, 2) flows bg[k] (frame k+1 -> frame k) and whose masked object
    moves rigidly: obj_step(k) = its (u, v) from frame k+1 to frame k.
    vis[k]: the pixel of frame k+1 shows the same surface in frame k (the flow
    lands inside the frame and, on the background, not within a pixel of the
    object of frame k)."""
    import inpaint_numpy as ip
    H, W = masks[0].shape
    ii, jj = np.mgrid[0:H, 0:W]
    flows, vis = [], []
    for k in range(len(masks) - 1):
        obj = masks[k + 1] != 0
        f = np.where(obj[..., None], np.float32(obj_step(k)), bg[k]).astype(np.float32)
        r, q = ii + f[..., 1].astype(np.float64), jj + f[..., 0].astype(np.float64)
        ok = (q >= 0) & (q <= W - 1) & (r >= 0) & (r <= H - 1)
        ri, qi = np.clip(np.rint(r).astype(int), 0, H - 1), np.clip(np.rint(q).astype(int), 0, W - 1)
        near_obj = ip.grow(masks[k], 1)[ri, qi] != 0
        flows.append(f)
        vis.append(ok & np.where(obj, masks[k][ri, qi] != 0, ~near_obj))
    return flows, vis


def scene_truth():
    """(frames, true_bw, true_vis) of the quality tests' clip, the 9 frames of
    48 x 64 of inpaint_numpy.scene(0): the background moves by its known flows,
    the rectangle by whole pixels."""
    import inpaint_numpy as ip
    frames, masks, _, bw, _ = ip.scene(0)
    pos = [(int(round(ip.OBJ_X0 + ip.OBJ_V[0] * s)), int(round(ip.OBJ_Y0 + ip.OBJ_V[1] * s)))
           for s in range(len(frames))]
    flows, vis = _truth(masks, bw, lambda k: (pos[k][0] - pos[k + 1][0], pos[k][1] - pos[k + 1][1]))
    return frames, flows, vis
