"""numpy float64 restatement of the Poisson solver behind the blended fill
(include/optflow.h, "Gradient-domain blending"): the fixed multilevel schedule
of of_poisson_solve operation for operation, in the order the header writes
it, and the two-stage blended fill built on inpaint_numpy.fill.  Test helper,
not a conftest."""
import numpy as np

import inpaint_numpy as ip

FIXED, UNKNOWN, EXCLUDED = 0, 1, 2
SPATIAL = 3
CMAX = 1024        # (H_L + 2) * (W_L + 2) of the coarsest level
OMEGA = 1.5        # the coarse correction's factor
CYCLES, SWEEPS, COARSE = 8, 2, 32
MAX_CYCLES, MAX_SWEEPS, MAX_COARSE = 64, 2, 64


def n_levels(H, W):
    """L: the first level whose frame, with a one-cell apron, has at most CMAX
    cells; level l has ceil(H / 2^l) x ceil(W / 2^l) cells."""
    L = 0
    while (-(-H >> L) + 2) * (-(-W >> L) + 2) > CMAX:
        L += 1
    return L


def _pad(a, value):
    w = [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)]
    return np.pad(a, w, constant_values=value)


def _nb(P):
    """The neighbours up, down, left, right of the inner cells of a padded array."""
    return P[..., :-2, 1:-1], P[..., 2:, 1:-1], P[..., 1:-1, :-2], P[..., 1:-1, 2:]


class _Level:
    """One level's window: rows r0 .. r0 + h - 1 and columns c0 .. of the level's
    grid (anchored at the frame origin).  d: the diagonal (0: the cell is not
    solved for), w: the weights of the neighbours up, down, left, right (0: no
    coupling), all integers."""

    def __init__(self, d, w, r0, c0):
        self.r0, self.c0 = r0, c0
        self.h, self.w_ = d.shape
        self.d, self.w = d, w
        self.unk = d > 0
        self.dd = np.maximum(d, 1).astype(np.float64)
        self.wd = [x.astype(np.float64) for x in w]
        self.nbu = [x != 0 for x in w]
        ii, jj = np.mgrid[r0:r0 + self.h, c0:c0 + self.w_]
        self.colour = [self.unk & (((ii + jj) & 1) == k) for k in (0, 1)]

    @classmethod
    def finest(cls, lab, r0, c0):
        """d = deg, the neighbours that are not excluded, on the unknown cells
        (an unknown cell with deg 0 is left alone); w = 1 towards an unknown
        neighbour."""
        P = _pad(lab, EXCLUDED)
        deg = np.zeros(lab.shape, np.int64)
        for n in _nb(P):
            deg += n != EXCLUDED
        d = np.where(lab == UNKNOWN, deg, 0)
        Pd = _pad(d, 0)
        w = [((d > 0) & (n > 0)).astype(np.int64) for n in _nb(Pd)]
        return cls(d, w, r0, c0)

    def coarsen(self):
        """The next level's window, the Galerkin operator of piecewise-constant
        transfer: with the children c00 c01 / c10 c11 of a cell,
          w_up = w_up(c00) + w_up(c01), w_down = w_down(c10) + w_down(c11),
          w_left = w_left(c00) + w_left(c10), w_right = w_right(c01) + w_right(c11),
          d = d(c00) + d(c01) + d(c10) + d(c11)
              - 2 (w_right(c00) + w_right(c10) + w_down(c00) + w_down(c01))."""
        def ch(a, i, j):
            return a[i::2, j::2]
        U, D, L, R = self.w
        w = [ch(U, 0, 0) + ch(U, 0, 1), ch(D, 1, 0) + ch(D, 1, 1), ch(L, 0, 0) + ch(L, 1, 0),
             ch(R, 0, 1) + ch(R, 1, 1)]
        d = ch(self.d, 0, 0) + ch(self.d, 0, 1) + ch(self.d, 1, 0) + ch(self.d, 1, 1) \
            - 2 * (ch(R, 0, 0) + ch(R, 1, 0) + ch(D, 0, 0) + ch(D, 0, 1))
        return _Level(d, w, self.r0 >> 1, self.c0 >> 1)


def _relax(lv, x, b, k):
    """One colour of red-black Gauss-Seidel: x_p = (b_p + w_n x_n over the
    coupled neighbours up, down, left, right) / d on the solved cells with
    (i + j) & 1 == k."""
    P = _pad(x, 0.0)
    t = b.copy()
    for n, u, w in zip(_nb(P), lv.nbu, lv.wd):
        t = np.where(u, t + w * n, t)
    return np.where(lv.colour[k], t / lv.dd, x)


def _residual(lv, x, b):
    P = _pad(x, 0.0)
    r = b - lv.dd * x
    for n, u, w in zip(_nb(P), lv.nbu, lv.wd):
        r = np.where(u, r + w * n, r)
    return np.where(lv.unk, r, 0.0)


def _restrict(lv, x, b):
    """The coarse right-hand side: the four children's residuals, (2I, 2J),
    (2I, 2J+1), (2I+1, 2J), (2I+1, 2J+1) in this order."""
    r = _residual(lv, x, b)
    r = r.reshape(r.shape[0], lv.h // 2, 2, lv.w_ // 2, 2)
    return ((r[:, :, 0, :, 0] + r[:, :, 0, :, 1]) + r[:, :, 1, :, 0]) + r[:, :, 1, :, 1]


def _cycle(lvs, l, x, b, sweeps, coarse):
    lv = lvs[l]
    if l == len(lvs) - 1:
        for _ in range(coarse):
            x = _relax(lv, x, b, 0)
            x = _relax(lv, x, b, 1)
        return x
    for _ in range(sweeps):
        x = _relax(lv, x, b, 0)
        x = _relax(lv, x, b, 1)
    nx = lvs[l + 1]
    rc = np.where(nx.unk, _restrict(lv, x, b), 0.0)
    e = np.zeros_like(rc)
    e = _cycle(lvs, l + 1, e, rc, sweeps, coarse)
    if l + 1 < len(lvs) - 1:
        e = _cycle(lvs, l + 1, e, rc, sweeps, coarse)  # W: every level but the coarsest twice
    up = np.repeat(np.repeat(e, 2, axis=1), 2, axis=2)
    x = np.where(lv.unk, x + OMEGA * up, x)
    for _ in range(sweeps):
        x = _relax(lv, x, b, 0)
        x = _relax(lv, x, b, 1)
    return x


def solve(label, v, s=None, h=None, cycles=CYCLES, sweeps=SWEEPS, coarse=COARSE, crop=True, trace=None):
    """of_poisson_solve: label (H, W) of FIXED / UNKNOWN / EXCLUDED, v (C, H, W)
    float64, s (C, H, W) and h (H, W) the guidance or None.  Returns x
    (C, H, W) float64.  crop: work on the window around the unknowns only (the
    library's), else on the whole frame; the results are the same bits.
    trace(k, x): called with the frame-sized iterate after every cycle."""
    label = np.asarray(label, np.uint8)
    v = np.asarray(v, np.float64)
    H, W = label.shape
    out = v.copy()
    ii, jj = np.nonzero(label == UNKNOWN)
    if ii.size == 0:
        return out
    L = n_levels(H, W)
    if crop:
        a_i, b_i, a_j, b_j = (ii.min() >> L) - 1, (ii.max() >> L) + 1, (jj.min() >> L) - 1, (jj.max() >> L) + 1
    else:
        a_i, b_i, a_j, b_j = -1, -(-H >> L), -1, -(-W >> L)
    r0, r1, c0, c1 = a_i << L, (b_i + 1) << L, a_j << L, (b_j + 1) << L  # the fine window [r0, r1) x [c0, c1)
    fi0, fi1, fj0, fj1 = max(r0, 0), min(r1, H), max(c0, 0), min(c1, W)
    win = (slice(fi0 - r0, fi1 - r0), slice(fj0 - c0, fj1 - c0))
    src = (slice(fi0, fi1), slice(fj0, fj1))

    def window(a, fill, dtype):
        w = np.full(a.shape[:-2] + (r1 - r0, c1 - c0), fill, dtype)
        w[(Ellipsis,) + win] = a[(Ellipsis,) + src]
        return w

    lab = window(label, EXCLUDED, np.uint8)
    lv = _Level.finest(lab, r0, c0)
    lvs = [lv]
    for _ in range(L):
        lvs.append(lvs[-1].coarsen())
    x = window(v, 0.0, np.float64)
    # the right-hand side: the guidance, then the fixed neighbours' values, each up, down, left, right
    Pv = _pad(x, 0.0)
    g = np.zeros_like(x)
    if s is not None:
        sw = window(np.asarray(s, np.float64), 0.0, np.float64)
        hw = window(np.asarray(h) != 0, False, bool)
        Ps, Ph = _pad(sw, 0.0), _pad(hw, False)
        for n, hn, cn in zip(_nb(Ps), _nb(Ph), _nb(_pad(lab, EXCLUDED))):
            g = np.where(hw & hn & (cn != EXCLUDED), g + (sw - n), g)
    f = np.zeros_like(x)
    for n, cn in zip(_nb(Pv), _nb(_pad(lab, EXCLUDED))):
        f = np.where(cn == FIXED, f + n, f)
    b = np.where(lv.unk, g + f, 0.0)
    for k in range(cycles):
        x = _cycle(lvs, 0, x, b, sweeps, coarse)
        if trace is not None:
            o = out.copy()
            o[(Ellipsis,) + src] = x[(Ellipsis,) + win]
            trace(k, o)
    out[(Ellipsis,) + src] = x[(Ellipsis,) + win]
    return out


def exact(label, v, s=None, h=None):
    """The same linear problem solved by scipy.sparse (a singular component
    raises or gives garbage: callers avoid it)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    label = np.asarray(label, np.uint8)
    v = np.asarray(v, np.float64)
    Cn, H, W = v.shape
    idx = -np.ones((H, W), np.int64)
    ii, jj = np.nonzero(label == UNKNOWN)
    idx[ii, jj] = np.arange(ii.size)
    deg = np.zeros(ii.size)
    rhs = np.zeros((ii.size, Cn))
    rows, cols, vals = [], [], []
    hh = None if h is None else np.asarray(h) != 0
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ni, nj = ii + di, jj + dj
        ok = (ni >= 0) & (ni < H) & (nj >= 0) & (nj < W)
        nic, njc = np.clip(ni, 0, H - 1), np.clip(nj, 0, W - 1)
        ok &= label[nic, njc] != EXCLUDED
        deg += ok
        un = ok & (label[nic, njc] == UNKNOWN)
        rows.append(np.flatnonzero(un))
        cols.append(idx[nic, njc][un])
        vals.append(-np.ones(int(un.sum())))
        fx = ok & (label[nic, njc] == FIXED)
        rhs[fx] += v[:, nic[fx], njc[fx]].T
        if s is not None:
            gd = ok & hh[ii, jj] & hh[nic, njc]
            rhs[gd] += (np.asarray(s, np.float64)[:, ii[gd], jj[gd]] - np.asarray(s, np.float64)[:, nic[gd], njc[gd]]).T
    keep = deg > 0
    rows.append(np.arange(ii.size))
    cols.append(np.arange(ii.size))
    vals.append(np.where(keep, deg, 1.0))
    rhs[~keep] = v[:, ii[~keep], jj[~keep]].T
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ii.size, ii.size))
    sol = spl.splu(A).solve(rhs)
    out = v.copy()
    out[:, ii, jj] = sol.T
    return out


def blend(frames, masks, fw, bw, t, radius=8, grow_=2, cycles=CYCLES, sweeps=SWEEPS, coarse=COARSE, solver=solve):
    """of_inpaint_blend: (out float32 in the frames' shape, status (H, W) uint8)."""
    s32, st, _, _ = ip.fill(frames, masks, fw, bw, t, radius, grow_ + 1)
    shape = s32.shape
    I32 = np.asarray(frames[t]).astype(np.float32).reshape(shape)
    chan = (lambda a: a[None]) if I32.ndim == 2 else (lambda a: np.moveaxis(a, 2, 0))
    I, s = chan(I32).astype(np.float64), chan(s32).astype(np.float64)
    h = st == ip.FILLED
    Om = ip.grow(masks[t], grow_) != 0
    lab = np.where(Om & h, UNKNOWN, np.where(Om, EXCLUDED, FIXED)).astype(np.uint8)
    x = solver(lab, np.where(lab == UNKNOWN, s, I), s, h, cycles=cycles, sweeps=sweeps, coarse=coarse)
    if (Om & ~h).any():
        lab = np.where(Om & ~h, UNKNOWN, FIXED).astype(np.uint8)
        x = solver(lab, np.where(lab == UNKNOWN, I, x), cycles=cycles, sweeps=sweeps, coarse=coarse)
    x32 = x.astype(np.float32)
    x32 = x32[0] if I32.ndim == 2 else np.moveaxis(x32, 0, 2)
    out = np.where(Om if I32.ndim == 2 else Om[..., None], x32, I32)
    status = np.where(Om, np.where(h, ip.FILLED, SPATIAL), ip.KEPT).astype(np.uint8)
    return out, status


def blob_label(H, W):
    """The accuracy tests' hole: an ellipse whose rim is modulated by sin * cos,
    with a 4-pixel-high strip attached that reaches to 3 pixels from the left
    edge."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx, ry, rx = 0.5 * H, 0.55 * W, 0.33 * H, 0.3 * W
    th = np.arctan2(yy - cy, xx - cx)
    rim = 1.0 + 0.18 * np.sin(5.0 * th) * np.cos(3.0 * th)
    m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= rim ** 2
    i0 = int(cy) - 2
    m[i0:i0 + 4, 3:int(cx)] = True
    return m.astype(np.uint8)


def off_start(rng, truth, label):
    """Truth on the fixed pixels; on the unknown ones off by 10 % gain + 12
    with sigma = 3 noise."""
    bad = 1.1 * truth + 12.0 + rng.normal(0.0, 3.0, truth.shape)
    return np.where(label == UNKNOWN, bad, truth)
