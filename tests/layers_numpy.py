"""numpy float64 restatement of the layered motion segmentation
(include/optflow.h, "Layered motion segmentation"): hypotheses from the cells
of the pass-0 tile records, consensus extraction, joint assign-and-refit rounds
and the label mode filter, operation for operation, on the ordered sums and the
solve of tests/motion_numpy.py.  Test helper, not a conftest."""
from types import SimpleNamespace

import numpy as np

import motion_numpy as mn

NONE = 255


def _r2(th, x, y, u, v):
    with np.errstate(all="ignore"):
        uh = th[0] + th[1] * x + th[2] * y
        vh = th[3] + th[4] * x + th[5] * y
        ru, rv = u - uh, v - vh
        return ru * ru + rv * rv


def _planes(th, x, y, u, v, w0, c2):
    """The 13 planes of one pass of the fit: pass 0 for c2 None, else a Tukey
    pass with the squared cutoff c2."""
    with np.errstate(all="ignore"):
        r2 = _r2(th, x, y, u, v)
        if c2 is None:
            w = w0
        else:
            z = r2 / c2
            t = np.where(z < 1.0, z, 1.0)
            w = w0 * ((1.0 - t) * (1.0 - t))
        wx, wy = w * x, w * y
        return (w, wx, wy, wx * x, wx * y, wy * y, w * u, wx * u, wy * u, w * v, wx * v, wy * v, w * r2)


def mode_filter(lab, n, r):
    """Every label becomes the value among 0 .. n-1, 255 that occurs most often
    in the in-frame part of its (2r+1)^2 window; the smallest value wins a tie."""
    H, W = lab.shape
    if r == 0:
        return lab.copy()
    pad = np.full((H + 2 * r, W + 2 * r), 254, np.uint8)   # 254: outside the frame, never counted
    pad[r:r + H, r:r + W] = lab
    best = np.full((H, W), -1, np.int64)
    out = np.zeros((H, W), np.uint8)
    for val in list(range(n)) + [NONE]:
        cnt = np.zeros((H, W), np.int64)
        for di in range(2 * r + 1):
            for dj in range(2 * r + 1):
                cnt += pad[di:di + H, dj:dj + W] == val
        m = cnt > best
        best = np.where(m, cnt, best)
        out = np.where(m, np.uint8(val), out)
    return out


def pick(counts):
    """The hypothesis with the largest count, the lowest index on a tie;
    `counts` maps index -> count.  None without a hypothesis."""
    best = None
    for h in sorted(counts):
        if best is None or counts[h] > counts[best]:
            best = h
    return best


def assign(ths, x, y, uf, vf, fin, c2):
    """The layer with the smallest r2 below c2, the lowest index on a tie,
    else NONE; pixels whose flow is not finite get NONE."""
    best = np.full(x.shape, c2)
    lab = np.full(x.shape, NONE, np.uint8)
    for l, th in enumerate(ths):
        r2 = _r2(th, x, y, uf, vf)
        m = fin & (r2 < best)
        best = np.where(m, r2, best)
        lab = np.where(m, np.uint8(l), lab)
    return lab


def segment(flow, model="affine", max_layers=4, grid=8, passes=4, rounds=3, smooth=2, cutoff=1.0, min_support=0.03,
            weight=None, state=None):
    """of_segment_motion.  Returns a namespace: labels, labels_raw (H, W)
    uint8, n, layers (namespaces with theta, matrix, support, rms, pixels,
    degenerate), and `seen`, the set of branches this run took: "stop" (an
    extraction stopped for lack of support), "discard" (a refitted layer fell
    below the support), "none" (a NONE pixel in the closing assignment),
    "mode" (the filter changed a label), "nohyp" (a cell without a
    hypothesis)."""
    model = mn.MODELS.get(model, model)
    f = np.asarray(flow).astype(np.float32)
    H, W = f.shape[:2]
    fin = np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
    ok = fin.copy()
    if state is not None:
        ok &= np.asarray(state) == 0
    uf = np.where(fin, f[..., 0], np.float32(0)).astype(np.float64)
    vf = np.where(fin, f[..., 1], np.float32(0)).astype(np.float64)
    w0 = np.ones((H, W)) if weight is None else np.asarray(weight).astype(np.float32).astype(np.float64)
    w0 = np.where(ok, w0, 0.0)
    usable = w0 > 0.0
    total = int(usable.sum())
    _, _, _, x, y = mn.frame_coords(H, W)
    c2 = cutoff * cutoff
    thr = min_support * float(total)
    seen = set()

    def below(count):
        return float(count) < thr

    def sums(th, mask, cc):
        """One pass of the fit with every pixel outside `mask` masked by the state."""
        return [mn.ordered_sum(p) for p in _planes(th, x, y, np.where(mask, uf, 0.0), np.where(mask, vf, 0.0),
                                                   np.where(mask, w0, 0.0), cc)]

    # 1. hypotheses: the cells of the pass-0 tile records
    nty, ntx = -(-H // 8), -(-W // 64)
    tv = [mn.tile_values(p).reshape(nty, ntx) for p in _planes([0.0] * 6, x, y, np.where(ok, uf, 0.0),
                                                               np.where(ok, vf, 0.0), w0, None)]
    ch, cw = -(-nty // grid), -(-ntx // grid)
    hyps = {}
    for a in range(grid):
        for b in range(grid):
            r0, r1, q0, q1 = a * ch, min((a + 1) * ch, nty), b * cw, min((b + 1) * cw, ntx)
            if r0 >= r1 or q0 >= q1:
                continue
            S = [mn.group_tree(t[r0:r1, q0:q1].ravel()) for t in tv]
            if S[0] > 0.0:
                hyps[a * grid + b] = mn.solve(S, model)
            else:
                seen.add("nohyp")

    # 2. extraction
    rem = usable.copy()
    ths, lost = [], []
    for _ in range(max_layers):
        counts = {h: int((rem & (_r2(th, x, y, uf, vf) < c2)).sum()) for h, (th, _) in hyps.items()}
        h = pick(counts)
        if h is None or below(counts[h]):
            seen.add("stop")
            break
        th, deg = list(hyps[h][0]), int(hyps[h][1])
        for _ in range(passes):
            S = sums(th, rem, c2)
            if not S[0] > 0.0:
                break
            th, lo = mn.solve(S, model)
            deg |= int(lo)
        inl = rem & (_r2(th, x, y, uf, vf) < c2)
        if below(int(inl.sum())):
            seen.add("discard")
            break
        ths.append(th)
        lost.append(deg)
        rem &= ~inl

    # 3. joint rounds and the closing assignment
    n = len(ths)
    for _ in range(rounds):
        lab = assign(ths, x, y, uf, vf, fin, c2)
        for l in range(n):
            S = sums(ths[l], usable & (lab == l), c2)
            if S[0] > 0.0:
                ths[l], lo = mn.solve(S, model)
                lost[l] |= int(lo)
    raw = assign(ths, x, y, uf, vf, fin, c2)
    closing = [sums(ths[l], usable & (raw == l), c2) for l in range(n)]

    # 4. the mode filter
    labels = mode_filter(raw, n, smooth)
    if (raw == NONE).any():
        seen.add("none")
    if (labels != raw).any():
        seen.add("mode")
    layers = []
    for l in range(n):
        S = closing[l]
        with np.errstate(all="ignore"):
            rms = float(np.sqrt(np.float64(mn._div(S[12], S[0]))))
        layers.append(SimpleNamespace(theta=np.array(ths[l], dtype=np.float64), matrix=mn.matrix_of(ths[l], H, W),
                                      support=S[0], rms=rms, pixels=int((labels == l).sum()), degenerate=lost[l]))
    return SimpleNamespace(labels=labels, labels_raw=raw, n=n, layers=layers, seen=seen)
