"""numpy float64 restatement of the mask propagation (include/optflow.h, "Mask
propagation"): of_mask_advance operation for operation, in the order the header
writes them, the session built from it by hand, and the recoloured scene of the
quality tests with its layered flows.  Test helper, not a conftest."""
import numpy as np

import inpaint_numpy as ip
from fuse_numpy import bil
from track_numpy import inside

CARRIED, VOTED, UNKNOWN, GIVEN = 0, 1, 2, 3
BRANCHES = {"carried", "voted-colour", "voted-count", "unknown", "smooth-flip", "smooth-tie"}


def carry(M, B, S=None):
    """The carried plane A, (H, W) float32: (float)bil(M != 0) where the flow
    decides, -1 elsewhere."""
    m = (np.asarray(M) != 0).astype(np.float64)
    H, W = m.shape
    F = np.asarray(B).astype(np.float32)
    ii, jj = np.mgrid[0:H, 0:W]
    fin = np.isfinite(F[..., 0]) & np.isfinite(F[..., 1])
    with np.errstate(all="ignore"):
        u, v = F[..., 0].astype(np.float64), F[..., 1].astype(np.float64)
        r, q = ii + v, jj + u
        ok = fin & inside(r, q, H, W)
    if S is not None:
        ok &= np.asarray(S) == 0
    A = np.full((H, W), np.float32(-1.0), np.float32)
    A[ok] = bil(m, r[ok], q[ok]).astype(np.float32)
    return A


def vote(A, G, R, rng_, seen=None):
    """(labels, status) of every pixel from the carried plane and the guide."""
    H, W = A.shape
    G = np.asarray(G).astype(np.float32).astype(np.float64).reshape(H, W, -1)
    C = G.shape[2]
    lab = (A >= np.float32(0.5)).astype(np.uint8)
    st = np.full((H, W), CARRIED, np.uint8)
    ui, uj = np.nonzero(A < 0)
    if seen is not None and (A >= 0).any():
        seen.add("carried")
    if ui.size == 0:
        return lab, st
    n = ui.size
    num, den = np.zeros(n), np.zeros(n)
    cnt, ones = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rr = float(rng_) * float(rng_)
    gp = G[ui, uj]
    for di in range(-R, R + 1):
        for dj in range(-R, R + 1):
            y, x = ui + di, uj + dj
            inf = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
            an = A[yc, xc]
            ok = inf & (an >= 0)
            gn = G[yc, xc]
            with np.errstate(all="ignore"):
                D = np.zeros(n)
                for c in range(C):
                    d = gp[:, c] - gn[:, c]
                    D = D + d * d
                D = D / float(C)
                z = D / rr
                w = np.where(z < 1.0, (1.0 - z) * (1.0 - z), 0.0)
            w = np.where(ok, w, 0.0)          # adding 0.0 to a sum that is never negative changes no bit
            num = num + w * np.where(ok, an, np.float32(0.0)).astype(np.float64)
            den = den + w
            cnt += ok
            ones += ok & (an >= np.float32(0.5))
    by_colour, by_count = den > 0.0, (den <= 0.0) & (cnt > 0)
    none = ~by_colour & ~by_count
    l = np.zeros(n, np.uint8)
    l[by_colour] = num[by_colour] >= 0.5 * den[by_colour]
    l[by_count] = 2 * ones[by_count] >= cnt[by_count]
    lab[ui, uj] = l
    st[ui, uj] = np.where(none, UNKNOWN, VOTED)
    if seen is not None:
        for name, hit in (("voted-colour", by_colour), ("voted-count", by_count), ("unknown", none)):
            if hit.any():
                seen.add(name)
    return lab, st


def mode(lab, s, seen=None):
    """One pass of the mode filter of radius s over labels 0 / 1."""
    if s == 0:
        return lab.copy()
    H, W = lab.shape
    k = np.zeros((H, W), np.int64)
    n = np.zeros((H, W), np.int64)
    p1 = np.pad(lab.astype(np.int64), s)
    pn = np.pad(np.ones((H, W), np.int64), s)
    for a in range(2 * s + 1):
        for b in range(2 * s + 1):
            k += p1[a:a + H, b:b + W]
            n += pn[a:a + H, b:b + W]
    out = np.where(2 * k > n, 1, np.where(2 * k < n, 0, lab)).astype(np.uint8)
    if seen is not None:
        if (out != lab).any():
            seen.add("smooth-flip")
        if (2 * k == n).any():
            seen.add("smooth-tie")
    return out


def advance(M, G, B, S=None, vote_radius=8, vote_range=20.0, smooth=1, seen=None):
    """of_mask_advance: (mask (H, W) uint8 0 / 1, status (H, W) uint8).  G
    (H, W) or (H, W, C), B (H, W, 2) current -> previous, S (H, W) or None.
    `seen`, a set, collects the branches that occurred."""
    lab, st = vote(carry(M, B, S), G, vote_radius, vote_range, seen)
    return mode(lab, smooth, seen), st


def session(frames, keys, pair_fn, advance_fn):
    """The session by hand: frame k with keys[k] (a mask or None) pushed in
    order.  pair_fn(previous, this) -> (bw, state_bw); advance_fn(mask, frame,
    bw, state_bw) -> (mask, status).  Returns [(mask, status)] by frame."""
    out = []
    mask = None
    for k, (f, m) in enumerate(zip(frames, keys)):
        if m is not None:
            mask = (np.asarray(m) != 0).astype(np.uint8)
            out.append((mask, np.full(mask.shape, GIVEN, np.uint8)))
        else:
            bw, sb = pair_fn(frames[k - 1], f)
            mask, st = advance_fn(mask, f, bw, sb)
            out.append((mask, st))
    return out


# ---- the scene of the quality tests -----------------------------------------
def recolour(frames, masks):
    """The scene's frames with the object bright and the background dark, the
    texture kept at a quarter and a third of its contrast."""
    return [np.where(np.asarray(m) != 0, 200.0 + 0.25 * (f.astype(np.float64) - 128.0),
                     90.0 + 0.35 * (f.astype(np.float64) - 128.0)).astype(np.float32) for f, m in zip(frames, masks)]


def scene(seed=0, recoloured=True):
    """(frames, masks, bw, states, truth) of inpaint_numpy.scene(seed), the
    frames and the truth recoloured (or not).  bw[s], states[s] for s = 1 .. 8
    (index 0 is None): the layered flow frame s -> s-1, the scene's background
    flow on the background and the rectangle's integer step on the rectangle,
    and its state: 1 where a background pixel lands (bil > 0) under the previous
    rectangle, 2 where it lands outside the frame, else 0."""
    frames, masks, _, bwf, truth = ip.scene(seed)
    H, W = masks[0].shape
    ii, jj = np.mgrid[0:H, 0:W]
    bw, states = [None], [None]
    for s in range(1, len(frames)):
        x0, y0 = int(round(ip.OBJ_X0 + ip.OBJ_V[0] * s)), int(round(ip.OBJ_Y0 + ip.OBJ_V[1] * s))
        xp, yp = int(round(ip.OBJ_X0 + ip.OBJ_V[0] * (s - 1))), int(round(ip.OBJ_Y0 + ip.OBJ_V[1] * (s - 1)))
        obj = masks[s] != 0
        f = bwf[s - 1].copy()
        f[obj] = np.float32([xp - x0, yp - y0])
        r, q = ii + f[..., 1].astype(np.float64), jj + f[..., 0].astype(np.float64)
        ins = inside(r, q, H, W)
        st = np.zeros((H, W), np.uint8)
        st[~obj & ~ins] = 2
        land = np.zeros((H, W), bool)
        land[ins] = bil((masks[s - 1] != 0).astype(np.float64), r[ins], q[ins]) > 0
        st[~obj & ins & land] = 1
        bw.append(f)
        states.append(st)
    if recoloured:
        truth = recolour(truth, [np.zeros_like(m) for m in masks])
        frames = recolour(frames, masks)
    return frames, masks, bw, states, truth


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    u = (a | b).sum()
    return float((a & b).sum()) / float(u) if u else 1.0
