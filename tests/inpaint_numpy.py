"""numpy float64 restatement of the flow-guided video inpainting
(include/optflow.h, "Flow-guided video inpainting"): the grown mask, the pair
weight and of_inpaint_fill operation for operation, in the order the header
writes them, the session's schedule built from them, and the synthetic scene of
the quality tests.  Test helper, not a conftest."""
import numpy as np

from fuse_numpy import bil
from track_numpy import inside

KEPT, FILLED, UNFILLED = 0, 1, 2
# how a walk of a hole pixel ended (fill's `ends`): 0 for a pixel outside the grown mask
HIT, END_NAN, END_OUT, END_HOPS = 1, 2, 3, 4


def grow(M, g):
    """grow(M, g): (H, W) uint8, 1 where any M != 0 within g pixels per axis
    inside the frame.  Rows, then columns: the same set as the square window."""
    M = np.asarray(M) != 0
    H, W = M.shape
    rows = np.zeros((H, W), bool)
    p = np.pad(M, ((0, 0), (g, g)))
    for b in range(2 * g + 1):
        rows |= p[:, b:b + W]
    out = np.zeros((H, W), bool)
    p = np.pad(rows, ((g, g), (0, 0)))
    for a in range(2 * g + 1):
        out |= p[a:a + H]
    return out.astype(np.uint8)


def grow_union(A, B, g):
    return grow((np.asarray(A) != 0) | (np.asarray(B) != 0), g)


def pair_weight(mask_a, mask_b, grow_=2, margin=4):
    """The pair weight of two frames' masks as drawn: (H, W) float32."""
    D = grow_union(grow(mask_a, grow_), grow(mask_b, grow_), margin)
    return np.where(D != 0, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def _walk(flows, targets, ii, jj):
    """One walk of the hole pixels (ii, jj): flows[d-1] and targets[d-1] = (D,
    I) of hop d.  Returns (hops (n,) int, colour (n, C) float64, end (n,))."""
    H, W = targets[0][0].shape if targets else (0, 0)
    n = ii.size
    r, q = ii.astype(np.float64), jj.astype(np.float64)
    live = np.ones(n, bool)
    hops = np.zeros(n, np.int64)
    end = np.full(n, END_HOPS, np.int64)
    col = np.zeros((n, targets[0][1].shape[2] if targets else 1))
    for d, (F, (Dt, It)) in enumerate(zip(flows, targets), start=1):
        L = np.flatnonzero(live)
        if L.size == 0:
            break
        with np.errstate(all="ignore"):
            u, v = bil(F[..., 0], r[L], q[L]), bil(F[..., 1], r[L], q[L])
            fin = np.isfinite(u) & np.isfinite(v)
            rn, qn = r[L] + v, q[L] + u
            ins = fin & inside(rn, qn, H, W)
        end[L[~fin]] = END_NAN
        end[L[fin & ~ins]] = END_OUT
        live[L[~ins]] = False
        L, rn, qn = L[ins], rn[ins], qn[ins]
        r[L], q[L] = rn, qn
        i0, j0 = np.floor(rn).astype(np.int64), np.floor(qn).astype(np.int64)
        i1, j1 = np.minimum(i0 + 1, H - 1), np.minimum(j0 + 1, W - 1)
        clear = (Dt[i0, j0] | Dt[i0, j1] | Dt[i1, j0] | Dt[i1, j1]) == 0
        Lh = L[clear]
        col[Lh] = bil(It, rn[clear], qn[clear])
        hops[Lh] = d
        end[Lh] = HIT
        live[Lh] = False
    return hops, col, end


def fill(frames, masks, fw, bw, t, radius=8, grow_=2, seen=None):
    """of_inpaint_fill: (out float32 in the frames' shape, status (H, W) uint8,
    hops (2, H, W) uint8, ends (2, H, W) uint8: how each walk ended).  `seen`,
    a set, collects the branches that occurred."""
    T = len(frames)
    I = [np.asarray(f).astype(np.float32).astype(np.float64) for f in frames]
    shape = I[0].shape
    I = [f[..., None] if f.ndim == 2 else f for f in I]
    D = [grow(m, grow_) for m in masks]
    F = [np.asarray(f).astype(np.float32).astype(np.float64) for f in fw]
    B = [np.asarray(f).astype(np.float32).astype(np.float64) for f in bw]
    H, W = D[t].shape
    out = np.asarray(frames[t]).astype(np.float32).reshape(I[t].shape).copy()
    status = np.zeros((H, W), np.uint8)
    hops = np.zeros((2, H, W), np.uint8)
    ends = np.zeros((2, H, W), np.uint8)
    ii, jj = np.nonzero(D[t])
    if ii.size:
        nf = [s for s in range(t + 1, min(t + radius, T - 1) + 1)]
        nb = [s for s in range(t - 1, max(t - radius, 0) - 1, -1)]
        df, cf, ef = _walk([F[s - 1] for s in nf], [(D[s], I[s]) for s in nf], ii, jj)
        db, cb, eb = _walk([B[s] for s in nb], [(D[s], I[s]) for s in nb], ii, jj)
        both, onlyf, onlyb = (df > 0) & (db > 0), (df > 0) & (db == 0), (df == 0) & (db > 0)
        with np.errstate(all="ignore"):
            mix = (db[:, None].astype(np.float64) * cf + df[:, None].astype(np.float64) * cb) \
                / (df + db)[:, None].astype(np.float64)
        val = out[ii, jj].copy()
        val[both] = mix[both].astype(np.float32)
        val[onlyf] = cf[onlyf].astype(np.float32)
        val[onlyb] = cb[onlyb].astype(np.float32)
        out[ii, jj] = val
        none = (df == 0) & (db == 0)
        status[ii, jj] = np.where(none, UNFILLED, FILLED)
        hops[0, ii, jj], hops[1, ii, jj] = df, db
        ends[0, ii, jj], ends[1, ii, jj] = ef, eb
        if seen is not None:
            seen |= {"both"} if both.any() else set()
            seen |= {"forward"} if onlyf.any() else set()
            seen |= {"backward"} if onlyb.any() else set()
            for code, name in ((END_NAN, "nan"), (END_OUT, "out"), (END_HOPS, "hops")):
                if (none & ((ef == code) | (eb == code))).any():
                    seen.add("unfilled-" + name)
    if seen is not None and (D[t] == 0).any():
        seen.add("kept")
    return out.reshape(shape), status, hops, ends


def session(frames, masks, radius=8, grow_=2, margin=4, weight_fn=pair_weight, pair_fn=None, fill_fn=None):
    """The session's schedule: pair j is estimated with weight_fn(masks[j],
    masks[j+1], grow, margin) by pair_fn(frame_j, frame_j+1, w) -> (fw, bw);
    frame t comes from fill_fn(frames, masks, fw, bw, t, radius, grow) ->
    (out, status).  Returns (outputs by frame, the (push, index) order in which
    they are emitted: push k emits k - radius, the flush the rest)."""
    T = len(frames)
    fw, bw = [], []
    for j in range(T - 1):
        f, b = pair_fn(frames[j], frames[j + 1], weight_fn(masks[j], masks[j + 1], grow_, margin))
        fw.append(f)
        bw.append(b)
    outs = [fill_fn(frames, masks, fw, bw, t, radius, grow_) for t in range(T)]
    order = [(k, k - radius) for k in range(T) if k >= radius] + [("flush", t) for t in range(max(T - radius, 0), T)]
    return outs, order


# ---- the scene of the quality tests -----------------------------------------
SCENE_T, SCENE_H, SCENE_W = 9, 48, 64
BG_V = (1.3, -0.7)    # frame s samples the background at (x, y) + s * BG_V
OBJ_V = (3.1, 0.4)    # the rectangle's
OBJ_W, OBJ_H, OBJ_X0, OBJ_Y0 = 14, 18, 10, 14


def _texture(rng, x, y):
    a = rng.uniform(10.0, 30.0, 12)
    fx = rng.uniform(0.05, 0.45, 12) * rng.choice([-1.0, 1.0], 12)
    fy = rng.uniform(0.05, 0.45, 12) * rng.choice([-1.0, 1.0], 12)
    p = rng.uniform(0.0, 2.0 * np.pi, 12)
    out = np.full(np.broadcast(x, y).shape, 128.0)
    for k in range(12):
        out = out + a[k] * np.sin(fx[k] * x + fy[k] * y + p[k])
    return out


def scene(seed=0):
    """(frames, masks, fw, bw, truth): 9 frames of 48 x 64; the background, 128
    plus 12 sinusoids of amplitude 10..30 and frequency 0.05..0.45, is sampled
    at (x + 1.3 s, y - 0.7 s) in frame s; a textured 14-wide, 18-tall rectangle
    starting at column 10, row 14 moves by (3.1, 0.4) px per frame over it and
    is the mask.  fw / bw: the background's flows everywhere, so that
    I_s(x, y) = I_s+1(x + u, y + v) on the background.  truth: the frames
    without the rectangle.  (Sampled at (x - 1.3 s, y + 0.7 s) instead, the
    rectangle moves only (1.8, 1.1) px per frame against the background and
    cannot clear its own 14 pixels in 4 hops: 76 % filled at radius 4, where
    the prototype of this scene filled every pixel.)"""
    yy, xx = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)
    frames, masks, truth = [], [], []
    for s in range(SCENE_T):
        bg = _texture(np.random.default_rng(seed), xx + BG_V[0] * s, yy + BG_V[1] * s)
        x0, y0 = int(round(OBJ_X0 + OBJ_V[0] * s)), int(round(OBJ_Y0 + OBJ_V[1] * s))
        m = np.zeros((SCENE_H, SCENE_W), np.uint8)
        m[y0:y0 + OBJ_H, x0:x0 + OBJ_W] = 1
        obj = 255.0 - _texture(np.random.default_rng(seed + 1), 2.0 * (xx - x0), 2.0 * (yy - y0)) + \
            60.0 * np.sign(np.sin(0.9 * (xx - x0)) * np.sin(0.9 * (yy - y0)))
        truth.append(bg.astype(np.float32))
        frames.append(np.where(m != 0, obj, bg).astype(np.float32))
        masks.append(m)
    u, v = -BG_V[0], -BG_V[1]
    fw = [np.broadcast_to(np.float32([u, v]), (SCENE_H, SCENE_W, 2)).copy() for _ in range(SCENE_T - 1)]
    bw = [np.broadcast_to(np.float32([-u, -v]), (SCENE_H, SCENE_W, 2)).copy() for _ in range(SCENE_T - 1)]
    return frames, masks, fw, bw, truth


def hole_scores(outs, statuses, masks, truth):
    """Over the pixels of the masks as drawn, all frames together: (share with
    status FILLED, mean squared error of the FILLED ones against truth)."""
    n = filled = 0
    err = 0.0
    for o, st, m, tr in zip(outs, statuses, masks, truth):
        hole = np.asarray(m) != 0
        ok = hole & (st == FILLED)
        n += int(hole.sum())
        filled += int(ok.sum())
        err += float(((np.asarray(o, np.float64) - tr.astype(np.float64)) ** 2)[ok].sum())
    return filled / n, err / max(filled, 1)
