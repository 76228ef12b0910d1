"""numpy float64 restatement of the point tracker (include/optflow.h, "Dense
point trajectories"): of_track_advance and of_track_seed operation for
operation, in the order the header writes them, plus a pure-numpy assembler of
trajectories from per-frame snapshots.  Test helper, not a conftest."""
import numpy as np

ALIVE, OCCLUDED, LEFT_FRAME, MOTION_BOUNDARY = 0, 1, 2, 3


def near(x, n):
    """min(max(floor(x + 0.5), 0), n-1) with C's fmax / fmin (NaN gives 0)."""
    return np.fmin(np.fmax(np.floor(x + 0.5), 0.0), float(n - 1)).astype(np.int64)


def inside(r, q, H, W):
    with np.errstate(invalid="ignore"):
        return (q >= 0.0) & (q <= float(W - 1)) & (r >= 0.0) & (r <= float(H - 1))


def bil(A, r, q):
    """The clamped bilinear sample of plane A (float64) at finite (r, q)."""
    H, W = A.shape
    qc = np.minimum(np.maximum(q, 0.0), float(W - 1))
    rc = np.minimum(np.maximum(r, 0.0), float(H - 1))
    qf, rf = np.floor(qc), np.floor(rc)
    j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
    fc, fr = qc - qf, rc - rf
    j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
    return (1.0 - fr) * ((1.0 - fc) * A[i0, j0] + fc * A[i0, j1]) + fr * ((1.0 - fc) * A[i1, j0] + fc * A[i1, j1])


def advance(xy, status, fw, bw, alpha1=0.01, alpha2=0.5, beta1=0.01, beta2=0.002):
    """of_track_advance.  xy (N, 2) float32 {x, y}, status (N,) uint8, flows
    (H, W, 2) holding float32 values.  Returns new (xy, status)."""
    xy = np.array(xy, dtype=np.float32)
    st = np.array(status, dtype=np.uint8)
    F = np.asarray(fw).astype(np.float32).astype(np.float64)
    B = np.asarray(bw).astype(np.float32).astype(np.float64)
    H, W = F.shape[:2]
    out_xy, out_st = xy.copy(), st.copy()
    with np.errstate(all="ignore"):
        for t in range(xy.shape[0]):
            if st[t] != ALIVE:
                continue
            xd, yd = np.float64(xy[t, 0]), np.float64(xy[t, 1])
            if not inside(yd, xd, H, W):
                out_st[t] = LEFT_FRAME
                continue
            u, v = bil(F[..., 0], yd, xd), bil(F[..., 1], yd, xd)
            x1, y1 = xd + u, yd + v
            if not inside(y1, x1, H, W):
                out_st[t] = LEFT_FRAME
                continue
            bu, bv = bil(B[..., 0], y1, x1), bil(B[..., 1], y1, x1)
            du, dv = u + bu, v + bv
            err = du * du + dv * dv
            thr = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2
            if not err <= thr:
                out_st[t] = OCCLUDED
                continue
            i, j = int(near(yd, H)), int(near(xd, W))
            jm, jp, im, ip = max(j - 1, 0), min(j + 1, W - 1), max(i - 1, 0), min(i + 1, H - 1)
            ux, uy = F[i, jp, 0] - F[i, jm, 0], F[ip, j, 0] - F[im, j, 0]
            vx, vy = F[i, jp, 1] - F[i, jm, 1], F[ip, j, 1] - F[im, j, 1]
            g = 0.25 * ((ux * ux + uy * uy) + (vx * vx + vy * vy))
            if not g <= beta1 * (u * u + v * v) + beta2:
                out_st[t] = MOTION_BOUNDARY
                continue
            out_xy[t, 0], out_xy[t, 1] = np.float32(x1), np.float32(y1)
    return out_xy, out_st


def seed_flags(gray, xy, status, step, min_eig):
    """The accept flag of every seeding cell, (nci, ncj) bool."""
    G = np.asarray(gray).astype(np.float32).astype(np.float64)
    H, W = G.shape
    nci, ncj = -(-H // step), -(-W // step)
    occ = np.zeros((nci, ncj), dtype=bool)
    if xy is not None and len(xy):
        p = np.asarray(xy, dtype=np.float32).astype(np.float64)
        alive = np.asarray(status) == ALIVE
        with np.errstate(invalid="ignore"):
            ci, cj = near(p[:, 1], H) // step, near(p[:, 0], W) // step
        occ[ci[alive], cj[alive]] = True
    # every cell at once: the same operations per cell, in the same order
    i, j = np.meshgrid(np.arange(nci) * step + step // 2, np.arange(ncj) * step + step // 2, indexing="ij")
    free = (i < H) & (j < W) & ~occ
    if min_eig == 0:
        return free
    i, j = np.minimum(i, H - 1), np.minimum(j, W - 1)  # cells without a candidate: any pixel, masked below
    Jxx, Jxy, Jyy = np.zeros((nci, ncj)), np.zeros((nci, ncj)), np.zeros((nci, ncj))
    with np.errstate(all="ignore"):
        for da in (-1, 0, 1):
            for db in (-1, 0, 1):
                a, b = np.clip(i + da, 0, H - 1), np.clip(j + db, 0, W - 1)
                gx = 0.5 * (G[a, np.minimum(b + 1, W - 1)] - G[a, np.maximum(b - 1, 0)])
                gy = 0.5 * (G[np.minimum(a + 1, H - 1), b] - G[np.maximum(a - 1, 0), b])
                Jxx = Jxx + gx * gx
                Jxy = Jxy + gx * gy
                Jyy = Jyy + gy * gy
        T, D = Jxx + Jyy, Jxx * Jyy - Jxy * Jxy
        return free & (T >= 2.0 * min_eig) & ((D - min_eig * T) + min_eig * min_eig >= 0.0)


def seed(gray, xy, status, step, max_tracks, min_eig):
    """of_track_seed for a table xy / status (None: empty).  Returns
    (xy_new (n_new, 2) float32, n_dropped)."""
    n = 0 if xy is None else len(xy)
    flags = seed_flags(gray, xy, status, step, float(min_eig))
    ci, cj = np.nonzero(flags)  # row-major order
    pts = np.stack([cj * step + step // 2, ci * step + step // 2], axis=1).astype(np.float32).reshape(-1, 2)
    room = max_tracks - n
    return pts[:room], max(len(pts) - room, 0)


def assemble(snaps):
    """Trajectories from per-frame snapshots [(xy, status, start), ...]:
    (xy (T, N, 2) float32 with NaN outside a track's life, start, length,
    status), written with plain loops."""
    T = len(snaps)
    N = len(snaps[-1][0]) if T else 0
    xy = np.full((T, N, 2), np.nan, dtype=np.float32)
    length = np.zeros(N, dtype=np.int32)
    for t, (p, s, _) in enumerate(snaps):
        for k in range(len(p)):
            if s[k] == ALIVE:
                xy[t, k] = p[k]
                length[k] += 1
    start = np.array(snaps[-1][2], dtype=np.int32) if T else np.zeros(0, np.int32)
    status = np.array(snaps[-1][1], dtype=np.uint8) if T else np.zeros(0, np.uint8)
    return xy, start, length, status
