"""Why k_cgs's K-th iterate was not the textbook one on levels of two or more
bands before its T5 seam fix (tests/test_gpu_solver_shapes.py): a float64 restatement of its iteration
with beta from the rho recurrence, once with q.M^-1 q exact and once with the
T5 term's band-seam edges counted as the kernel counted them.  T5 = v2.N v2
takes each vertical edge once, from the pixel below it in the band's walk;
odd bands walk bottom to top, so the edge between an even band and the odd
band below it is counted by neither and the edge between an odd band and the
even band below it by both (now an odd band takes both of its
seam edges).  Prints, per shape and K, the deviation of x_K
from textbook CG (max-norm, relative to max|x_K|) for both forms beside the
deviation measured on an MI355X before the fix.  CPU only.
usage: python tools/cgs_t5_seams.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "optical-flow-python_amd"),
                os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import solver_inputs as SI  # noqa: E402
import solver_numpy as SN  # noqa: E402

# measured: max|x - x64_K| / max|x64_K| of 'backslash' at K = 4, 8
GPU = {(40, 120): (2.46e-4, 7.71e-5), (40, 128): (2.74e-3, 1.11e-3), (41, 230): (2.65e-3, 2.13e-4),
       (9, 500): (4.63e-3, 7.10e-4), (4100, 1): (4.07e-2, 3.65e-3), (1, 4100): (2.24e-6, 5.51e-6)}


def iterate(A, b, H, W, K, bands, R, seams):
    """x_K of k_cgs's control flow (cg_prologue): alpha = r.z / p.q, beta from
    rho = r.z - 2 alpha q.z + alpha^2 q.M^-1 q, restart on a 10 % drift"""
    M = SN._Precond(A, "poly5", np.float64, SN.CG_CHEB_A, A)
    N, c5, n = M.N.tocsr(), M.c[SN.CG_DEG], H * W
    cols = np.arange(W)

    def seam(v, i):  # sum of w v_a v_b over the edges between rows i and i + 1, u and v
        a, d = cols * H + i, cols * H + i + 1
        return sum(float((np.asarray(N[o + a, o + d]).ravel() * v[o + a] * v[o + d]).sum()) for o in (0, n))

    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    rho_pred = S = q = None
    for k in range(K + 1):
        beta = 0.0
        if k:
            pq, qz, qMq, rz = S
            a = rz / pq
            rho = rz - 2 * a * qz + a * a * qMq
            drift = k >= 2 and not abs(rz - rho_pred) <= 0.1 * rz
            beta, rho_pred = 0.0 if drift else rho / rz, rho
            x, r = x + a * p, r - a * q
        if k == K:
            return x
        z = M(r)
        p = z + beta * p
        q = A @ p
        qMq = float(q @ M(q))
        if seams:
            v2 = M.dinv(N @ M.dinv(N @ M.dinv(q)))
            for bnd in range(bands - 1):  # the seam below band bnd: dropped (even) or doubled (odd)
                e = 2 * c5 * seam(v2, (bnd + 1) * R - 1)
                qMq += -e if bnd % 2 == 0 else e
        S = (float(p @ q), float(q @ z), qMq, float(r @ z))


for (H, W), gpu in GPU.items():
    _, bands, R = SI.K_CGS[(H, W)]
    A, b = SI.flow_system(H, W, SI.seed_of(H, W, 1), couple="all")  # the systems measured then
    for K, g in zip(SI.KS, gpu):
        x64, _ = SN.cg_iterates(A, b, K, "poly5", np.float64, SN.CG_CHEB_A)
        dev = [np.abs(iterate(A, b, H, W, K, bands, R, s) - x64).max() / np.abs(x64).max() for s in (False, True)]
        print(f"{H}x{W} ({bands} bands of {R}) K {K}: exact q.M^-1 q {dev[0]:.2e}  T5 seams as the kernel counted "
              f"them {dev[1]:.2e}  MI355X then {g:.2e}", flush=True)
