"""Plain numpy / scipy statements of the linear solvers, for the solver shape
tests (test_solver_shapes_cpu.py, test_gpu_solver_shapes.py).  No GPU, no
project code beyond the sparse layout: A is the 2N x 2N scipy matrix of
methods/base.py (pixel index k = j H + i, u block then v block).

cg_iterates   textbook preconditioned CG from x = 0 for exactly K iterations
              (no stopping test), in float64 (the reference) or float32 (the
              yardstick e32: A, the vectors, alpha and beta in float32, dot
              products accumulated in float64 as the kernels do), with the
              three preconditioners of the GPU solvers and two planted bugs
cg_stop       scipy's control flow (stop when ||r|| < rtol ||b|| before an
              iteration) with the residual history
sor_lex       lexicographic SOR (base.py:138-172) of any A in its own
              ordering, each sweep one sparse triangular solve; sor_ratios
              gives the stopping figure of every sweep
cheb_poly     the coefficients of the degree-m polynomial preconditioner,
              restated from cheb_poly in csrc/host_solve.hip
"""
import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

CG_DEG = 5                 # csrc/kernels_solve.hip
CG_CHEB_A = 0.04           # csrc/host_solve.hip: method alpha >= 0.5
CG_CHEB_A_ROBUST = 0.01    # ... alpha < 0.5 (the robust GNC stages)


def cheb_poly(m, a, b=2.0):
    """c_0..c_m of M^-1 = sum_i c_i B^i D^-1, B = I - X, X = D^-1 A: the
    Chebyshev residual polynomial 1 - X p(X) = T_{m+1}((b + a - 2X) / (b - a))
    / T_{m+1}((b + a) / (b - a)), re-expanded in powers of B."""
    from math import comb
    T = [np.array([1.0]), np.array([0.0, 1.0])]
    for i in range(2, m + 2):
        t = np.zeros(i + 1)
        t[1:] += 2.0 * T[i - 1]
        t[:i - 1] -= T[i - 2]
        T.append(t)
    t = T[m + 1]
    s, g = (b + a) / (b - a), -2.0 / (b - a)
    Ts = sum(t[k] * s ** k for k in range(m + 2))
    Rx = np.zeros(m + 2)  # R(X) in powers of X
    for k in range(m + 2):
        for j in range(k + 1):
            Rx[j] += t[k] * comb(k, j) * s ** (k - j) * g ** j / Ts
    pX = -Rx[1:]  # p(X) = (1 - R(X)) / X
    return np.array([sum(pX[j] * comb(j, i) * (-1.0) ** i for j in range(i, m + 1)) for i in range(m + 1)])


def poly_interval(alpha):
    """lower end of the Chebyshev interval that cg_setup (host_solve.hip)
    picks from the method's alpha"""
    return CG_CHEB_A_ROBUST if alpha < 0.5 else CG_CHEB_A


def _blocks(A):
    """(a, c, d) of the 2x2 pixel blocks of A"""
    n = A.shape[0] // 2
    dg = A.diagonal()
    c = np.asarray(A.tocsr()[np.arange(n), n + np.arange(n)]).ravel()
    return dg[:n], c, dg[n:]


def drop_seam(A, H, W, axis, at):
    """A without the entries that couple column `at` to column `at + 1`
    (axis 1) or row `at` to row `at + 1` (axis 0): the operator of a kernel
    whose halo lane (row) at that seam reads 0.  The diagonal is kept."""
    N = H * W
    A = sparse.coo_matrix(A)
    pos = [(A.row % N) % H, (A.row % N) // H], [(A.col % N) % H, (A.col % N) // H]
    pr, pc = pos[0][axis], pos[1][axis]
    cut = (A.row // N == A.col // N) & (((pr == at) & (pc == at + 1)) | ((pr == at + 1) & (pc == at)))
    return sparse.csr_matrix((np.where(cut, 0.0, A.data), (A.row, A.col)), shape=A.shape)


def line_indices(H, W, axis, at):
    """unknowns (u and v) of column `at` (axis 1) or row `at` (axis 0)"""
    N = H * W
    k = np.arange(N)
    sel = k[(k // H if axis == 1 else k % H) == at]
    return np.concatenate([sel, N + sel])


class _Precond:
    """z = M^-1 r in `dtype` arithmetic: 'jacobi', 'block' or 'poly5'"""

    def __init__(self, A, kind, dtype, poly_a, A_op):
        f = dtype
        a, c, d = (v.astype(f) for v in _blocks(A))
        self.n = a.size
        self.kind = kind
        if kind == "jacobi":  # base.py:129-131
            with np.errstate(divide="ignore"):
                self.ia = np.where(np.abs(a) > 1e-12, f(1) / a, f(0)).astype(f)
                self.id = np.where(np.abs(d) > 1e-12, f(1) / d, f(0)).astype(f)
            self.ic = np.zeros_like(a)
            return
        det = a * d - c * c
        assert np.all(det > 0), "singular 2x2 block"
        self.ia, self.ic, self.id = (d / det).astype(f), (-c / det).astype(f), (a / det).astype(f)
        if kind == "poly5":
            # the float32 coefficients the kernels are handed
            self.c = cheb_poly(CG_DEG, poly_a).astype(np.float32).astype(f)
            n = self.n
            i = np.arange(n)
            D = sparse.csr_matrix((np.concatenate([a, d, c, c]),
                                   (np.concatenate([i, n + i, i, n + i]), np.concatenate([i, n + i, n + i, i]))),
                                  shape=A.shape)
            self.N = (D - A_op.astype(f)).tocsr().astype(f)  # A = D - N

    def dinv(self, r):
        n = self.n
        return np.concatenate([self.ia * r[:n] + self.ic * r[n:], self.ic * r[:n] + self.id * r[n:]])

    def __call__(self, r):
        y = self.dinv(r)
        if self.kind != "poly5":
            return y
        c = self.c
        g = c[CG_DEG - 1] * y + c[CG_DEG] * self.dinv(self.N @ y)  # Horner in B = D^-1 N
        for i in range(CG_DEG - 2, -1, -1):
            g = c[i] * y + self.dinv(self.N @ g)
        return g


def cg_iterates(A, b, K, precond, dtype=np.float64, poly_a=None, dup=None, drop=None):
    """x_K and ||r_K|| / ||b|| of preconditioned CG from x = 0 after exactly K
    iterations.  Planted bugs (this reference only): `dup`, indices of the
    unknowns every dot product counts twice; `drop`, the operator that takes
    A's place in every stencil application (drop_seam), D staying A's."""
    f = np.dtype(dtype).type
    A_op = sparse.csr_matrix(A if drop is None else drop).astype(f)
    M = _Precond(sparse.csr_matrix(A), precond, f, poly_a, A_op)
    wgt = np.ones(A.shape[0])
    if dup is not None:
        wgt[dup] = 2.0

    def dot(u, v):  # float64 accumulation of the dtype products' operands
        return float(np.dot(u.astype(np.float64) * wgt, v.astype(np.float64)))

    b = np.asarray(b).astype(f)
    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    rho_prev = 1.0
    for it in range(K):
        z = M(r)
        rho = dot(r, z)
        beta = f(0) if it == 0 else f(rho / rho_prev)
        p = z + beta * p
        q = A_op @ p
        pq = dot(p, q)
        if not (pq > 0 and rho > 0):
            break  # converged exactly: nothing left to divide
        alpha = f(rho / pq)
        x = x + alpha * p
        r = r - alpha * q
        rho_prev = rho
    assert x.dtype == f and r.dtype == f
    bn = np.linalg.norm(b.astype(np.float64))
    return x, float(np.linalg.norm(r.astype(np.float64)) / bn) if bn > 0 else 0.0


def cg_stop(A, b, rtol, maxiter, precond="jacobi"):
    """scipy.sparse.linalg.cg's control flow in float64: (iterations,
    [||r_0||, ||r_1||, ...] up to the iterate it stopped at)."""
    A = sparse.csr_matrix(A)
    M = _Precond(A, precond, np.float64, None, A)
    b = np.asarray(b, dtype=np.float64)
    atol = rtol * np.linalg.norm(b)
    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    hist = [float(np.linalg.norm(r))]
    rho_prev = 1.0
    it = 0
    while it < maxiter and hist[-1] >= atol and hist[-1] > 0:
        z = M(r)
        rho = float(r @ z)
        p = z + (0.0 if it == 0 else rho / rho_prev) * p
        q = A @ p
        alpha = rho / float(p @ q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho
        hist.append(float(np.linalg.norm(r)))
        it += 1
    return it, hist


def _sor_sweeps(A, b, omega):
    """generator of (x, ||x - x_old|| / ||x||) after each lexicographic sweep"""
    A = sparse.csr_matrix(A, dtype=np.float64)
    dg = A.diagonal()
    assert np.all(np.abs(dg) >= 1e-15)
    low = (sparse.tril(A, -1) + sparse.diags(dg / omega)).tocsc()
    rest = (sparse.triu(A, 1) + sparse.diags((1.0 - 1.0 / omega) * dg)).tocsr()
    lu = splu(low, permc_spec="NATURAL", diag_pivot_thresh=0.0, options={"SymmetricMode": False})
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    while True:
        xn = lu.solve(b - rest @ x)
        dn, x = np.linalg.norm(xn - x), xn
        yield x, dn / np.linalg.norm(x)


def sor_lex(A, b, omega=1.9, tol=1e-2, maxit=10000):
    """Lexicographic SOR in A's own ordering from x = 0, float64:
    (D / omega + L) x_new = b - (U + (1 - 1 / omega) D) x_old per sweep; stops
    after the sweep with ||x_new - x_old|| < tol ||x_new||.  Returns (x, sweeps)."""
    for it, (x, ratio) in enumerate(_sor_sweeps(A, b, omega), 1):
        if ratio < tol or it >= maxit:
            return x, it


def sor_ratios(A, b, nsweeps, omega=1.9):
    """||x_k - x_{k-1}|| / ||x_k|| of sweeps 1 .. nsweeps, no stopping test"""
    out = []
    for _, ratio in _sor_sweeps(A, b, omega):
        out.append(float(ratio))
        if len(out) == nsweeps:
            return out
