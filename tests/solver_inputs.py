"""Seeded linear systems and the case table of the solver shape tests
(test_solver_shapes_cpu.py checks the table's claims without a GPU,
test_gpu_solver_shapes.py runs it).

flow_system   the 5-point + 2x2-coupling system flow_operator assembles, by the
              recipe of test_gpu_stages._spd_flow_system: positive edge weights
              over 4 decades, rank-1 data blocks psi g g^T, diagonal = data +
              incident edge weights.  One term is added to that recipe, and
              only where a pixel has no neighbour (the 1 x 1 level), whose
              rank-1 data block is singular without it: the diagonal coupling
              lambda2 t of the alternating methods' operator (alt_ba's uvhat
              term), 1e-2 .. 1 per unknown.  The 7
              planes are rounded to float32 FIRST and A is built from the
              rounded planes, the rhs is float32 too: the GPU and the float64
              reference see the same numbers.
dia_system    A = sum_q F_q^T diag(w_q) F_q per component + the same data and
              coupling blocks, F_q the valid placements of filter q's taps (a
              filter that does not fit the shape contributes nothing), weights
              over 4 decades; rounded through float32 DIA planes, so
              sparse_to_dia(A) in float32 reproduces A exactly.

Unknown order as methods/base.py: k = j H + i, u block then v block.
"""
import numpy as np

# the filter lists of tests/test_gpu_filters.py (restated: that module is a
# GPU test module)
FILTERS = {
    "diag4": [np.array([[1, -1]]), np.array([[1], [-1]]), np.array([[1, 0], [0, -1]]), np.array([[0, 1], [-1, 0]])],
    "wide": [np.array([[1, -2, 1]]), np.array([[1], [-2], [1]])],
}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _data_blocks(rng, H, W):
    ix, iy = rng.normal(0, 3, (H, W)), rng.normal(0, 3, (H, W))
    psi = 10.0 ** rng.uniform(-1, 1, (H, W))
    return psi * ix * ix, psi * ix * iy, psi * iy * iy


def flow_planes(H, W, seed, couple="isolated"):
    """(7 float32-valued planes, float32-valued rhs of 2 H W entries);
    couple = "all" adds the coupling term to every unknown (the systems
    tools/cgs_t5_seams.py was measured on)"""
    rng = np.random.default_rng(seed)
    coef = np.zeros((7, H, W))
    for pl in range(4):
        coef[pl] = 10.0 ** rng.uniform(-2, 2, (H, W))
    coef[0][:, -1] = coef[2][:, -1] = 0.0   # no edge right of the last column
    coef[1][-1, :] = coef[3][-1, :] = 0.0   # nor below the last row
    a, c, d = _data_blocks(rng, H, W)
    deg = [coef[2 * e].copy() + coef[2 * e + 1] for e in range(2)]
    for e in range(2):
        deg[e][:, 1:] += coef[2 * e][:, :-1]
        deg[e][1:, :] += coef[2 * e + 1][:-1, :]
    b = rng.normal(0, 1, 2 * H * W)
    cu, cv = 10.0 ** rng.uniform(-2, 0, (2, H, W))
    if couple != "all":
        cu, cv = np.where(deg[0] == 0, cu, 0.0), np.where(deg[1] == 0, cv, 0.0)
    coef[4] = a + deg[0] + cu
    coef[5] = c
    coef[6] = d + deg[1] + cv
    return f32(coef), f32(b)


def flow_system(H, W, seed, couple="isolated"):
    from optical_flow.methods.base import planes_to_sparse
    coef, b = flow_planes(H, W, seed, couple)
    return planes_to_sparse(coef).tocsr(), b


def dia_system(H, W, filters, seed):
    from scipy import sparse
    from optical_flow.methods.base import dia_to_sparse, sparse_to_dia
    rng = np.random.default_rng(seed)
    N = H * W
    k = np.arange(N).reshape(W, H).T  # k[i, j] = j H + i
    blocks = []
    for comp in range(2):
        S = sparse.csr_matrix((N, N))
        for f in filters:
            f = np.atleast_2d(np.asarray(f, dtype=float))
            fh, fw = f.shape
            nh, nw = H - fh + 1, W - fw + 1
            w = 10.0 ** rng.uniform(-2, 2, (max(nh, 0), max(nw, 0)))  # drawn whether or not the filter fits
            if nh < 1 or nw < 1:
                continue
            rows, cols, vals = [], [], []
            r = np.arange(nh * nw).reshape(nh, nw)
            for a in range(fh):
                for c in range(fw):
                    if f[a, c] != 0:
                        rows.append(r.ravel())
                        cols.append(k[a:a + nh, c:c + nw].ravel())
                        vals.append(np.full(nh * nw, f[a, c]))
            F = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                                  shape=(nh * nw, N))
            S = S + F.T @ sparse.diags(w.ravel()) @ F
        blocks.append(S)
    a, c, d = _data_blocks(rng, H, W)
    b = rng.normal(0, 1, 2 * N)
    cu, cv = 10.0 ** rng.uniform(-2, 0, (2, H, W))
    fl = lambda p: p.ravel(order="F")  # noqa: E731
    # the coupling term only where no filter placement touches the pixel
    cu = np.where(blocks[0].diagonal().reshape(H, W, order="F") == 0, cu, 0.0)
    cv = np.where(blocks[1].diagonal().reshape(H, W, order="F") == 0, cv, 0.0)
    A = sparse.bmat([[blocks[0] + sparse.diags(fl(a + cu)), sparse.diags(fl(c))],
                     [sparse.diags(fl(c)), blocks[1] + sparse.diags(fl(d + cv))]]).tocsr()
    D, planes = sparse_to_dia(A, H, W)
    return dia_to_sparse(f32(planes), D).tocsr(), f32(b)


def flat(x):
    """(H, W, 2) solution of _solve_linear_system -> A's unknown order"""
    return np.concatenate([x[..., 0].ravel(order="F"), x[..., 1].ravel(order="F")])


def planes(v, H, W):
    """A's unknown order -> (2, H, W)"""
    return np.stack([v[:H * W].reshape(H, W, order="F"), v[H * W:].reshape(H, W, order="F")])


# ---- the case table -----------------------------------------------------------
# (a) K-th iterate.  A case: (kernel, solver, H, W, extra); extra is the
# method's alpha for the 5-point 'backslash' (which Chebyshev interval
# cg_setup picks: alpha < 0.5 -> 0.01, else 0.04) or the filter list of a
# DIA case.  Methods: classic+nl-fast carries alpha = 1.0 (interval 0.04);
# the tests set alpha = 0.0 on it for the robust interval 0.01.
KS = (4, 8)
# gate of the K-th iterate in units of e32: twice the largest GPU error / e32
# measured on an MI355X over the cases below (5.75, k_cg_reg 'backslash' 32x64
# K = 8; test_gpu_solver_shapes.py), rounded up to a power of two
M = 16

# k_cg: shape -> (strips, bands, R) that of_solver_geometry must report
K_CG = {
    (34, 124): (1, 9, 4),      # one full strip; last band 2 rows; last block has one live wave
    (34, 125): (2, 9, 4),      # second strip owns one column; odd W
    (33, 249): (3, 9, 4),      # third strip owns one column; odd W
    (17, 248): (2, 5, 4),      # two full strips
    (70, 63): (1, 18, 4),      # one partly filled strip; odd W
    (5, 1000): (9, 2, 3),      # 9 strips; bands of 3 and 2 rows
    (1, 4100): (34, 1, 1),     # one row; 34 strips
    (4100, 1): (1, 586, 7),    # one column; R = 7
    (2600, 2): (1, 520, 5),    # R = 5
    (3300, 3): (1, 550, 6),    # R = 6
    (5000, 1): (1, 625, 8),    # R = 8
    (130, 2500): (21, 26, 5),  # many strips and R = 5 (the one large case)
}
# k_cgs: the shapes of test_gpu_cgs_strips.py and test_gpu_cgs_edges.py, one
# row, one column -> (strips, bands, R)
K_CGS = {
    (40, 120): (1, 5, 8), (40, 128): (1, 5, 8), (40, 129): (2, 5, 8), (40, 240): (2, 5, 8),
    (40, 241): (3, 5, 8), (40, 353): (4, 5, 8),
    (70, 121): (1, 9, 8), (41, 230): (2, 6, 7), (9, 500): (5, 2, 5),
    (1, 4100): (37, 1, 1), (4100, 1): (1, 456, 9),
}
CGS_BOTH_INTERVALS = (41, 230)  # solved with alpha = 1.0 and alpha = 0.0
K_CG_REG = [(32, 64), (23, 89), (4, 511), (3, 600), (1, 2048), (2048, 1), (1, 70), (70, 1)]  # <= 2048 px
K_CG_SMALL = [(3, 683), (64, 64), (65, 63), (1, 4096), (4096, 1)]  # 2049 .. 4096 px
FIRST_FUSED = (17, 241)  # 4097 px: k_cg / k_cgs, not k_cg_small
DIA_SHAPES = [(1, 70), (70, 1), (3, 3), (37, 65), (60, 1100)]
TINY = [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3)]
SOR_SHAPES = [(1, 70), (70, 1), (2, 3), (65, 40), (64, 36), (64, 37)]
DIA_SOR = [("diag4", 60, 1100), ("diag4", 3, 3), ("wide", 60, 1100), ("wide", 3, 3)]

CG_REG_PX, CG_SMALL_PX = 2048, 4096


# The system of a case is that of salt 1 unless the planted-bug condition of
# test_solver_shapes_cpu.py (a column counted twice and a dropped seam edge each
# move x_K by >= 3 M e32) fails there: then a later salt at which it holds for
# both K (searched 1 .. 24; 1 .. 3 above 50 k pixels).  e32 varies 30-fold with
# the seed on the degree-5 polynomial cases.
CASE_SALT = {
    "k_cg-pcg-130x2500": 2,
    "k_cgs-backslash-40x120": 2,
    "k_cgs-backslash-40x128": 11,
    "k_cgs-backslash-40x129": 12,
    "k_cgs-backslash-40x240": 14,
    "k_cgs-backslash-40x241": 11,
    "k_cgs-backslash-40x353": 11,
    "k_cgs-backslash-70x121": 10,
    "k_cgs-backslash-41x230": 5,
    "k_cgs-backslash-41x230-alpha0": 12,
    "k_cgs-backslash-9x500": 3,
    "k_cgs-backslash-1x4100": 8,
    "k_cgs-backslash-4100x1": 14,
    "k_cg_reg-backslash-32x64": 2,
    "k_cg_reg-backslash-23x89": 2,
    "k_cg_reg-backslash-4x511": 7,
    "k_cg_reg-backslash-3x600": 10,
    "k_cg_reg-backslash-1x2048": 17,
    "k_cg_reg-backslash-2048x1": 7,
    "k_cg_reg-backslash-70x1": 2,
    "k_cg_small-backslash-3x683": 17,
    "k_cg_small-backslash-64x64": 2,
    "k_cg_small-backslash-65x63": 2,
    "k_cg_small-backslash-1x4096": 21,
    "dia_cg-pcg-60x1100-diag4": 2,
    "dia_cg-backslash-60x1100-diag4": 3,
}
# What no salt of that search satisfies at K = 8: the degree-5 polynomial on one
# row or one column of 4096 pixels, where the column is one pixel and e32 is
# large.  K = 4 only there, at which both planted bugs separate.
EXCEPTIONS = {
    "k_cg_small-backslash-1x4096": dict(ks=(4,)),  # column twice / e32 at K = 4, 8: 56.1, 27.1 (the best of 24 salts)
    "k_cg_small-backslash-4096x1": dict(ks=(4,)),  # ... 50.7, 24.5 at salt 1; at most 34.8, 26.1 elsewhere
}


def seed_of(H, W, salt=0):
    return 1000003 * salt + 4099 * H + W


# (b): the converged 'pcg' count may differ from the oracle's by one only if the
# float64 residual at the stopping iteration and at the one before is not
# within 5 % of rtol ||b|| (test_solver_shapes_cpu.py); where the system of
# salt 1 is, the first salt at which it is not
CONVERGED_SALT = {(23, 89): 5, (4, 511): 3, (3, 600): 7, (1, 2048): 3, (2048, 1): 5, (70, 1): 3, (65, 63): 2,
                  (1, 4096): 14, (4096, 1): 7}


def converged_seed(H, W):
    return seed_of(H, W, CONVERGED_SALT.get((H, W), 1))


def iterate_cases():
    """every (a) case: dict(kernel, solver, H, W, alpha, filt, ks)"""
    out = []

    def add(kernel, solver, H, W, alpha=1.0, filt=None):
        c = dict(kernel=kernel, solver=solver, H=H, W=W, alpha=alpha, filt=filt, ks=KS, dup=True)
        c.update(EXCEPTIONS.get(case_id(c), {}))
        out.append(c)

    for H, W in K_CG:
        add("k_cg", "pcg", H, W)
    for H, W in K_CGS:
        add("k_cgs", "backslash", H, W)
        if (H, W) == CGS_BOTH_INTERVALS:
            add("k_cgs", "backslash", H, W, alpha=0.0)
    for kernel, shapes in (("k_cg_reg", K_CG_REG), ("k_cg_small", K_CG_SMALL)):
        for H, W in shapes:
            add(kernel, "pcg", H, W)
            add(kernel, "backslash", H, W)
    add("k_cg", "pcg", *FIRST_FUSED)
    add("k_cgs", "backslash", *FIRST_FUSED)
    for tag in ("diag4", "wide"):
        for H, W in DIA_SHAPES:
            add("dia_cg", "pcg", H, W, filt=tag)
            add("dia_cg", "backslash", H, W, filt=tag)
    return out


def case_id(c):
    s = f"{c['kernel']}-{c['solver']}-{c['H']}x{c['W']}"
    if c["filt"]:
        s += "-" + c["filt"]
    if c["alpha"] != 1.0:
        s += f"-alpha{c['alpha']:g}"
    return s


def case_system(c, salt=None):
    """(A, b) of a case: salt 1 unless CASE_SALT names another"""
    seed = seed_of(c["H"], c["W"], salt or CASE_SALT.get(case_id(c), 1))
    if c["filt"]:
        return dia_system(c["H"], c["W"], FILTERS[c["filt"]], seed)
    return flow_system(c["H"], c["W"], seed)


def is_five_point(A, H, W):
    """whether _solve_linear_system sends A to the 5-point solvers (of_solve)
    rather than the DIA ones: diag4 on one row or one column is a 5-point
    operator"""
    from optical_flow.methods.base import sparse_to_planes
    try:
        sparse_to_planes(A, H, W)
    except NotImplementedError:
        return False
    return True


def case_precond(c, A):
    """(precond, poly_a) of the solver a case reaches"""
    if c["solver"] == "pcg":
        return "jacobi", None
    if c["filt"] and not is_five_point(A, c["H"], c["W"]):
        return "block", None  # gen_solve: 2x2 block Jacobi
    from solver_numpy import poly_interval
    return "poly5", poly_interval(c["alpha"])


def case_seam(c):
    """(axis, at): the column (axis 1) or row (axis 0) the planted bugs sit at:
    the last column the first strip owns (k_cg 123, k_cgs 119) where the level
    is wider than that, else the middle column; for one column the last row of
    the first band (fused kernels) or the middle row"""
    H, W = c["H"], c["W"]
    sw = {"k_cg": 124, "k_cgs": 120}.get(c["kernel"])
    if W > 1:
        return 1, sw - 1 if sw and W > sw else (W - 1) // 2
    R = {"k_cg": K_CG, "k_cgs": K_CGS}[c["kernel"]][(H, W)][2] if sw else H // 2
    return 0, R - 1
