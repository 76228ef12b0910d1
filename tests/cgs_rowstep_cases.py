"""Cases and fixtures of test_gpu_cgs_rowstep.py: K-th iterates of the
'backslash' solver (k_cgs) that must stay bit for bit what the commit before
the row-step change computed.

The fixtures under tests/golden/ were recorded on an MI355X from that commit
with tools/cgs_rowstep_record.py: cgs_rowstep_sha1.json holds the sha1 of the
float32 bytes of every iterate (and the iteration count the solve reported),
cgs_rowstep_iterates.npz the float32 iterates themselves for the two smallest
shapes, so that a mismatch there can be located pixel by pixel.

Shapes (the smallest at which each thing the change moves can go wrong):

  41 x 230   two strips; several bands, the odd ones flipped; a short last
             band; image rows above and below the walk
  17 x 241   odd width (the ODD instances); two bands
  70 x 121   one strip that owns all 128 lanes; nine bands, so the ring
             counter wraps many times across flips
  9 x 500    few rows per band, five strips; the whole walk is fill and drain
  1 x 4100   every neighbour row of the walk is outside the image
  4100 x 1   the band count capped by the block target; long bands; the
             wrap at CGS_NREC hundreds of times

Each with the quadratic operator (alpha = 1.0, Chebyshev interval [0.04, 2])
and the robust one (alpha = 0.0, [0.01, 2]) at K = 1 (the FIRST instance), 2
and 8; K = 20 on 41 x 230.  'fallback' is the 41 x 230 operator with a_uv set
on a handful of pixels so that a d - c^2 <= 0 there: cg_inv<true> takes the
scalar-Jacobi inverse on those lanes.  With rtol 0 the residual replacement
never acts (its threshold is sqrt(rtol)), so 'converged' adds one solve with
the default tolerances, which runs past launch 16 and through the x_lo = 0
path; its iteration count is compared too.
"""
import hashlib
import json
import os

import numpy as np

import solver_inputs as SI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHA1_FILE = os.path.join(GOLDEN, "cgs_rowstep_sha1.json")
NPZ_FILE = os.path.join(GOLDEN, "cgs_rowstep_iterates.npz")

SHAPES = [(41, 230), (17, 241), (70, 121), (9, 500), (1, 4100), (4100, 1)]
ALPHAS = (1.0, 0.0)
KS = (1, 2, 8)
LONG_SHAPE, LONG_K = (41, 230), 20
ARRAY_SHAPES = sorted(SHAPES, key=lambda s: s[0] * s[1])[:2]  # iterates kept as arrays
# (row, column) of the pixels whose 2x2 block is made indefinite: first and
# last pixel, both sides of the strip seam (columns 119 / 120), halo lanes of
# both strips, flipped and unflipped bands
FALLBACK_PX = [(0, 0), (5, 7), (13, 118), (20, 119), (22, 120), (30, 64), (33, 113), (40, 229)]


def cases():
    """dict(id, H, W, alpha, K, kind); K None: default tolerances"""
    out = []
    for H, W in SHAPES:
        for a in ALPHAS:
            ks = KS + ((LONG_K,) if (H, W) == LONG_SHAPE else ())
            for K in ks:
                out.append(dict(id=f"{H}x{W}-alpha{a:g}-K{K}", H=H, W=W, alpha=a, K=K, kind="plain"))
    H, W = LONG_SHAPE
    for K in KS:
        out.append(dict(id=f"{H}x{W}-fallback-K{K}", H=H, W=W, alpha=1.0, K=K, kind="fallback"))
    out.append(dict(id=f"{H}x{W}-converged", H=H, W=W, alpha=1.0, K=None, kind="plain"))
    return out


def system(H, W, kind):
    """(A, b) of a shape: the seeded flow system of solver_inputs, for
    'fallback' with c = 1.25 sqrt(a d) at FALLBACK_PX"""
    from optical_flow.methods.base import planes_to_sparse
    coef, b = SI.flow_planes(H, W, SI.seed_of(H, W, 1))
    if kind == "fallback":
        for i, j in FALLBACK_PX:
            coef[5, i, j] = 1.25 * np.sqrt(coef[4, i, j] * coef[6, i, j])
        coef = SI.f32(coef)
        a, c, d = (coef[p][tuple(zip(*FALLBACK_PX))] for p in (4, 5, 6))
        assert np.all(a * d - c * c < 0)
    return planes_to_sparse(coef).tocsr(), b


def solve(c, A, b):
    """(float32 iterate in A's unknown order, reported iterations, kernels run)"""
    import ctypes as C
    from optical_flow import _native as nat
    from optical_flow.methods.config import load_of_method
    o = load_of_method("classic+nl-fast")
    o.solver = "backslash"
    o.alpha = c["alpha"]
    if c["K"] is not None:
        o.backslash_rtol, o.backslash_maxiter = 0.0, c["K"]
    ctx = nat.context()
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    try:
        x = o._solve_linear_system(A, b, (c["H"], c["W"], 2))
        n = C.c_int(0)
        names = (C.c_char_p * 256)()
        ctx.check(ctx.lib.of_kernel_times(ctx.handle, 256, names, None, None, None, C.byref(n)))
        ran = {names[i].decode() for i in range(min(n.value, 256))}
    finally:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return np.ascontiguousarray(SI.flat(x), dtype=np.float32), int(o.last_solve["iters"]), ran


def digest(x):
    assert x.dtype == np.float32
    return hashlib.sha1(x.tobytes()).hexdigest()


def load_fixtures():
    with open(SHA1_FILE) as f:
        sha = json.load(f)
    with np.load(NPZ_FILE) as z:
        arrays = {k: z[k] for k in z.files}
    return sha, arrays
