"""Band and strip edges of the fused CG iteration (k_cgs).

k_cgs issues the same loads and stores at every row step of its walk and
turns the ones a step does not need (rows of the walk outside the band, x
rows after a residual replacement) into out-of-range buffer offsets, which
the hardware answers with 0 / drops.  A wrong select shows as a row stored
into a neighbouring band or a band row left unwritten, i.e. as a wrong
solution, at the shapes where a walk leaves its band in every way:

  70 x 121  odd width (the ODD instance), 2 strips, 9 bands of 8 rows with a
            last band of 6, odd bands walked bottom to top
  41 x 230  3 strips, 6 bands of 7 rows with a last band of 6
   9 x 500  5 strips, 2 bands of 5 and 4 rows: shorter than the 19-row
            pipeline, so most steps of a walk are outside the band

(of_solver_geometry; all above CG_SMALL_PX = 4096 px, so k_cgs runs.)  Each
shape is solved three times: two independent random H x W systems, and the
2H-row system that stacks them with no edge between the halves (bands of
another height, one of them across the join).  Yardstick as in
test_gpu_stages.test_solve_synthetic_both_cg_paths: 'backslash' within 1e-4
relative error of scipy's direct solve.  For the stacked system each half is
held to that bound against the direct solve of its own H-row system: the
halves are decoupled, so a difference is a store that crossed the join or a
band end.

Seeds: 2 * H * W and 2 * H * W + 1, fixed before the first GPU run, on which
all nine solves took 16 or more iterations (19 to 41; 70 x 121: 23, 19 and
23 stacked; 41 x 230: 21, 27, 26; 9 x 500: 34, 28, 41), so no seed had to be
searched for.  Relative errors measured there: 7e-7 to 4e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(70, 121), (41, 230), (9, 500)]
RTOL = 1e-4


def _spd_flow_planes(H, W, seed):
    """test_gpu_stages._spd_flow_system, returning the coefficient planes: a
    random flow system of the shape flow_operator assembles: positive edge
    weights spanning 4 decades (robust IRLS weights), PSD 2x2 data blocks,
    diagonal = data block + sum of incident edge weights."""
    rng = np.random.default_rng(seed)
    coef = np.zeros((7, H, W))
    for pl in range(4):
        coef[pl] = 10.0 ** rng.uniform(-2, 2, (H, W))
    coef[0][:, -1] = coef[2][:, -1] = 0.0   # no edge right of the last column
    coef[1][-1, :] = coef[3][-1, :] = 0.0   # nor below the last row
    ix, iy = rng.normal(0, 3, (H, W)), rng.normal(0, 3, (H, W))
    psi = 10.0 ** rng.uniform(-1, 1, (H, W))
    deg = [coef[2 * c].copy() + coef[2 * c + 1] for c in range(2)]
    for c in range(2):
        deg[c][:, 1:] += coef[2 * c][:, :-1]
        deg[c][1:, :] += coef[2 * c + 1][:-1, :]
    coef[4] = psi * ix * ix + deg[0]
    coef[5] = psi * ix * iy
    coef[6] = psi * iy * iy + deg[1]
    return coef, rng.normal(0, 1, 2 * H * W)


def _planes(v, H, W):
    """flat (column-major pixels, u block then v block) -> (2, H, W)"""
    return np.stack([v[:H * W].reshape(H, W, order="F"), v[H * W:].reshape(H, W, order="F")])


def _flat(p):
    return np.concatenate([p[0].ravel(order="F"), p[1].ravel(order="F")])


def _gpu_solve(coef, b):
    """'backslash' through the method's _solve_linear_system with the solve
    log on: (solution as (2, H, W) planes, iterations of the logged solve)"""
    from optical_flow import _native
    from optical_flow.methods.base import planes_to_sparse
    from optical_flow.methods.config import load_of_method
    _, H, W = coef.shape
    o = load_of_method("classic+nl-fast")
    ctx = _native.context()
    ctx.set_solve_log(True)
    try:
        x = o._solve_linear_system(planes_to_sparse(coef), b, (H, W, 2))
        recs = ctx.solve_log()
    finally:
        ctx.set_solve_log(False)
    assert len(recs) == 1 and (recs[0]["h"], recs[0]["w"]) == (H, W), recs
    return np.moveaxis(x, 2, 0), recs[0]["iters"]


_cache = {}


def _case(H, W):
    """the two H x W systems, their direct solves, and the three GPU solves
    of a shape (computed once, read by every test)"""
    if (H, W) in _cache:
        return _cache[(H, W)]
    from optical_flow.methods.base import planes_to_sparse
    from scipy.sparse.linalg import spsolve
    halves = [_spd_flow_planes(H, W, seed=2 * H * W + s) for s in range(2)]
    ref = [_planes(spsolve(planes_to_sparse(c).tocsc(), b), H, W) for c, b in halves]
    alone = [_gpu_solve(c, b) for c, b in halves]
    # rows 0 .. H-1: the first system, H .. 2H-1: the second; the first
    # system's last row has no edge below it, so nothing joins the halves
    coef2 = np.concatenate([halves[0][0], halves[1][0]], axis=1)
    assert not coef2[1][H - 1].any() and not coef2[3][H - 1].any()
    b2 = _flat(np.concatenate([_planes(halves[0][1], H, W), _planes(halves[1][1], H, W)], axis=1))
    stacked = _gpu_solve(coef2, b2)
    _cache[(H, W)] = {"ref": ref, "alone": alone, "stacked": stacked}
    return _cache[(H, W)]


def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("H,W", SHAPES)
def test_cgs_edges_solve(H, W):
    """each H x W system alone: <= 1e-4 of the direct solve"""
    c = _case(H, W)
    errs = [_rel(x, r) for (x, _), r in zip(c["alone"], c["ref"])]
    print(f"{H}x{W} alone: rel err {errs[0]:.3e} {errs[1]:.3e}  iters {[it for _, it in c['alone']]}")
    assert np.all(np.isfinite(errs)) and max(errs) <= RTOL, errs


@pytest.mark.parametrize("H,W", SHAPES)
def test_cgs_edges_stacked_halves(H, W):
    """the 2H-row stack of the two systems: each half <= 1e-4 of the direct
    solve of its own H-row system (no store crosses the join or a band end)"""
    c = _case(H, W)
    x, it = c["stacked"]
    assert x.shape == (2, 2 * H, W)
    errs = [_rel(x[:, :H], c["ref"][0]), _rel(x[:, H:], c["ref"][1])]
    print(f"{2 * H}x{W} stacked: rel err of the halves {errs[0]:.3e} {errs[1]:.3e}  iters {it}")
    assert np.all(np.isfinite(errs)) and max(errs) <= RTOL, errs


def test_cgs_edges_residual_replacement():
    """at least one solve runs 16 or more iterations: long enough for the
    residual replacement (k_cg_update) to act, after which k_cgs restarts
    x_lo from 0 (the xz path: x loads from an out-of-range offset)"""
    iters = {}
    for H, W in SHAPES:
        c = _case(H, W)
        iters[(H, W)] = [it for _, it in c["alone"]] + [c["stacked"][1]]
    print("iterations (first, second, stacked):", iters)
    assert max(max(v) for v in iters.values()) >= 16, iters
