"""Image-edge strips of the fused CG iteration (k_cgs) own their halo lanes.

A k_cgs strip is 64 lanes x 2 px; strip t holds columns [112 t, 112 t + 128)
and owns lanes 4..59.  The first strip also owns lanes 0..3 and the last
strip lanes 60..63 (no neighbouring strip recomputes those columns), so n
strips cover 112 n + 16 columns.  A wrong lane rule shows as columns stored
by no strip or by two, or as pixels counted twice or not at all in the dot
products, i.e. as a wrong solution, at the widths where the rule changes:

    W    strips
    120  1   lanes 60..63 lie beyond W
    128  1   all 64 lanes are output
    129  2   odd width (the ODD instance); the second strip owns 9 columns
    240  2   both strips full: 120 + 120
    241  3   odd width
    352  3   an interior strip between two full edge strips
    353  4   odd width

H = 40 throughout (40 x 120 = 4800 px > CG_SMALL_PX = 4096, so k_cgs runs at
every width).  Systems as test_gpu_cgs_edges._spd_flow_planes builds them
(restated here), solved with 'backslash' through _solve_linear_system with
the solve log on.  Yardstick as there: within 1e-4 relative error of scipy's
direct solve.  Each width is solved three times: two independent H x W
systems alone, and the H x 2W system that puts them side by side.  Column
W - 1 has no edge to its right, so nothing couples the halves and each half
is held to the bound against the direct solve of its own system: a store or
a dot product that crosses a strip edge shows as a wrong half.

Seeds: 2 * H * W and 2 * H * W + 1, fixed before the first GPU run, on which
all 21 solves took 19 to 30 iterations, so no seed had to be searched for.
Relative errors measured there: 7e-7 to 4.5e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 40
WIDTHS = [120, 128, 129, 240, 241, 352, 353]
RTOL = 1e-4


def _spd_flow_planes(H, W, seed):
    """test_gpu_cgs_edges._spd_flow_planes: a random flow system of the shape
    flow_operator assembles: positive edge weights spanning 4 decades, PSD
    2x2 data blocks, diagonal = data block + sum of incident edge weights."""
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
    _, h, w = coef.shape
    o = load_of_method("classic+nl-fast")
    ctx = _native.context()
    ctx.set_solve_log(True)
    try:
        x = o._solve_linear_system(planes_to_sparse(coef), b, (h, w, 2))
        recs = ctx.solve_log()
    finally:
        ctx.set_solve_log(False)
    assert len(recs) == 1 and (recs[0]["h"], recs[0]["w"]) == (h, w), recs
    return np.moveaxis(x, 2, 0), recs[0]["iters"]


_cache = {}


def _case(W):
    """the two H x W systems, their direct solves, and the three GPU solves
    of a width (computed once, read by every test)"""
    if W in _cache:
        return _cache[W]
    from optical_flow.methods.base import planes_to_sparse
    from scipy.sparse.linalg import spsolve
    halves = [_spd_flow_planes(H, W, seed=2 * H * W + s) for s in range(2)]
    ref = [_planes(spsolve(planes_to_sparse(c).tocsc(), b), H, W) for c, b in halves]
    alone = [_gpu_solve(c, b) for c, b in halves]
    # columns 0 .. W-1: the first system, W .. 2W-1: the second; the first
    # system's last column has no edge to its right, so nothing joins them
    coef2 = np.concatenate([halves[0][0], halves[1][0]], axis=2)
    assert not coef2[0][:, W - 1].any() and not coef2[2][:, W - 1].any()
    b2 = _flat(np.concatenate([_planes(halves[0][1], H, W), _planes(halves[1][1], H, W)], axis=2))
    beside = _gpu_solve(coef2, b2)
    _cache[W] = {"ref": ref, "alone": alone, "beside": beside}
    return _cache[W]


def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("W", WIDTHS)
def test_cgs_strips_geometry(W):
    """the widths exercise the strip counts the table above states"""
    from optical_flow import _native
    want = {120: 1, 128: 1, 129: 2, 240: 2, 241: 3, 352: 3, 353: 4}[W]
    assert _native.solver_geometry(H, W, "backslash")["grid_x"] == want


@pytest.mark.parametrize("W", WIDTHS)
def test_cgs_strips_solve(W):
    """each H x W system alone: <= 1e-4 of the direct solve"""
    c = _case(W)
    errs = [_rel(x, r) for (x, _), r in zip(c["alone"], c["ref"])]
    print(f"{H}x{W} alone: rel err {errs[0]:.3e} {errs[1]:.3e}  iters {[it for _, it in c['alone']]}")
    assert np.all(np.isfinite(errs)) and max(errs) <= RTOL, errs


@pytest.mark.parametrize("W", WIDTHS)
def test_cgs_strips_side_by_side(W):
    """the two systems side by side in one H x 2W system: each half <= 1e-4
    of the direct solve of its own system (no store or dot product crosses a
    strip edge)"""
    c = _case(W)
    x, it = c["beside"]
    assert x.shape == (2, H, 2 * W)
    errs = [_rel(x[:, :, :W], c["ref"][0]), _rel(x[:, :, W:], c["ref"][1])]
    print(f"{H}x{2 * W} side by side: rel err of the halves {errs[0]:.3e} {errs[1]:.3e}  iters {it}")
    assert np.all(np.isfinite(errs)) and max(errs) <= RTOL, errs


def test_cgs_strips_residual_replacement():
    """at least one solve runs 16 or more iterations: long enough for the
    residual replacement (k_cg_update) to act, after which k_cgs restarts
    x_lo from 0, with the edge strips' added output lanes"""
    iters = {}
    for W in WIDTHS:
        c = _case(W)
        iters[W] = [it for _, it in c["alone"]] + [c["beside"][1]]
    print("iterations (first, second, side by side):", iters)
    assert max(max(v) for v in iters.values()) >= 16, iters
