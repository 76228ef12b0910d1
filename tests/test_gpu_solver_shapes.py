"""The linear solvers at strip-seam, size-limit and
degenerate shapes, iterate by iterate: every case goes through a method's
_solve_linear_system, as test_gpu_stage_shapes.py does for the stage kernels.

(a) K-th iterate, per pixel.  CG corrects itself: a dot product that counts a
    halo lane twice or leaves the padded pixel of an odd width in changes
    alpha and beta, and the solve still converges to the right x with a few
    more iterations, below every converged-solve gate of the suite.  So the
    solve is stopped after exactly K = 4 and K = 8 iterations (rtol 0,
    maxiter K) and x_K is compared, max-norm relative to max|x_K|, with the
    float64 iterate of tests/solver_numpy.py on the same float32-valued
    system; the yardstick e32 is the same iteration in float32 arithmetic,
    computed here for each case, and the gate is M e32 (solver_inputs.M).
    test_solver_shapes_cpu.py shows without a GPU that a column counted twice
    and an edge dropped at a seam move x_K by at least 3 M e32.
(b) Converged solves with the default tolerances at the tiny shapes where a
    K-th iterate means nothing and at every one-workgroup shape: 'backslash'
    within 1e-4 of scipy's direct solve, 'pcg' with the oracle's iteration
    count +- 1, everything finite.
(c) SOR at degenerate shapes: the three arms bitwise equal, the oracle's
    sweep count +- 1 and x within 1e-4, no silent fallback; the DIA SOR
    against a float64 lexicographic SOR of the same A.

Shapes and what each covers: tests/solver_inputs.py.  Preconditioners: 'pcg'
is scalar Jacobi everywhere; the 5-point 'backslash' (k_cgs, k_cg_small,
k_cg_reg) is the degree-5 polynomial on [0.04, 2] for a method with alpha >=
0.5 (classic+nl-fast as loaded: alpha = 1.0) and on [0.01, 2] for alpha < 0.5
(the same method with alpha = 0.0, case 41x230-alpha0); the DIA 'backslash'
is 2x2 block Jacobi.  diag4 on one row or one column is a 5-point operator,
which _solve_linear_system hands to the 5-point solvers (k_cg_reg there).

Measured on an MI355X, GPU error / e32 (min / median / max over the cases
and K of each kernel; profiles/solver_shapes.md has every case):

  k_cg 'pcg'                 0.47 /   0.90 /      1.93
  k_cgs 'backslash'          0.17 /   1.02 /      3.15  (after the fix below)
  k_cg_reg 'pcg'             0.33 /   0.97 /      1.60
  k_cg_reg 'backslash'       0.09 /   1.12 /      5.75  (32x64, K = 8)
  k_cg_small 'pcg'           0.46 /   0.79 /      1.46
  k_cg_small 'backslash'     0.33 /   0.68 /      1.78
  DIA CG 'pcg'               0.21 /   1.00 /      2.67
  DIA CG 'backslash'         0.39 /   1.17 /      3.37

M = 16: twice 5.75, rounded up to a power of two.  Every case runs both K
but k_cg_small 'backslash' 1x4096 and 4096x1 (K = 4 only: at K = 8 one pixel
counted twice is below 3 M e32 at every seed searched, solver_inputs.py).

These cases found a bug in k_cgs.  Before its fix the kernel was 17 ..
11 175 e32 (4e-5 .. 4e-2 of max|x_K|, the size of the dropped-seam-edge bug)
from the textbook iterate on every level of two or more bands (measured on
the first seeds of these shapes, with the coupling term on every unknown:
40x120 K = 4 678 e32, 40x128 4755, 41x230 4611, 9x500 11 175, 4100x1 10 464)
and 0.42 e32 on the one level of a single band (1x4100), while every
converged-solve test passed.  Stage F's T5 term of q.M^-1 q takes each vertical edge once, from
the pixel below it in the band's walk; odd bands walk bottom to top, so the
edge between an even band and the odd band below it was counted by neither
and the edge between an odd band and the even band below it by both.  Only
the rho recurrence, i.e. beta, moved (amplified by the recurrence's
cancellation): the solve converged with directions that were not conjugate.
tools/cgs_t5_seams.py restates that miscount in float64 and reproduces the
deviations measured then to three digits.  Now an odd band takes both of its
seam edges (one more row step of its walk) and an even band its inner edges.

Every test prints a line "solver_shapes | kernel | HxW | figure".
"""
import ctypes as C
import functools

import numpy as np
import pytest

import solver_inputs as SI
import solver_numpy as SN

pytestmark = pytest.mark.gpu

CASES = SI.iterate_cases()


def _say(kernel, H, W, fig):
    print(f"solver_shapes | {kernel} | {H}x{W} | {fig}")


def _method(solver, alpha=1.0, filt=None, name="classic+nl-fast"):
    from optical_flow.methods.config import load_of_method
    o = load_of_method(name)
    if filt:
        f = SI.FILTERS[filt]
        o.spatial_filters = f
        o.rho_spatial_u = [o.rho_spatial_u[i % 2] for i in range(len(f))]
        o.rho_spatial_v = [o.rho_spatial_v[i % 2] for i in range(len(f))]
    o.solver = solver
    o.alpha = alpha
    return o


def _solve(o, A, b, H, W):
    """(x in A's unknown order, last_solve, names of the kernels that ran)"""
    from optical_flow import _native as nat
    ctx = nat.context()
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    try:
        x = o._solve_linear_system(A, b, (H, W, 2))
        n = C.c_int(0)
        names = (C.c_char_p * 256)()
        ctx.check(ctx.lib.of_kernel_times(ctx.handle, 256, names, None, None, None, C.byref(n)))
        ran = {names[i].decode() for i in range(min(n.value, 256))}
    finally:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return SI.flat(x), dict(o.last_solve), ran


@functools.lru_cache(maxsize=None)
def _system(i):
    A, b = SI.case_system(CASES[i])
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def _reference(i, K):
    """(x64_K, e32) of case i"""
    c = CASES[i]
    A, b = _system(i)
    pc, pa = SI.case_precond(c, A)
    x64, _ = SN.cg_iterates(A, b, K, pc, np.float64, pa)
    x32, _ = SN.cg_iterates(A, b, K, pc, np.float32, pa)
    x64.setflags(write=False)
    return x64, float(np.abs(x32 - x64).max() / np.abs(x64).max())


def _launch_name(c, A):
    """the profiling name of the iteration kernel a case must reach"""
    H, W = c["H"], c["W"]
    if c["filt"] and not SI.is_five_point(A, H, W):
        return "dia_dir"
    return "pcg_small" if H * W <= SI.CG_SMALL_PX else "pcg_iter"


# ---- (a) the K-th iterate ------------------------------------------------------
@pytest.mark.parametrize("i,K", [(i, K) for i, c in enumerate(CASES) for K in c["ks"]],
                         ids=[f"{SI.case_id(c)}-K{K}" for c in CASES for K in c["ks"]])
def test_kth_iterate(i, K):
    c = CASES[i]
    H, W = c["H"], c["W"]
    A, b = _system(i)
    x64, e32 = _reference(i, K)
    o = _method(c["solver"], c["alpha"], c["filt"])
    o.pcg_rtol, o.pcg_maxiter = 0.0, K
    o.backslash_rtol, o.backslash_maxiter = 0.0, K
    x, info, ran = _solve(o, A, b, H, W)
    err = float(np.abs(x - x64).max() / np.abs(x64).max())
    _say(SI.case_id(c), H, W, f"K {K} iters {info['iters']} err {err:.2e} e32 {e32:.2e} ratio {err / e32:.2f} "
                              f"gate {SI.M} ran {sorted(r for r in ran if r.startswith(('pcg', 'dia_d')))}")
    assert info["iters"] == K, info
    want = _launch_name(c, A)
    assert want in ran and not ({"pcg_small", "pcg_iter", "dia_dir"} - {want}) & ran, (want, ran)
    assert np.all(np.isfinite(x))
    assert err <= SI.M * e32, (err, e32, err / e32)


# ---- (b) converged solves ------------------------------------------------------
CONVERGED = SI.TINY + SI.K_CG_REG + SI.K_CG_SMALL


@functools.lru_cache(maxsize=None)
def _flow(H, W):
    coef, b = SI.flow_planes(H, W, SI.converged_seed(H, W))
    from optical_flow.methods.base import planes_to_sparse
    for a in (coef, b):
        a.setflags(write=False)
    return coef, planes_to_sparse(coef).tocsr(), b


@pytest.mark.parametrize("H,W", CONVERGED, ids=[f"{h}x{w}" for h, w in CONVERGED])
def test_converged_backslash(H, W):
    """the project's gate: within 1e-4 of the direct solve"""
    from scipy.sparse.linalg import spsolve
    _, A, b = _flow(H, W)
    xr = spsolve(A.tocsc(), b)
    x, info, ran = _solve(_method("backslash"), A, b, H, W)
    err = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    _say("backslash converged", H, W, f"rel err {err:.2e} gate 1e-4 iters {info['iters']}")
    assert "pcg_small" in ran, ran
    assert np.all(np.isfinite(x))
    assert err <= 1e-4, err


@pytest.mark.parametrize("H,W", CONVERGED, ids=[f"{h}x{w}" for h, w in CONVERGED])
def test_converged_pcg(H, W):
    """the oracle's iteration count at rtol 1e-3, +- 1 (the residuals around
    the stopping iteration are clear of the threshold:
    test_solver_shapes_cpu.py)"""
    import oracle as Or
    coef, A, b = _flow(H, W)
    o = _method("pcg")
    xo, it, _ = Or.solve(o.to_params(), coef, SI.planes(b, H, W))
    x, info, ran = _solve(o, A, b, H, W)
    err = float(np.linalg.norm(x - SI.flat(np.moveaxis(xo, 0, 2))) / np.linalg.norm(xo))
    _say("pcg converged", H, W, f"iters {info['iters']} oracle {it} (+-1) rel diff {err:.2e}")
    assert "pcg_small" in ran, ran
    assert np.all(np.isfinite(x))
    assert abs(info["iters"] - it) <= 1, (info, it)


# ---- (c) SOR -------------------------------------------------------------------
def _sor_modes(o, A, b, H, W):
    """the solve under OF_OPT_SOR_PIPELINE 0 (k_sor_lex), 1 (k_sor_pipe) and 2
    (k_sor_wg where its ring fits)"""
    from optical_flow import _native as nat
    from optical_flow._abi import OF_OPT_SOR_PIPELINE
    ctx = nat.context()
    out = []
    try:
        for m in (0, 1, 2):
            ctx.set_option(OF_OPT_SOR_PIPELINE, m)
            out.append(_solve(o, A, b, H, W))
    finally:
        ctx.set_option(OF_OPT_SOR_PIPELINE, 2)  # the default
    return out


@pytest.mark.parametrize("H,W", SI.SOR_SHAPES, ids=[f"{h}x{w}" for h, w in SI.SOR_SHAPES])
def test_sor_degenerate(H, W):
    import oracle as Or
    from optical_flow import _abi, _native as nat
    coef, A, b = _flow(H, W)
    o = _method("sor", name="hs")
    fb0 = nat.context().get_option(_abi.OF_OPT_SOR_FALLBACKS)
    (x0, s0, r0), (x1, s1, r1), (x2, s2, r2) = _sor_modes(o, A, b, H, W)
    fb1 = nat.context().get_option(_abi.OF_OPT_SOR_FALLBACKS)
    xo, it, _ = Or.solve(o.to_params(), coef, SI.planes(b, H, W))
    err = float(np.linalg.norm(x2 - SI.flat(np.moveaxis(xo, 0, 2))) / np.linalg.norm(xo))
    arm = [sorted(r & {"sor_sweep", "sor_pipe", "sor_wg"}) for r in (r0, r1, r2)]
    _say("sor", H, W, f"sweeps {s0['iters']} {s1['iters']} {s2['iters']} oracle {it} (+-1) rel err {err:.2e} "
                      f"gate 1e-4 arms {arm} fallbacks {fb1 - fb0}")
    assert fb1 == fb0
    # k_sor_wg: one strip and a ring of >= OF_SORW_MIN_RING (8) sweeps in
    # OF_SORW_RING_BYTES (144 KiB) of LDS
    wg = H <= 64 and H * W * 8 * 8 <= 144 * 1024
    assert arm == [["sor_sweep"], ["sor_pipe"], ["sor_wg"] if wg else ["sor_pipe"]], arm
    assert s1["iters"] == s0["iters"] and s2["iters"] == s0["iters"], (s0, s1, s2)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(x2, x0)
    assert np.all(np.isfinite(x0))
    assert abs(s0["iters"] - it) <= 1, (s0, it)
    assert err <= 1e-4, err


@pytest.mark.parametrize("filt,H,W", SI.DIA_SOR, ids=[f"{f}-{h}x{w}" for f, h, w in SI.DIA_SOR])
def test_dia_sor(filt, H, W):
    """k_dia_sor (one workgroup, a thread per column up to 1024) against a
    float64 lexicographic SOR of the same A"""
    A, b = SI.dia_system(H, W, SI.FILTERS[filt], SI.seed_of(H, W, 2))
    assert not SI.is_five_point(A, H, W)
    o = _method("sor", filt=filt)
    P = o.to_params()
    xr, it = SN.sor_lex(A, b, P.sor_omega, P.sor_tol, P.sor_max_iters)
    x, info, ran = _solve(o, A, b, H, W)
    err = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    _say(f"dia_sor {filt}", H, W, f"sweeps {info['iters']} fp64 {it} (+-1) rel err {err:.2e} gate 1e-4")
    assert "dia_sor" in ran, ran
    assert np.all(np.isfinite(x))
    assert abs(info["iters"] - it) <= 1, (info, it)
    assert err <= 1e-4, err
