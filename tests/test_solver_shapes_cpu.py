"""Conditions on the inputs of test_gpu_solver_shapes.py, checked without a GPU:
the case table claims what of_solver_geometry reports, the systems are the
float32 numbers the GPU gets, the float64 iterates stay clear of the kernels'
noise-floor logic, the float32 yardstick is usable, the numpy reference agrees
with the oracle's independent C statement, and the two planted bugs (a column
counted twice in every dot product, an edge dropped at a seam) move the K-th
iterate by at least three times the gate the GPU test applies: a kernel that
is subtly wrong in that way cannot pass it.
"""
import functools

import numpy as np
import pytest

import solver_inputs as SI
import solver_numpy as SN

CASES = SI.iterate_cases()
IDS = [SI.case_id(c) for c in CASES]
CONVERGED = SI.TINY + SI.K_CG_REG + SI.K_CG_SMALL


def _rel(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


# ---- the geometry the table claims ---------------------------------------------
@pytest.mark.parametrize("solver,table", [("pcg", SI.K_CG), ("backslash", SI.K_CGS)], ids=["k_cg", "k_cgs"])
def test_fused_geometry_table(solver, table):
    from optical_flow import _native
    for (H, W), (strips, bands, R) in table.items():
        g = _native.solver_geometry(H, W, solver)
        assert (g["grid_x"], g["bands"], g["rows"]) == (strips, bands, R), ((H, W), g)
        assert H * W > SI.CG_SMALL_PX  # the fused kernels, not k_cg_small
        assert (bands - 1) * R < H <= bands * R


def test_k_cg_properties():
    """what the k_cg rows say they cover (strips of 124 columns, 4 bands per block)"""
    from optical_flow import _native
    g = _native.solver_geometry(34, 124, "pcg")
    assert 34 - (g["bands"] - 1) * g["rows"] == 2          # last band 2 rows
    assert g["bands"] - 4 * (g["grid_y"] - 1) == 1         # last block: one live wave
    assert 125 - 124 * 1 == 1 and 249 - 124 * 2 == 1       # a strip that owns one column
    assert 248 == 2 * 124 and 63 < 124
    assert sorted({SI.K_CG[s][2] for s in SI.K_CG}) == [1, 3, 4, 5, 6, 7, 8]  # every R
    assert [w % 2 for _, w in [(34, 125), (33, 249), (70, 63)]] == [1, 1, 1]   # the ODD instances
    g = _native.solver_geometry(5, 1000, "pcg")
    assert (g["rows"], 5 - g["rows"]) == (3, 2)             # bands of 3 and 2 rows


def test_k_cgs_covers_both_width_parities_and_a_lone_strip():
    strips = {s: SI.K_CGS[s][0] for s in SI.K_CGS}
    assert strips[(40, 128)] == 1 and strips[(40, 129)] == 2      # 128 columns: the widest lone strip
    assert strips[(40, 240)] == 2 and strips[(40, 241)] == 3      # 120 + 120, then a third strip of one column
    assert {w % 2 for _, w in SI.K_CGS} == {0, 1}


def test_one_workgroup_sizes():
    px = [h * w for h, w in SI.K_CG_REG]
    assert max(px) == SI.CG_REG_PX and SI.CG_REG_PX - 1 in px and all(p <= SI.CG_REG_PX for p in px)
    px = [h * w for h, w in SI.K_CG_SMALL]
    assert min(px) == SI.CG_REG_PX + 1 and max(px) == SI.CG_SMALL_PX and SI.CG_SMALL_PX - 1 in px
    assert all(SI.CG_REG_PX < p <= SI.CG_SMALL_PX for p in px)
    assert SI.FIRST_FUSED[0] * SI.FIRST_FUSED[1] == SI.CG_SMALL_PX + 1
    assert 3 * 600 > 512 > 600 - 512 and 4 * 511 == 2044      # a row across the 512-thread stride


def test_size_limits_are_the_kernels():
    """the hand-overs the shapes sit on are the ones the sources define: both
    one-workgroup kernels launch under one profiling name, so only these pin
    which of them a 2048 px or 2049 px level reaches"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optical-flow-python_amd", "csrc")
    wg = open(os.path.join(src, "kernels_cg_wg.hip")).read()
    host = open(os.path.join(src, "host_solve.hip")).read()

    def define(text, name):
        return re.search(r"#define %s\s+(.+)" % name, text).group(1).strip()
    assert int(define(wg, "CGR_T")) * int(define(wg, "CGR_M")) == SI.CG_REG_PX
    assert define(wg, "CG_REG_PX") == "(CGR_T * CGR_M)"
    assert int(define(wg, "CG_SMALL_PX")) == SI.CG_SMALL_PX
    assert "if ((double)H * W <= CG_REG_PX)" in host and "(double)H * W <= CG_SMALL_PX ? solve_cg_small" in host


def test_first_fused_size_reports_the_fused_geometry():
    """17x241 = 4097 px: strips, bands and R of k_cg and k_cgs"""
    from optical_flow import _native
    g = _native.solver_geometry(*SI.FIRST_FUSED, "pcg")
    assert (g["grid_x"], g["bands"], g["rows"], g["strip_cols"]) == (2, 5, 4, 124), g
    g = _native.solver_geometry(*SI.FIRST_FUSED, "backslash")
    assert (g["grid_x"], g["bands"], g["rows"], g["strip_cols"]) == (3, 3, 6, 120), g


def test_sor_shapes():
    from optical_flow import _native
    ring = lambda h, w: min(8, 144 * 1024 // (8 * h * w))  # noqa: E731  (sor_wg_ring, host_solve.hip)
    assert ring(64, 36) == 8 and 64 * 36 * 8 * 8 == 144 * 1024 and ring(64, 37) == 7
    assert _native.solver_geometry(65, 40, "sor")["bands"] == 2 and 65 - 64 == 1
    assert _native.solver_geometry(70, 1, "sor")["bands"] == 2 and 70 - 64 == 6
    assert all(_native.solver_geometry(h, w, "sor")["bands"] == 1 for h, w in [(1, 70), (2, 3), (64, 36), (64, 37)])


def test_sparse_to_planes_one_row_or_column():
    """_solve_linear_system's first step on a level of one row or one column
    (it raised ValueError there: scipy answers an empty fancy index with one
    element)"""
    from optical_flow.methods.base import sparse_to_planes
    for H, W in [(1, 70), (70, 1), (1, 1), (1, 2), (2, 1)]:
        coef, _ = SI.flow_planes(H, W, SI.seed_of(H, W, 1))
        A, _ = SI.flow_system(H, W, SI.seed_of(H, W, 1))
        np.testing.assert_array_equal(sparse_to_planes(A, H, W), coef)


# ---- the systems ----------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_system_is_float32_exact(i):
    from optical_flow.methods.base import dia_to_sparse, planes_to_sparse, sparse_to_dia, sparse_to_planes
    c = CASES[i]
    H, W = c["H"], c["W"]
    A, b = SI.case_system(c)
    assert np.array_equal(b, SI.f32(b)) and np.array_equal(A.data, SI.f32(A.data))
    assert abs(A - A.T).max() == 0
    if SI.is_five_point(A, H, W):
        assert abs(planes_to_sparse(SI.f32(sparse_to_planes(A, H, W))) - A).max() == 0
    else:
        D, planes = sparse_to_dia(A, H, W)
        assert D == {"diag4": 1, "wide": 2}[c["filt"]]
        assert abs(dia_to_sparse(SI.f32(planes), D) - A).max() == 0
    if A.shape[0] <= 300:
        assert np.linalg.eigvalsh(A.toarray()).min() > 0


def test_dia_filters_that_do_not_fit():
    """3x3 holds one placement of a 1x3 filter per row; one row holds no
    vertical or diagonal filter (diag4 is a 5-point operator there) and
    60x1100 exceeds k_dia_sor's 1024 threads"""
    A, _ = SI.dia_system(1, 70, SI.FILTERS["diag4"], 5)
    assert SI.is_five_point(A, 1, 70)
    A, _ = SI.dia_system(70, 1, SI.FILTERS["diag4"], 5)
    assert SI.is_five_point(A, 70, 1)
    for tag in ("diag4", "wide"):
        for H, W in [(3, 3), (37, 65)] + ([(1, 70), (70, 1)] if tag == "wide" else []):
            A, _ = SI.dia_system(H, W, SI.FILTERS[tag], 5)
            assert not SI.is_five_point(A, H, W), (tag, H, W)
    assert 1100 > 1024


# ---- the iterates ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _figures(i):
    """per K: (x64, ||r_K|| / ||b||, e32, column twice, seam edge dropped)"""
    c = CASES[i]
    H, W = c["H"], c["W"]
    A, b = SI.case_system(c)
    pc, pa = SI.case_precond(c, A)
    ax, at = SI.case_seam(c)
    dup = SN.line_indices(H, W, ax, at)
    drop = SN.drop_seam(A, H, W, ax, at)
    out = {}
    for K in c["ks"]:
        x64, res = SN.cg_iterates(A, b, K, pc, np.float64, pa)
        x32, _ = SN.cg_iterates(A, b, K, pc, np.float32, pa)
        xd, _ = SN.cg_iterates(A, b, K, pc, np.float64, pa, dup=dup)
        xe, _ = SN.cg_iterates(A, b, K, pc, np.float64, pa, drop=drop)
        out[K] = (x64, res, _rel(x32, x64), _rel(xd, x64), _rel(xe, x64))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_iterate_conditions(i):
    c = CASES[i]
    for K, (x64, res, e32, dup, drop) in _figures(i).items():
        print(f"{IDS[i]} K {K}: |r|/|b| {res:.2e} e32 {e32:.2e} gate {SI.M * e32:.2e} "
              f"column twice {dup:.2e} edge dropped {drop:.2e}")
        assert np.all(np.isfinite(x64))
        assert res >= 1e-4, res                     # clear of the noise floor and drift restart
        assert np.isfinite(e32) and e32 > 0
        assert drop >= 3 * SI.M * e32, (K, drop, e32)
        if c["dup"]:
            assert dup >= 3 * SI.M * e32, (K, dup, e32)


def test_planted_bug_exceptions_are_needed():
    """every entry of solver_inputs.EXCEPTIONS and CASE_SALT names a case, no
    case drops the twice counted column, and no entry is an exception for
    nothing: with both K the condition fails"""
    assert set(SI.CASE_SALT) <= set(IDS) and all(c["dup"] for c in CASES)
    assert set(SI.EXCEPTIONS) <= set(IDS)
    for i, c in enumerate(CASES):
        if IDS[i] not in SI.EXCEPTIONS:
            assert c["ks"] == SI.KS and c["dup"]
            continue
        full = dict(c, ks=SI.KS, dup=True)
        A, b = SI.case_system(full)
        pc, pa = SI.case_precond(full, A)
        ax, at = SI.case_seam(full)
        dup = SN.line_indices(c["H"], c["W"], ax, at)
        short = []
        for K in SI.KS:
            x64, _ = SN.cg_iterates(A, b, K, pc, np.float64, pa)
            e32 = _rel(SN.cg_iterates(A, b, K, pc, np.float32, pa)[0], x64)
            short.append(_rel(SN.cg_iterates(A, b, K, pc, np.float64, pa, dup=dup)[0], x64) < 3 * SI.M * e32)
        assert any(short), IDS[i]
        if not c["dup"]:
            assert all(short), IDS[i]


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["solver"] == "pcg" and not c["filt"]],
                         ids=[n for n, c in zip(IDS, CASES) if c["solver"] == "pcg" and not c["filt"]])
def test_oracle_restates_the_pcg_iterate(i):
    """oracle.solve with rtol 0 and maxiter K is the same algorithm in C: both
    float64, so they differ by rounding only (1e-9 allows 1e7 ulps for the
    growth over K iterations on weights spanning 4 decades)"""
    import oracle as Or
    from optical_flow.methods.base import sparse_to_planes
    from optical_flow.methods.config import load_of_method
    c = CASES[i]
    H, W = c["H"], c["W"]
    A, b = SI.case_system(c)
    o = load_of_method("classic+nl-fast")
    o.solver, o.pcg_rtol = "pcg", 0.0
    coef = sparse_to_planes(A, H, W)
    for K, (x64, *_) in _figures(i).items():
        o.pcg_maxiter = K
        xo, it, _ = Or.solve(o.to_params(), coef, SI.planes(b, H, W))
        assert it == K
        assert _rel(SI.flat(np.moveaxis(xo, 0, 2)), x64) <= 1e-9


def test_float32_iterate_is_float32():
    A, b = SI.flow_system(9, 14, 3)
    for pc, pa in (("jacobi", None), ("block", None), ("poly5", 0.04)):
        x, _ = SN.cg_iterates(A, b, 3, pc, np.float32, pa)
        assert x.dtype == np.float32


def test_cheb_poly_is_the_chebyshev_residual():
    """1 - X p(X) equioscillates on [a, 2] with amplitude 1 / T_6((2 + a) / (2 - a))"""
    for a in (SN.CG_CHEB_A, SN.CG_CHEB_A_ROBUST):
        c = SN.cheb_poly(SN.CG_DEG, a)
        X = np.linspace(a, 2.0, 20001)
        p = sum(ci * (1 - X) ** i for i, ci in enumerate(c))
        amp = 1.0 / np.cosh(6 * np.arccosh((2 + a) / (2 - a)))
        assert np.all(p > 0)
        np.testing.assert_allclose(np.abs(1 - X * p).max(), amp, rtol=1e-6)
    assert SN.poly_interval(0.0) == 0.01 and SN.poly_interval(1.0) == 0.04 and SN.poly_interval(0.5) == 0.04


# ---- the converged solves -------------------------------------------------------
@pytest.mark.parametrize("H,W", CONVERGED, ids=[f"{h}x{w}" for h, w in CONVERGED])
def test_pcg_stop_is_clear_of_the_threshold(H, W):
    """the residuals at the stopping iteration and the one before are not
    within 5 % of rtol ||b||: fp32 rounding cannot move the GPU's count by
    more than the +- 1 its test allows; the oracle counts the same"""
    import oracle as Or
    from optical_flow.methods.config import load_of_method
    coef, b = SI.flow_planes(H, W, SI.converged_seed(H, W))
    A, _ = SI.flow_system(H, W, SI.converged_seed(H, W))
    o = load_of_method("classic+nl-fast")
    o.solver = "pcg"
    it, hist = SN.cg_stop(A, b, o.pcg_rtol, o.pcg_maxiter)
    _, ito, _ = Or.solve(o.to_params(), coef, SI.planes(b, H, W))
    atol = o.pcg_rtol * np.linalg.norm(b)
    print(f"{H}x{W}: {it} iterations, last residuals / atol {[round(h / atol, 3) for h in hist[-2:]]}")
    assert it == ito
    if it < o.pcg_maxiter:
        for h in hist[-2:]:
            assert not 0.95 * atol <= h <= 1.05 * atol, (hist[-2:], atol)


@pytest.mark.parametrize("H,W", CONVERGED, ids=[f"{h}x{w}" for h, w in CONVERGED])
def test_converged_systems_are_well_posed(H, W):
    """a direct solve is meaningful: the smallest 2x2 pivot is positive (the
    coupling term; a 1x1 level has no edges)"""
    A, b = SI.flow_system(H, W, SI.converged_seed(H, W))
    a, c, d = SN._blocks(A)
    assert np.all(a * d - c * c > 0)
    if A.shape[0] <= 300:
        ev = np.linalg.eigvalsh(A.toarray())
        assert ev.min() > 0 and ev.max() / ev.min() < 1e6


# ---- SOR --------------------------------------------------------------------------
def _sor_stop_is_clear(A, b, n):
    """The fp32 kernel's sweep count is within 1 of the float64 count n when no
    sweep before n - 1 comes within 0.1 % of the threshold from above and
    sweep n or n + 1 is below it by 0.1 %.  The margin: one fp32 sweep rounds x
    by ~6e-8 |x|, which moves ||dx|| / ||x|| ~ 1e-2 by ~1e-5 of itself; 0.1 %
    is a hundred times that."""
    r = SN.sor_ratios(A, b, n + 1)
    print(f"{n} sweeps, |dx|/|x| of the last four {[f'{v:.4e}' for v in r[-4:]]}")
    assert r[n - 1] < 1e-2 and all(v >= 1e-2 for v in r[:n - 1])
    assert all(v >= 1.001e-2 for v in r[:n - 2]), r[:n - 2][-3:]
    assert min(r[n - 1], r[n]) <= 0.999e-2, r[n - 1:]


@pytest.mark.parametrize("H,W", SI.SOR_SHAPES, ids=[f"{h}x{w}" for h, w in SI.SOR_SHAPES])
def test_sor_lex_matches_the_oracle(H, W):
    """the numpy SOR that test_dia_sor compares with is the oracle's
    lexicographic SOR on a 5-point system: same sweeps, same x"""
    import oracle as Or
    from optical_flow.methods.config import load_of_method
    coef, b = SI.flow_planes(H, W, SI.converged_seed(H, W))
    A, _ = SI.flow_system(H, W, SI.converged_seed(H, W))
    o = load_of_method("hs")
    o.solver = "sor"
    P = o.to_params()
    xo, it, _ = Or.solve(P, coef, SI.planes(b, H, W))
    x, n = SN.sor_lex(A, b, P.sor_omega, P.sor_tol, P.sor_max_iters)
    assert n == it
    assert _rel(x, SI.flat(np.moveaxis(xo, 0, 2))) <= 1e-10
    _sor_stop_is_clear(A, b, n)


@pytest.mark.parametrize("filt,H,W", SI.DIA_SOR, ids=[f"{f}-{h}x{w}" for f, h, w in SI.DIA_SOR])
def test_dia_sor_stop_is_clear_of_the_threshold(filt, H, W):
    A, b = SI.dia_system(H, W, SI.FILTERS[filt], SI.seed_of(H, W, 2))
    n = SN.sor_lex(A, b)[1]
    assert n < 10000
    _sor_stop_is_clear(A, b, n)
