"""One pyramid level's warping loop (hs_base, irls_base in host_flow.hip) and
the kernels only it launches, at tile-seam and degenerate shapes.

A level is not a smooth function of its inputs (medians and robust weights
flip on last bits), so nothing here compares a whole level with float64 under
a tolerance.  The chain has no new tolerance in it:

  a-c  every stage a level uses has a stage entry (include/optflow.h) and is
       checked alone at the seam shapes: against the float64 oracle under the
       bound an existing test holds the same quantity to (the operator bounds
       of test_operator_planes, 1e-5 occlusion, 1e-6 median), and bit for bit
       where numpy float32 can restate its arithmetic or another kernel
       computes the same thing.
  d    the level, of_compute_flow_base[_weighted], equals bit for bit the same
       loop written in Python from those stage entries
       (level_numpy.level_loop with GpuBackend).
  cpu  that Python loop with the oracle's float64 stages reproduces the
       oracle's own level to 1e-12 (tests/test_level_shapes_cpu.py).

A mismatch in d with a-c passing is the loop's glue or buffer handling; a
mismatch in a-c is one kernel.

Shapes: test_gpu_stage_shapes.SMALL -- one row, one column, below the filter
radius, OF_BX + 1 columns, the ROF tile seams -- and for the elementwise
launches (130, 4100): 2015 blocks, a second grid-stride pass.  113x49 and
112x48 are above CG_SMALL_PX, so the level's solves there are the strip
solver's.  Inputs: tests/level_inputs.py.

Every test prints a line "level_shapes | what | shape | figure".
"""
import ctypes as C
import functools

import numpy as np
import pytest

import level_inputs as L
import level_numpy as LN
import oracle as O
import stage_inputs as S

pytestmark = pytest.mark.gpu

F = np.float32


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


def _say(what, hw, fig):
    print(f"level_shapes | {what} | {hw[0]}x{hw[1]} | {fig}")


@functools.lru_cache(maxsize=None)
def _in(H, W):
    d = L.make(H, W)
    for a in d.values():
        a.setflags(write=False)
    return d


def _b(a):
    """the float32 bytes of an array holding float32 values"""
    a32 = np.asarray(a).astype(F)
    assert np.array_equal(a32.astype(np.float64), np.asarray(a, dtype=np.float64))
    return np.ascontiguousarray(a32).tobytes()


def _method(name, **over):
    from optical_flow.methods.config import load_of_method
    o = load_of_method(name)
    o.display = False
    for k, v in over.items():
        setattr(o, k, v)
    return o


# ---- a. fused warp + assembly against the two kernels, every instance --------
# pen_mode() (host_flow.hip) by parameter set:
#   OF_PM_Q                  alpha = 1 and every quadratic stand-in quadratic: classic+nl at alpha 1
#   OF_PM_R(GEN_CHARBONNIER) alpha = 0, data and spatial penalties generalized Charbonnier: classic+nl at alpha 0
#   OF_PM_R(CHARBONNIER)     alpha = 0, all Charbonnier: classic-c at alpha 0
#   OF_PM_R(LORENTZIAN)      alpha = 0, all Lorentzian: ba at alpha 0
#   OF_PM_R(CONST)           Horn-Schunck (its level always assembles at alpha 0 with constant weights)
#   OF_PM_ANY                0 < alpha < 1 (both stages blended): classic+nl at alpha 0.5; and alpha = 0 with a
#                            data penalty of another kind than the spatial ones: ba with a Charbonnier rho_data
MODES = [("Q", "classic+nl", 1.0, None), ("R gen_charbonnier", "classic+nl", 0.0, None),
         ("R charbonnier", "classic-c", 0.0, None), ("R lorentzian", "ba", 0.0, None), ("R const", "hs", 0.0, None),
         ("ANY blend", "classic+nl", 0.5, None), ("ANY mixed", "ba", 0.0, ("charbonnier", 1e-3))]


@pytest.mark.parametrize("mode,meth,alpha,rho_data", MODES, ids=[m[0].replace(" ", "_") for m in MODES])
@pytest.mark.parametrize("H,W", L.SMALL + [L.BIG], ids=_ids(L.SMALL + [L.BIG]))
def test_fused_equals_two_kernels(H, W, mode, meth, alpha, rho_data):
    """of_warp_operator against of_partial_deriv + of_flow_operator_weighted:
    equal bytes in all 7 + 2 planes, for 3 interpolations x nc in {1, 3} x
    weight in {none, plane} of this penalty mode (MODES above): the 72
    k_warp_operator instances over the parametrisation, with the fused
    kernel's own neighbour gather (ld_nbr) at every seam shape."""
    from optical_flow.robust.robust_function import RobustFunction
    from optical_flow.utils.derivatives import partial_deriv
    d = _in(H, W)
    n = 0
    for interp in S.INTERPS:
        for nc in (1, 3):
            o = _method(meth, interpolation_method=interp)
            if rho_data:
                o.rho_data = RobustFunction(*rho_data)
            o.images = d["images"] if nc == 1 else d["images3"]
            It, Ix, Iy = partial_deriv(o.images, d["uv"], interp, S.FILT, 0.5)
            # some sample stays in the plane: there is a data term to assemble.  (The reference's
            # bi-cubic needs the cell's far corner, row floor(y) + 1 <= H, derivatives.py:27-145:
            # on one row or column it has no sample inside, whatever the flow.)
            has_data = bool((It != 0).any())
            assert has_data or (interp == "bi-cubic" and min(H, W) == 1)
            plain = None
            for w in (None, d["weight"]):
                two = o._operator_planes(d["uv"], None, It, Ix, Iy, alpha, data_weight=w)
                if w is None:
                    plain = two
                elif has_data and H * W >= 20:  # the weight is really in there
                    assert two[0][4:].tobytes() != plain[0][4:].tobytes()
                one = o._warp_operator_planes(d["uv"], alpha, 0.5, w)
                for a, b, what in zip(one, two, ("coef", "rhs")):
                    assert a.dtype == b.dtype == F and np.all(np.isfinite(a))
                    diff = a != b
                    assert a.tobytes() == b.tobytes(), (interp, nc, w is not None, what, int(diff.sum()),
                                                        np.argwhere(diff)[:5])
                n += 1
    _say(f"fused == two kernels, {mode}", (H, W), f"{n} instances x 9 planes equal")


@pytest.mark.parametrize("method", ["cubic", "bi-linear"])
@pytest.mark.parametrize("H,W", [(1, 70), (70, 1)], ids=_ids([(1, 70), (70, 1)]))
def test_partial_deriv_inside_one_row_or_column(H, W, method):
    """test_gpu_stage_shapes.test_partial_deriv has no sample inside the plane
    at these two shapes (its flow across the single row / column is never 0:
    "nonzero ref 0" in profiles/stage_shapes.md).  level_inputs' flow is 0
    across the plane at every second pixel, so half the samples stay inside,
    exactly on the plane in float32 as in float64; along the plane the
    coordinates keep stage_inputs' distance from the thresholds.  Bound:
    test_partial_deriv's 5e-3 + 1e-5 |ref|, one and three channels.  Not
    'bi-cubic': the reference's Hermite cell needs row floor(y) + 1 <= H, so
    on one row or column it has no sample inside."""
    from optical_flow.utils.derivatives import partial_deriv
    d = _in(H, W)
    uv = d["uv"]
    n = max(H, W)
    along = np.arange(1, n + 1.0).reshape(H, W) + uv[..., 0 if H == 1 else 1]
    assert not ((np.abs(along - 1) <= 1e-3) | (np.abs(along - n) <= 1e-3)).any()
    worst, nz = 0.0, 0
    for images in (d["images"], d["images3"]):
        out = partial_deriv(images, uv, method, S.FILT, 0.5)
        ref = O.partial_deriv(images, uv, method, S.FILT, 0.5)
        for got, r, name in zip(out, ref, ("It", "Ix", "Iy")):
            err = np.abs(got - r)
            bad = err > 5e-3 + 1e-5 * np.abs(r)
            worst = max(worst, float(err.max()))
            assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], float(err[bad].max()))
            nz += int((r != 0).sum())
    _say(f"partial_deriv {method}", (H, W), f"max err {worst:.2e} nonzero ref {nz}")
    assert nz >= 30


OP_ARMS = [("duv", "classic+nl", 0.0, 1, True, False), ("nc3", "classic-c", 0.0, 3, False, False),
           ("nc3 duv", "ba", 0.0, 3, True, False), ("weight hs", "hs", 0.0, 1, False, True),
           ("weight Q nc3 duv", "classic+nl", 1.0, 3, True, True)]


@pytest.mark.parametrize("arm,meth,alpha,nc,with_duv,weighted", OP_ARMS, ids=[a[0].replace(" ", "_") for a in OP_ARMS])
@pytest.mark.parametrize("H,W", L.SMALL + [L.BIG], ids=_ids(L.SMALL + [L.BIG]))
def test_operator_planes_arms(H, W, arm, meth, alpha, nc, with_duv, weighted):
    """The two-kernel form against the oracle under test_operator_planes'
    bounds, for the arms that sweep leaves out: duv given (ld_uvd), three
    channels, a weight.  With constant psi (HS, the quadratic stage) weighting
    the data term by w is scaling It, Ix and Iy by sqrt(w), as in
    test_gpu_weight.test_operator_against_the_oracle.

    Without duv the inputs are test_operator_planes' (generic float32).  With
    duv they lie on grids -- uv in multiples of 2^-16 px, duv of 2^-6 px, the
    derivative planes of 2^-6 -- so that uv + duv and the linearised residual
    It + Ix du + Iy dv are exact in float32 (20 and 24 significant bits at
    most).  The kernel and the float64 oracle then evaluate the penalties at
    the same point, as with stage_inputs.flow and the warped coordinate.  A
    residual rounded to float32 (half an ulp of ~30 grey levels, 2e-6) is
    otherwise amplified by the generalized Charbonnier weight's logarithmic
    derivative, 0.55 / sigma = 550 per grey level at |It| = sigma = 1e-3: up
    to 1e-3 relative in psi', against a bound of 1e-4, at the handful of
    pixels of a 130x4100 plane whose residual is that small
    (profiles/level_shapes.md).  That is the conditioning of the penalty, not
    the kernel's arithmetic, and says nothing about a seam."""
    d = _in(H, W)
    rng = np.random.default_rng(3000 + 7 * H + W)
    images = d["images"] if nc == 1 else d["images3"]
    o = _method(meth)
    o.images = images
    if with_duv:
        uv = np.round(rng.normal(0, 0.7, (H, W, 2)) * 65536.0) / 65536.0
        duv = np.round(rng.normal(0, 0.3, (H, W, 2)) * 64.0) / 64.0
        D = [np.round(a * 64.0) / 64.0 for a in O.partial_deriv(images, uv, o.interpolation_method, S.FILT, 0.5)]
        assert max(np.abs(a).max() for a in D) < 512 and np.abs(duv).max() < 2 and np.abs(uv).max() < 8
    else:
        uv = S.f32(rng.normal(0, 0.7, (H, W, 2)))
        duv = None
        D = [S.f32(a) for a in O.partial_deriv(images, uv, o.interpolation_method, S.FILT, 0.5)]
    w = d["weight"] if weighted else None
    coef, rhs = o._operator_planes(uv, duv, *D, alpha, data_weight=w)
    s = np.sqrt(w) if weighted else 1.0
    if weighted and nc > 1:
        s = s[..., None]
    oc, orhs = O.flow_operator(o.to_params(), alpha, uv, duv, *[a * s for a in D])
    scale = np.abs(oc).max(axis=(1, 2), keepdims=True)
    bscale = np.abs(orhs).max()
    ec = np.abs(coef - oc) / (1e-4 * np.abs(oc) + 1e-6 * scale + 1e-300)
    eb = np.abs(rhs - orhs) / (1e-4 * np.abs(orhs) + 2e-5 * bscale + 1e-300)
    _say(f"operator {arm}", (H, W), f"coef {ec.max():.3f} rhs {eb.max():.3f} of the bound")
    assert np.all(np.abs(coef - oc) <= 1e-4 * np.abs(oc) + 1e-6 * scale), np.abs(coef - oc).max()
    assert np.all(np.abs(rhs - orhs) <= 1e-4 * np.abs(orhs) + 2e-5 * bscale)


# ---- b. the update with clip and the occlusion map ------------------------------
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("H,W", L.SMALL + [L.BIG], ids=_ids(L.SMALL + [L.BIG]))
def test_flow_update(H, W, nc):
    """of_flow_update (k_update_occ as irls_base launches it): uv1 is
    float32(uv) + clip(float32(x)) in its bytes with the clip on and off, with
    and without the occlusion output; occ is detect_occlusion of that uv1
    within test_occlusion's 1e-5.  x has |x| > 1 in column 0, column W - 1,
    row 0 and at a row's first pixel: where the kernel recomputes the left and
    upper neighbour's uv + clip(x) (test_level_shapes_cpu.py plants the bugs
    this would catch)."""
    from optical_flow.utils.occlusion import flow_update
    d = _in(H, W)
    images = d["images"] if nc == 1 else d["images3"]
    uv, x = d["uvs"].astype(F), d["x"].astype(F)
    figs = []
    for clip in (True, False):
        want = uv + (np.clip(x, F(-1), F(1)) if clip else x)
        assert want.dtype == F
        uv1, occ = flow_update(d["uvs"], d["x"], clip, images)
        alone = flow_update(d["uvs"], d["x"], clip)
        assert _b(uv1) == want.tobytes(), np.argwhere(uv1 != want)[:5]
        assert _b(alone) == want.tobytes(), np.argwhere(alone != want)[:5]
        ref = O.detect_occlusion(uv1, images)
        e = float(np.abs(occ - ref).max())
        figs.append(f"clip {int(clip)}: uv1 exact, occ err {e:.2e} (occ max {ref.max():.2f})")
        assert e <= 1e-5, (clip, e, np.unravel_index(np.abs(occ - ref).argmax(), ref.shape))
    _say(f"flow_update nc {nc}", (H, W), "; ".join(figs))


# ---- c. the float2 median and the weighted median's base store ------------------
@pytest.mark.parametrize("H,W,size", [(h, w, z) for (h, w) in L.SMALL for z in S.MEDIAN_SIZES] + [L.BIG + (5,)])
def test_median_filter_flow(H, W, size):
    """of_median_filter_flow (k_median2<size>, the median the solve uses):
    the bytes of median_filter2 per component (k_median1<size>) and within
    test_median's 1e-6 of the oracle."""
    from optical_flow.utils.weighted_median import median_filter2, median_filter_flow
    uv = _in(H, W)["uv"]
    got = median_filter_flow(uv, size)
    assert _b(got) == _b(median_filter2(uv, size))
    e = float(np.abs(got - O.median_filter(uv, size)).max())
    _say(f"median2 {size}", (H, W), f"== median1, oracle {e:.2e}")
    assert e <= 1e-6, e


@pytest.mark.parametrize("guide,hsz,sig", [("gray", 7, 7.0), ("lab", 7, 7.0), ("gray", 3, 4.0), ("lab", 3, 4.0)])
@pytest.mark.parametrize("H,W", L.WMF_SHAPES, ids=_ids(L.WMF_SHAPES))
def test_weighted_median_base(H, W, guide, hsz, sig):
    """The weighted median's base store, which every Classic+NL warp ends in:
    float32(base) + (float32(wmf) - float32(base)) of the plain entry's
    output, in its bytes."""
    from optical_flow.utils.weighted_median import denoise_color_weighted_medfilt2 as wmf
    d = _in(H, W)
    g = d["guide"] if guide == "lab" else d["images"][..., 0]
    plain = wmf(d["uv"], g, d["occ"], hsz, [5, 5], sig).astype(F)
    # a generic float32 base (sigma 3 px, not on the flow's 2^-16 grid), so
    # that base + (median - base) is not the median again: the two roundings
    # are there to be seen
    base64 = S.f32(np.random.default_rng(7000 + 7 * H + W).normal(0, 3.0, (H, W, 2)))
    base = base64.astype(F)
    want = base + (plain - base)
    got = wmf(d["uv"], g, d["occ"], hsz, [5, 5], sig, base=base64)
    moved = int((want != plain).sum())
    _say(f"wmf base {guide} hsz {hsz}", (H, W), f"equal; the glue moves {moved}/{want.size} values off the median")
    assert _b(got) == want.tobytes(), np.argwhere(got != want)[:5]
    assert moved > 0 or want.size < 100


# ---- d. the level ----------------------------------------------------------------
INTERP_KERNEL = {"bi-cubic": "hermite", "cubic": "bspline", "bi-linear": "bilinear"}


def _level(ope, uv0, weight, profile):
    """(uv float32, names of the kernels that ran or None)"""
    from optical_flow import _native as nat
    ctx = nat.context()
    if not profile:
        return ope.compute_flow_base(uv0, data_weight=weight).astype(F), None
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    try:
        uv = ope.compute_flow_base(uv0, data_weight=weight).astype(F)
        n = C.c_int(0)
        names = (C.c_char_p * 256)()
        ctx.check(ctx.lib.of_kernel_times(ctx.handle, 256, names, None, None, None, C.byref(n)))
        ran = {names[i].decode() for i in range(min(n.value, 256))}
    finally:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return uv, ran


def _expected_kernels(name, ope, guide, nc, fused):
    """(must have run, must not have run)"""
    hs = ope._METHOD == 'hs'
    mf = ope._mf_size(ope.median_filter_size)
    lin = 1 if hs else int(ope.max_linear)
    warp = "warp_operator_" + INTERP_KERNEL[ope.interpolation_method]
    pd = "partial_deriv_" + INTERP_KERNEL[ope.interpolation_method]
    if fused and lin == 1 and nc in (1, 3):
        yes, no = {warp}, {pd, "flow_operator"}
    else:
        yes, no = {pd, "flow_operator"}, {warp}
    if hs:
        if name == "hs exit":
            return yes, no | {"add_update", f"median{mf}", "update", "update_occ"}
        return yes | {"add_update", f"median{mf}"}, no | {"update", "update_occ", "sub2", "axpy_diff", "wmf"}
    (yes if lin == 2 else no).add("sub2")
    if ope._METHOD == 'classic_nl' and mf and guide is not None:
        return yes | {"update_occ", "wmf"}, no | {"update", "axpy_diff", "add_update"}
    yes |= {"update", "axpy_diff"}
    no |= {"update_occ", "wmf", "add_update"}
    if mf:
        yes.add(f"median{mf}")
    return yes, no


@pytest.mark.parametrize("name", L.ARM_NAMES, ids=[n.replace(" ", "_") for n in L.ARM_NAMES])
@pytest.mark.parametrize("H,W", L.SMALL, ids=_ids(L.SMALL))
def test_level_equals_the_loop_of_stage_entries(H, W, name):
    """of_compute_flow_base[_weighted] of the arm (level_inputs.ARMS: two
    outer iterations) against level_loop(GpuBackend): equal bytes, with
    OF_OPT_FUSED_WARP at 1 and at 0.  First the level against itself (a
    second call, under profiling): the comparison means nothing without
    run-to-run repeatability.  Then, from of_kernel_times, the kernels the arm
    is meant to reach did run and the others did not."""
    from optical_flow import _abi, _native
    ope, images, guide, uv0, weight = L.arm(name, H, W, _in(H, W))
    nc = images.shape[2] // 2
    ctx = _native.context()
    assert ctx.get_option(_abi.OF_OPT_FUSED_WARP) == 1
    out = {}
    try:
        for fused in (1, 0):
            ctx.set_option(_abi.OF_OPT_FUSED_WARP, fused)
            got, _ = _level(ope, uv0, weight, False)
            again, ran = _level(ope, uv0, weight, True)
            assert np.all(np.isfinite(got))
            assert got.tobytes() == again.tobytes(), ("not repeatable", fused, int((got != again).sum()))
            yes, no = _expected_kernels(name, ope, guide, nc, fused)
            assert yes <= ran and not (no & ran), (fused, sorted(yes - ran), sorted(no & ran))
            ctx.set_option(_abi.OF_OPT_FUSED_WARP, 1)  # the stage entries run with the default
            want = LN.level_loop(LN.GpuBackend(fused), ope, images, guide, uv0, weight)
            assert want.dtype == F
            diff = (got != want).any(axis=2)
            assert got.tobytes() == want.tobytes(), (fused, int(diff.sum()), np.argwhere(diff)[:5],
                                                     float(np.abs(got - want).max()))
            out[fused] = got
    finally:
        ctx.set_option(_abi.OF_OPT_FUSED_WARP, 1)
    assert out[1].tobytes() == out[0].tobytes()
    moved = float(np.abs(out[1] - uv0).max())
    _say(f"level == loop, {name}", (H, W), f"fused and two-kernel equal; repeatable; max |uv - uv0| {moved:.3g}")
    if name == "hs exit":
        assert moved == 0.0
    else:
        assert moved > 0.0
