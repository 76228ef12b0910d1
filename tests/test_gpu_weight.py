"""GPU tests of the per-pixel data-term weight (include/optflow.h, "Per-pixel
data-term weights"): the weighted assembly kernels against their unweighted
siblings, against their own linearity in w and against the float64 oracle;
the fused and the two-kernel form; that a zero weight really removes the data
term; parity with the weighted reference (tests/golden/gen_weighted.py) and
the behaviour on a damaged frame; and what is refused."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_gpu_stages import OPS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _planes(o, alpha, uv, It, Ix, Iy, weight="sibling"):
    """(coef (7, H, W), rhs (2, H, W)) float32 straight from the C entries:
    of_flow_operator ("sibling"), or of_flow_operator_weighted with `weight`
    (None: NULL)."""
    from optical_flow import _native as nat
    H, W = uv.shape[:2]
    P = o.to_params()
    uvp, a, b, d = nat.planar(uv), nat.planar(It), nat.planar(Ix), nat.planar(Iy)
    coef = np.empty((7, H, W), dtype=np.float32)
    rhs = np.empty((2, H, W), dtype=np.float32)
    ctx = nat.context()
    head = (ctx.handle, C.byref(P), float(alpha), nat.ptr(uvp), None)
    tail = (nat.ptr(a), nat.ptr(b), nat.ptr(d), H, W, 1, nat.ptr(coef), nat.ptr(rhs))
    if isinstance(weight, str):
        ctx.check(ctx.lib.of_flow_operator(*head, *tail))
    else:
        w = None if weight is None else nat.f32(weight)
        ctx.check(ctx.lib.of_flow_operator_weighted(*head, nat.ptr(w), *tail))
    return coef, rhs


def _inputs(golden, tag, size):
    """operator.npz's 37 x 53 level, or random inputs at 37 x 70: H is no
    multiple of the 4-row block, W crosses the 64-lane wave, pitch != W."""
    d = golden("operator.npz")
    if size == "golden":
        if tag == "hs":
            It, Ix, Iy = O.partial_deriv(d["images"], d["uv"], "cubic")
        else:
            It, Ix, Iy = d["It"], d["Ix"], d["Iy"]
        return d["uv"], It, Ix, Iy
    rng = np.random.default_rng(370)
    H, W = 37, 70
    return (rng.normal(0, 0.7, (H, W, 2)), rng.normal(0, 8.0, (H, W)), rng.normal(0, 20.0, (H, W)),
            rng.normal(0, 20.0, (H, W)))


def _random_weight(shape, seed):
    """[0, 2] with exact zeros (a block and scattered pixels), ones and twos."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, shape).astype(np.float32)
    w[rng.uniform(size=shape) < 0.15] = 0.0
    w[3:9, 5:17] = 0.0
    w[0, 0], w[-1, -1], w[0, -1] = 1.0, 2.0, 0.0
    return w


def _method(meth):
    from optical_flow.methods.config import load_of_method
    return load_of_method(meth)


# ---- 1. ones and NULL are the unweighted kernels' bits ------------------------
@pytest.mark.parametrize("size", ["golden", "37x70"])
@pytest.mark.parametrize("tag,meth,alpha", OPS)
def test_operator_ones_and_null_equal_the_unweighted_entry(golden, tag, meth, alpha, size):
    o = _method(meth)
    uv, It, Ix, Iy = _inputs(golden, tag, size)
    base = _planes(o, alpha, uv, It, Ix, Iy)
    ones = _planes(o, alpha, uv, It, Ix, Iy, np.ones(uv.shape[:2]))
    null = _planes(o, alpha, uv, It, Ix, Iy, None)
    for got in (ones, null):
        assert got[0].tobytes() == base[0].tobytes()
        assert got[1].tobytes() == base[1].tobytes()


# ---- 2. linear in w, to the roundings the definition adds ----------------------
@pytest.mark.parametrize("size", ["golden", "37x70"])
@pytest.mark.parametrize("tag,meth,alpha", OPS)
def test_operator_is_linear_in_the_weight(golden, tag, meth, alpha, size):
    """E: the planes at w = 0, U: at w = 1.  The smoothness planes do not see
    w; a_uv(w) = fl(fl(psi w) ixy) against w fl(psi ixy): three roundings;
    a_uu, a_vv, b_u, b_v are E plus w times the data part U - E, with one
    extra rounding per product and per sum."""
    o = _method(meth)
    uv, It, Ix, Iy = _inputs(golden, tag, size)
    shape = uv.shape[:2]
    w = _random_weight(shape, 11)
    assert (w == 0).any() and w.max() > 1.5
    cw, bw = _planes(o, alpha, uv, It, Ix, Iy, w)
    ce, be = _planes(o, alpha, uv, It, Ix, Iy, np.zeros(shape))
    cu, bu = _planes(o, alpha, uv, It, Ix, Iy, np.ones(shape))
    assert cw[:4].tobytes() == cu[:4].tobytes() == ce[:4].tobytes()
    w64, cw, ce, cu = w.astype(np.float64), cw.astype(np.float64), ce.astype(np.float64), cu.astype(np.float64)
    bw, be, bu = bw.astype(np.float64), be.astype(np.float64), bu.astype(np.float64)
    assert np.all(ce[5] == 0)
    err = np.abs(cw[5] - w64 * cu[5])
    print(tag, size, "a_uv max err / bound", (err / np.maximum(4 * U * np.abs(w64 * cu[5]), 1e-300)).max())
    assert np.all(err <= 4 * U * np.abs(w64 * cu[5]))
    for name, gw, ge, gu in (("a_uu", cw[4], ce[4], cu[4]), ("a_vv", cw[6], ce[6], cu[6]),
                             ("b_u", bw[0], be[0], bu[0]), ("b_v", bw[1], be[1], bu[1])):
        err = np.abs(gw - (ge + w64 * (gu - ge)))
        bound = 8 * U * (np.abs(ge) + np.abs(gu))
        print(tag, size, name, "max err / bound", (err / np.maximum(bound, 1e-300)).max())
        assert np.all(err <= bound), name
    # the weight is really in there
    assert np.abs(cw[4] - cu[4]).max() > 1e-3 * np.abs(cu[4]).max()


# ---- 3. against the float64 oracle ---------------------------------------------
@pytest.mark.parametrize("tag,meth,alpha", [op for op in OPS if op[0] in ("hs", "nl_qua")])
def test_operator_against_the_oracle(golden, tag, meth, alpha):
    """With a constant psi (quadratic penalties) weighting the data term by w
    is scaling It, Ix and Iy by sqrt(w): the float64 oracle on the float32-
    rounded inputs times sqrt(w), under test_flow_operator's tolerances."""
    o = _method(meth)
    uv, It, Ix, Iy = _inputs(golden, tag, "golden")
    w = _random_weight(uv.shape[:2], 12)
    coef, rhs = o._operator_planes(uv, None, It, Ix, Iy, alpha, data_weight=w)
    s = np.sqrt(w.astype(np.float64))
    oc, orhs = O.flow_operator(o.to_params(), alpha, _f32(uv), None, _f32(It) * s, _f32(Ix) * s, _f32(Iy) * s)
    scale = np.abs(oc).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(coef - oc) <= 1e-4 * np.abs(oc) + 1e-6 * scale), np.abs(coef - oc).max()
    bscale = np.abs(orhs).max()
    assert np.all(np.abs(rhs - orhs) <= 1e-4 * np.abs(orhs) + 2e-5 * bscale)
    unweighted = O.flow_operator(o.to_params(), alpha, _f32(uv), None, _f32(It), _f32(Ix), _f32(Iy))[0]
    assert np.abs(coef[4] - unweighted[4]).max() > 1e-2 * scale[4]


# ---- 4. fused warp + assembly equals the two kernels ---------------------------
@pytest.mark.parametrize("method", ["classic+nl-fast", "hs", "ba"])
def test_fused_equals_two_kernels_with_a_weight(golden, method):
    import optical_flow
    from optical_flow import _abi, _native
    d = golden("e2e_small.npz")
    w = _random_weight(d["im1"].shape[:2], 13)
    w[20:34, 25:50] = 0.0
    ctx = _native.context()
    assert ctx.get_option(_abi.OF_OPT_FUSED_WARP) == 1
    fused = optical_flow.estimate_flow(d["im1"], d["im2"], method, data_weight=w)
    ctx.set_option(_abi.OF_OPT_FUSED_WARP, 0)
    try:
        two = optical_flow.estimate_flow(d["im1"], d["im2"], method, data_weight=w)
    finally:
        ctx.set_option(_abi.OF_OPT_FUSED_WARP, 1)
    assert np.all(np.isfinite(fused))
    np.testing.assert_array_equal(fused, two)
    plain = optical_flow.estimate_flow(d["im1"], d["im2"], method)
    assert not np.array_equal(fused, plain)


# ---- 5. a zero weight removes the pixel's data term ----------------------------
@pytest.mark.parametrize("method,alpha", [("hs", 0.0), ("ba", 1.0), ("ba", 0.0), ("classic-c", 1.0),
                                          ("classic-c", 0.0)])
def test_masked_pixels_of_frame_1_do_not_matter(method, alpha):
    """One level, 40 x 72.  Frame 1 enters a level through its own value at
    the pixel (It) and its 5-tap derivative filter there (Ix, Iy), reach
    2 px: with w = 0 on a rectangle dilated by 2 px, other values of frame 1
    inside the rectangle give the same flow, bit for bit.  (No colour guide
    in these methods, so the update kernel does not read the frames.)  With
    w = 1 there they give another flow."""
    from optical_flow.utils.synthetic import synth_pair
    im1, im2, _ = synth_pair(40, 72, 5)
    g1, g2 = im1.mean(axis=2), im2.mean(axis=2)
    r0, r1, c0, c1 = 12, 27, 20, 55
    other = g1.copy()
    other[r0:r1, c0:c1] = np.random.default_rng(5).uniform(0.0, 255.0, (r1 - r0, c1 - c0))
    w = np.ones((40, 72), dtype=np.float32)
    w[r0 - 2:r1 + 2, c0 - 2:c1 + 2] = 0.0
    yy, xx = np.mgrid[0:40, 0:72]
    uv0 = np.stack([0.4 * np.sin(xx / 9.0) + 0.3, 0.3 * np.cos(yy / 7.0) - 0.1], axis=2)

    def run(f1, weight):
        o = _method(method)
        o.images = np.stack([f1, g2], axis=2)
        o.alpha = alpha
        return o.compute_flow_base(uv0, data_weight=weight)

    a, b = run(g1, w), run(other, w)
    assert np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(run(g1, np.ones_like(w)), run(other, np.ones_like(w)))
    assert not np.array_equal(a, run(g1, None))


# ---- 6, 7. the damaged pair of tests/golden/gen_weighted.py ---------------------
RECT = (40, 75, 50, 110)


@pytest.fixture(scope="module")
def damaged(golden):
    """GPU flows on synth_pair(120, 160, 0) with frame 2 damaged, with and
    without the weight, computed once for the tests below."""
    import optical_flow
    d, s = golden("weighted.npz"), golden("e2e_synth.npz")
    im2 = d["im2_damaged"].astype(np.float64)
    out = {"gt": s["gt"]}
    for m in ("hs", "classic+nl-fast"):
        out[m, "weighted"] = optical_flow.estimate_flow(s["im1"], im2, m, data_weight=d["weight"])
        out[m, "plain"] = optical_flow.estimate_flow(s["im1"], im2, m)
    return out


@pytest.mark.parametrize("method,family", [("hs", "stable"), ("classic+nl-fast", "nlfast")])
def test_parity_with_the_weighted_reference(golden, damaged, method, family):
    """GPU flow with the weight against the reference's own code computing the
    weighted energy, under the project's gates for the same families on the
    undamaged pair of the same size (test_gpu_e2e.TOL)."""
    from test_gpu_e2e import TOL
    from conftest import epe_stats
    s = epe_stats(damaged[method, "weighted"], golden("weighted.npz")[method].astype(np.float64))
    print(method, "weighted GPU vs weighted reference", s)
    mean_tol, med_tol = TOL[family]
    assert s["mean"] < mean_tol and s["median"] < med_tol, s


@pytest.mark.parametrize("method", ["hs", "classic+nl-fast"])
def test_weight_repairs_the_damaged_region_and_leaves_the_rest(damaged, method):
    r0, r1, c0, c1 = RECT
    gt = damaged["gt"]
    inside = np.zeros(gt.shape[:2], dtype=bool)
    inside[r0:r1, c0:c1] = True
    far = np.ones(gt.shape[:2], dtype=bool)
    far[r0 - 12:r1 + 12, c0 - 12:c1 + 12] = False
    epe = {k: np.sqrt(((damaged[method, k] - gt) ** 2).sum(-1)) for k in ("weighted", "plain")}
    a_in = {k: float(e[inside].mean()) for k, e in epe.items()}
    a_far = {k: float(e[far].mean()) for k, e in epe.items()}
    print(method, "AEPE inside", a_in, "more than 12 px away", a_far)
    assert a_in["weighted"] < 0.5 * a_in["plain"]
    assert abs(a_far["weighted"] - a_far["plain"]) < 0.05


# ---- 8. refusals ----------------------------------------------------------------
def test_weight_with_general_filters_or_altba_is_refused(golden):
    import optical_flow
    d = golden("e2e_small.npz")
    w = np.ones(d["im1"].shape[:2])
    wide = {"spatial_filters": [np.array([[1, -2, 1]]), np.array([[1], [-2], [1]])]}
    with pytest.raises(NotImplementedError):
        optical_flow.estimate_flow(d["im1"], d["im2"], "classic-c", wide, data_weight=w)
    with pytest.raises(NotImplementedError):
        optical_flow.estimate_flow(d["im1"], d["im2"], "classic-c-a", data_weight=w)
    o = _method("ba")
    o.parse_input_parameter(wide)
    o.images = np.stack([d["gray1"], d["gray2"]], axis=2)
    with pytest.raises(NotImplementedError):
        o.compute_flow_base(np.zeros(w.shape + (2,)), data_weight=w)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -1.0])
def test_c_entries_refuse_a_bad_weight(bad):
    from optical_flow import _abi, _native as nat
    H, W = 24, 40
    o = _method("hs")
    P = o.to_params()
    im = nat.f32(np.random.default_rng(0).uniform(0, 255, (H, W)))
    w = np.ones((H, W), dtype=np.float32)
    w[7, 9] = bad
    out = np.full((2, H, W), 7.0, dtype=np.float32)
    ctx = nat.context()
    rc = ctx.lib.of_estimate_flow_weighted(ctx.handle, C.byref(P), nat.ptr(im), nat.ptr(im), H, W, 1, None, nat.ptr(w),
                                           nat.ptr(out), None)
    assert rc == _abi.OF_EINVAL
    assert np.all(out == 7.0)  # nothing ran
    images = np.stack([im, im])
    rc = ctx.lib.of_compute_flow_base_weighted(ctx.handle, C.byref(P), nat.ptr(images), H, W, 1, None, 0, 0.0,
                                               nat.ptr(np.zeros((2, H, W), dtype=np.float32)), nat.ptr(w),
                                               nat.ptr(out))
    assert rc == _abi.OF_EINVAL
