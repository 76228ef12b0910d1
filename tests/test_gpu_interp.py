"""Image warping and occlusion-aware frame interpolation on the GPU:
of_warp_image, of_interp_frames and of_estimate_interp (include/optflow.h;
k_warp_image, k_interp_splat / _resolve / _fill / _render).

The kernels are compared bitwise with the numpy float64 restatement below,
which follows the header's formulas operation for operation (the kernels run
them in double with no fma contraction, and the splat's winner is the minimum
of an order-independent 64-bit key)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- the numpy restatement --------------------------------------------------
def bil_numpy(A, r, q):
    """bil(A_c, r, q) for every channel: A (H, W, C) float64, r / q finite
    float64 arrays of one shape -> that shape + (C,)."""
    H, W = A.shape[:2]
    qc = np.minimum(np.maximum(q, 0.0), float(W - 1))
    rc = np.minimum(np.maximum(r, 0.0), float(H - 1))
    qf, rf = np.floor(qc), np.floor(rc)
    j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
    fc, fr = (qc - qf)[..., None], (rc - rf)[..., None]
    j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
    return ((1.0 - fr) * ((1.0 - fc) * A[i0, j0] + fc * A[i0, j1])
            + fr * ((1.0 - fc) * A[i1, j0] + fc * A[i1, j1]))


def inside_numpy(r, q, H, W):
    return (q >= 0) & (q <= W - 1) & (r >= 0) & (r <= H - 1)


def near_numpy(x, n):
    return np.minimum(np.maximum(np.floor(x + 0.5), 0.0), float(n - 1)).astype(np.int64)


def fb_numpy(fw, bw, alpha1, alpha2):
    """The state of of_fb_consistency (include/optflow.h) in numpy float64."""
    H, W = fw.shape[:2]
    ii, jj = np.mgrid[0:H, 0:W]
    u, v = fw[..., 0].astype(np.float64), fw[..., 1].astype(np.float64)
    B = bw.astype(np.float64)
    with np.errstate(all="ignore"):
        q, r = jj + u, ii + v
        inside = inside_numpy(r, q, H, W)
        q, r = np.where(inside, q, 0.0), np.where(inside, r, 0.0)
        qf, rf = np.floor(q), np.floor(r)
        j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
        fc, fr = q - qf, r - rf
        j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
        bu, bv = [(1.0 - fr) * ((1.0 - fc) * B[i0, j0, k] + fc * B[i0, j1, k])
                  + fr * ((1.0 - fc) * B[i1, j0, k] + fc * B[i1, j1, k]) for k in range(2)]
        du, dv = u + bu, v + bv
        err = du * du + dv * dv
        thr = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2
    return np.where(inside, (err > thr).astype(np.uint8), np.uint8(2)).astype(np.uint8)


def _img3(im):
    a = np.asarray(im, dtype=np.float32)
    return (a[..., None] if a.ndim == 2 else a).astype(np.float64)


def warp_numpy(im, uv):
    """of_warp_image: (float32 image of im's shape, bool valid)."""
    A = _img3(im)
    H, W = A.shape[:2]
    uv = np.asarray(uv, dtype=np.float32)
    ii, jj = np.mgrid[0:H, 0:W]
    fin = np.isfinite(uv[..., 0]) & np.isfinite(uv[..., 1])
    u = np.where(fin, uv[..., 0], np.float32(0)).astype(np.float64)
    v = np.where(fin, uv[..., 1], np.float32(0)).astype(np.float64)
    r, q = ii + v, jj + u
    out = np.where(fin[..., None], bil_numpy(A, r, q), 0.0).astype(np.float32)
    return out.reshape(np.shape(im)), fin & inside_numpy(r, q, H, W)


def interp_numpy(im1, im2, fw, bw, t, alpha1=0.01, alpha2=0.5):
    """of_interp_frames for one t: (out float32 of im1's shape, ut (H, W, 2)
    float32, info (H, W) uint8, number of fill passes)."""
    I1, I2 = _img3(im1), _img3(im2)
    H, W = I1.shape[:2]
    fw = np.asarray(fw, dtype=np.float32)
    bw = np.asarray(bw, dtype=np.float32)
    Sf, Sb = fb_numpy(fw, bw, alpha1, alpha2), fb_numpy(bw, fw, alpha1, alpha2)
    t = float(t)
    omt = 1.0 - t
    ii, jj = np.mgrid[0:H, 0:W]
    src = (ii * W + jj).astype(np.uint64)
    key = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    # 1. splat
    for f, flow, tau in ((0, fw, t), (1, bw, omt)):
        fin = np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
        g = np.where(fin[..., None], flow, np.float32(0))
        u, v = g[..., 0].astype(np.float64), g[..., 1].astype(np.float64)
        m = -g if f else g  # fp32 negation, exact
        a, b = m[..., 0].astype(np.float64), m[..., 1].astype(np.float64)
        q, r = jj + tau * u, ii + tau * v
        jf, i_f = np.floor(q), np.floor(r)
        for di in (0, 1):
            for dj in (0, 1):
                ti, tj = i_f + di, jf + dj
                ok = fin & inside_numpy(ti, tj, H, W)
                if dj:
                    ok &= q != jf
                if di:
                    ok &= r != i_f
                ti, tj = np.where(ok, ti, 0.0), np.where(ok, tj, 0.0)
                d = np.abs(bil_numpy(I1, ti - t * b, tj - t * a) - bil_numpy(I2, ti + omt * b, tj + omt * a))
                cost = np.zeros((H, W))
                for c in range(d.shape[2]):
                    cost = cost + d[..., c]
                bits = cost.astype(np.float32).view(np.uint32).astype(np.uint64)
                K = (bits << np.uint64(32)) | np.uint64(f << 31) | src
                idx = (ti.astype(np.int64) * W + tj.astype(np.int64))[ok]
                np.minimum.at(key, idx, K[ok])
    # 2. resolve
    key = key.reshape(H, W)
    hole = key == np.uint64(0xFFFFFFFFFFFFFFFF)
    s = (key & np.uint64(0x7FFFFFFF)).astype(np.int64)
    s = np.where(hole, 0, s)
    from_b = (key >> np.uint64(31)) & np.uint64(1) == 1
    ut = np.where(from_b[..., None], -bw.reshape(-1, 2)[s], fw.reshape(-1, 2)[s]).astype(np.float32)
    ut[hole] = 0
    # 3. fill
    filled = np.zeros((H, W), bool)
    passes = 0
    while hole.any():
        known = ~hole
        su, sv, cnt = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
        pk = np.pad(known, 1)
        pu = np.pad(np.where(known, ut[..., 0], np.float32(0)).astype(np.float64), 1)
        pv = np.pad(np.where(known, ut[..., 1], np.float32(0)).astype(np.float64), 1)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                sl = (slice(1 + di, 1 + di + H), slice(1 + dj, 1 + dj + W))
                k = pk[sl]
                su = np.where(k, su + pu[sl], su)
                sv = np.where(k, sv + pv[sl], sv)
                cnt += k
        take = hole & (cnt > 0)
        passes += 1
        if not take.any():  # no pixel has a motion
            ut[:] = 0
            break
        with np.errstate(all="ignore"):
            ut[..., 0] = np.where(take, (su / cnt).astype(np.float32), ut[..., 0])
            ut[..., 1] = np.where(take, (sv / cnt).astype(np.float32), ut[..., 1])
        filled |= take
        hole = hole & ~take
    # 4. render
    a, b = ut[..., 0].astype(np.float64), ut[..., 1].astype(np.float64)
    r1, q1 = ii - t * b, jj - t * a
    r2, q2 = ii + omt * b, jj + omt * a
    in1, in2 = inside_numpy(r1, q1, H, W), inside_numpy(r2, q2, H, W)
    o1 = in1 & (Sf[near_numpy(r1, H), near_numpy(q1, W)] == 1)
    o2 = in2 & (Sb[near_numpy(r2, H), near_numpy(q2, W)] == 1)
    w1, w2 = in1 & ~o2 & ~hole, in2 & ~o1 & ~hole
    s1, s2 = bil_numpy(I1, r1, q1), bil_numpy(I2, r2, q2)
    blend = omt * s1 + t * s2
    out = np.where((w1 == w2)[..., None], blend, np.where(w1[..., None], s1, s2)).astype(np.float32)
    info = np.where(w1 & w2, 0, np.where(w1, 1, np.where(w2, 2, 3))).astype(np.uint8) | (filled * np.uint8(4))
    return out.reshape(np.shape(im1)), ut, info.astype(np.uint8), passes


# ---- helpers ----------------------------------------------------------------
def _launch_counts(fn):
    from optical_flow import _native
    ctx = _native.context()
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    try:
        fn()
        n = C.c_int(0)
        names = (C.c_char_p * 512)()
        counts = (C.c_int64 * 512)()
        ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, None, counts, None, C.byref(n)))
        assert n.value <= 512
        return {names[k].decode(): counts[k] for k in range(n.value)}
    finally:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))


def tex(s, y, x):
    return 128 + 60 * np.sin(0.37 * x + 0.21 * y + s) * np.cos(0.29 * y - 0.17 * x + 2 * s)


def planted_case(H, W, Cc):
    """Seeded frames and flows in +-6 px with the edge cases planted: an
    integer displacement, -0.0, a NaN and an Inf component, one of 1e30."""
    rng = np.random.default_rng(1000 * H + W + 7 * Cc)
    shp = (H, W) if Cc == 1 else (H, W, Cc)
    im1 = rng.uniform(0, 255, shp).astype(np.float32)
    im2 = rng.uniform(0, 255, shp).astype(np.float32)
    fw = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    bw = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    n = H * W
    pix = lambda k: divmod(k, W)  # noqa: E731
    fw[pix(n - 1)] = (-0.0, -0.0)
    if n >= 5:
        fw[0, 0] = (min(1, W - 1), min(1, H - 1))  # integer displacement: zero-weight targets
        bw[pix(n // 2)] = (-1.0, 0.0) if W > 1 else (0.0, -1.0)
        i, j = pix(1)
        fw[i, j, 0] = np.nan
        i, j = pix(n - 2)
        bw[i, j, 1] = np.inf
        i, j = pix(2)
        fw[i, j, 1] = 1e30
        i, j = pix(3)
        bw[i, j, 0] = -1e30
    return im1, im2, fw, bw


SHAPES = [(1, 1), (1, 7), (5, 1), (37, 53), (3, 130), (64, 65)]


# ---- 1. bitwise against numpy -----------------------------------------------
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernels_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    im1, im2, fw, bw = planted_case(H, W, Cc)
    ts = [0.5, 0.3, 0.8125]
    outs, uts, infos = optical_flow.interpolate_frames(im1, im2, ts, flows=(fw, bw), return_info=True)
    assert len(outs) == len(uts) == len(infos) == 3
    for k, t in enumerate(ts):
        ro, ru, ri, _ = interp_numpy(im1, im2, fw, bw, t)
        assert outs[k].dtype == np.float64 and outs[k].shape == im1.shape
        assert uts[k].shape == (H, W, 2) and infos[k].dtype == np.uint8 and infos[k].shape == (H, W)
        assert np.array_equal(uts[k].astype(np.float32), ru), (t, np.argwhere(uts[k].astype(np.float32) != ru)[:5])
        assert np.array_equal(infos[k], ri), (t, np.argwhere(infos[k] != ri)[:5])
        assert np.array_equal(outs[k].astype(np.float32), ro), t
        assert np.all(np.isfinite(uts[k])) and np.all(np.isfinite(outs[k]))
    # one t at a time gives the same frames; a scalar t gives an array
    for k in (0, 1):
        o, u, i = optical_flow.interpolate_frames(im1, im2, ts[k], flows=(fw, bw), return_info=True)
        assert np.array_equal(o, outs[k]) and np.array_equal(u, uts[k]) and np.array_equal(i, infos[k])
        assert np.array_equal(optical_flow.interpolate_frames(im1, im2, ts[k], flows=(fw, bw)), outs[k])
    if H * W > 1000:
        assert all((infos[0] & 3 == k).any() for k in (0, 1, 2, 3))
    # other thresholds reach the masks
    o2, _, i2 = optical_flow.interpolate_frames(im1, im2, 0.5, flows=(fw, bw), alpha1=0.0, alpha2=1e-4,
                                                return_info=True)
    r2 = interp_numpy(im1, im2, fw, bw, 0.5, 0.0, 1e-4)
    assert np.array_equal(o2.astype(np.float32), r2[0]) and np.array_equal(i2, r2[2])
    # warp_image on the same inputs
    for im, uv in ((im1, fw), (im2, bw)):
        w, valid = optical_flow.warp_image(im, uv)
        rw, rv = warp_numpy(im, uv)
        assert w.dtype == np.float64 and w.shape == im.shape and valid.dtype == bool and valid.shape == (H, W)
        assert np.array_equal(w.astype(np.float32), rw) and np.array_equal(valid, rv)
    if H * W >= 5:
        _, valid = optical_flow.warp_image(im1, fw)
        assert valid[0, 0] and not valid[divmod(1, W)] and not valid[divmod(2, W)]


# ---- 2. hole filling ----------------------------------------------------------
def test_hole_filling_loops_until_no_hole_is_left():
    import optical_flow
    H, W = 37, 53
    rng = np.random.default_rng(5)
    im1 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    im2 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    fw = np.full((H, W, 2), np.nan, np.float32)
    bw = np.full((H, W, 2), np.nan, np.float32)
    fw[20, 11] = (2.5, -1.25)
    ro, ru, ri, passes = interp_numpy(im1, im2, fw, bw, 0.5)
    assert passes == 39  # the Chebyshev distance of column 52 from the 2 x 2 splatted targets
    res = {}
    counts = _launch_counts(lambda: res.update(r=optical_flow.interpolate_frames(
        im1, im2, 0.5, flows=(fw, bw), return_info=True)))
    o, u, i = res["r"]
    assert counts["interp_fill"] == passes
    assert np.array_equal(o.astype(np.float32), ro) and np.array_equal(u.astype(np.float32), ru)
    assert np.array_equal(i, ri)
    splatted = np.zeros((H, W), bool)
    splatted[19:21, 12:14] = True  # (20 - 0.625, 11 + 1.25) -> rows 19, 20 and columns 12, 13
    assert np.array_equal((i & 4) != 0, ~splatted)
    assert np.all(np.isfinite(u)) and np.all(u == np.float32([2.5, -1.25]))


def test_no_finite_flow_at_all():
    import optical_flow
    H, W = 37, 53
    rng = np.random.default_rng(6)
    im1 = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    im2 = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    nan = np.full((H, W, 2), np.nan, np.float32)
    res = {}
    counts = _launch_counts(lambda: res.update(r=optical_flow.interpolate_frames(
        im1, im2, 0.25, flows=(nan, nan), return_info=True)))
    o, u, i = res["r"]
    assert counts["interp_fill"] == 1  # the pass that found nothing to fill ends the loop
    assert np.all(u == 0) and np.all(i == 3)
    assert np.array_equal(o.astype(np.float32), (0.75 * im1.astype(np.float64) + 0.25 * im2).astype(np.float32))
    ro, ru, ri, _ = interp_numpy(im1, im2, nan, nan, 0.25)
    assert np.array_equal(o.astype(np.float32), ro) and np.array_equal(i, ri) and np.all(ru == 0)


def test_expanding_flow_leaves_holes_filled_in_one_pass():
    import optical_flow
    H, W = 37, 53
    rng = np.random.default_rng(7)
    im1 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    im2 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    ii, jj = np.mgrid[0:H, 0:W]
    fw = np.stack([1.5 * (jj - 26), 1.5 * (ii - 18)], -1).astype(np.float32)
    bw = np.full((H, W, 2), np.nan, np.float32)
    res = {}
    counts = _launch_counts(lambda: res.update(r=optical_flow.interpolate_frames(
        im1, im2, 0.9, flows=(fw, bw), return_info=True)))
    o, u, i = res["r"]
    assert counts["interp_fill"] == 1
    assert int(((i & 4) != 0).sum()) == 566
    ro, ru, ri, passes = interp_numpy(im1, im2, fw, bw, 0.9)
    assert passes == 1
    assert np.array_equal(o.astype(np.float32), ro) and np.array_equal(u.astype(np.float32), ru)
    assert np.array_equal(i, ri)


# ---- 3. identity --------------------------------------------------------------
def test_identity():
    import optical_flow
    im1 = np.random.default_rng(8).uniform(0, 255, (21, 34, 3))
    z = np.zeros((21, 34, 2))
    res = {}
    counts = _launch_counts(lambda: res.update(r=optical_flow.interpolate_frames(
        im1, im1, 0.3, flows=(z, z), return_info=True)))
    o, u, i = res["r"]
    assert np.array_equal(o, im1.astype(np.float32).astype(np.float64))
    assert np.all(i == 0) and np.all(u == 0)
    assert "interp_fill" not in counts  # no hole: the loop is skipped
    w, valid = optical_flow.warp_image(im1, z)
    assert np.array_equal(w, im1.astype(np.float32).astype(np.float64)) and valid.all()


# ---- 4. two-layer occlusion scene ----------------------------------------------
def two_layer(t):
    """Frame at time t: static background tex(1), foreground tex(5) on
    x in [12, 31], y in [10, 29] at t = 0, moving 8 px in +x per frame."""
    H, W = 40, 64
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 8.0 * t
    fg = (xx - d >= 12) & (xx - d <= 31) & (yy >= 10) & (yy <= 29)
    return np.where(fg, tex(5, yy, xx - d), tex(1, yy, xx)), fg


@pytest.mark.parametrize("t,n0,n1,n2", [(0.5, 2400, 80, 80), (0.25, 2400, 120, 40)])
def test_two_layer_occlusion_scene(t, n0, n1, n2):
    import optical_flow
    im1, fg1 = two_layer(0.0)
    im2, fg2 = two_layer(1.0)
    want, _ = two_layer(t)
    fw = np.zeros((40, 64, 2))
    bw = np.zeros((40, 64, 2))
    fw[fg1, 0] = 8.0
    bw[fg2, 0] = -8.0
    o, u, i = optical_flow.interpolate_frames(im1, im2, t, flows=(fw, bw), return_info=True)
    avg_err = np.abs(0.5 * (im1 + im2) - want).mean()
    bad = o.astype(np.float32) != want.astype(np.float32)
    print(f"t={t}: {int(bad.sum())} pixels differ from the analytic frame; info counts "
          f"{[int((i & 3 == k).sum()) for k in range(4)]}, filled {int((i & 4 != 0).sum())}; "
          f"mean |plain average - analytic| {avg_err:.3f}")
    assert not bad.any(), np.argwhere(bad)[:8]
    assert [int((i == k).sum()) for k in (0, 1, 2)] == [n0, n1, n2]
    if t == 0.5:
        assert abs(avg_err - 5.3) < 0.05
    ro, ru, ri, _ = interp_numpy(im1, im2, fw, bw, t)
    assert np.array_equal(o.astype(np.float32), ro) and np.array_equal(i, ri)


# ---- 5. one call equals two -----------------------------------------------------
@pytest.fixture(scope="module")
def pair48():
    from optical_flow.utils.synthetic import synth_pair
    a, b, _ = synth_pair(48, 64, seed=3)
    return a, b


@pytest.mark.parametrize("method", ["classic+nl-fast", "hs-brightness"])
def test_one_call_equals_two(pair48, method):
    import optical_flow
    im1, im2 = pair48
    ts = [0.25, 0.5]
    res = {}
    one = _launch_counts(lambda: res.update(a=optical_flow.interpolate_frames(im1, im2, ts, method)))
    r = optical_flow.estimate_flow_bidirectional(im1, im2, method)
    two = _launch_counts(lambda: res.update(b=optical_flow.interpolate_frames(im1, im2, ts, flows=r)))
    assert len(res["a"]) == 2 and res["a"][0].shape == im1.shape and res["a"][0].dtype == np.float64
    for x, y in zip(res["a"], res["b"]):
        assert np.array_equal(x, y)
    assert not np.array_equal(res["a"][0], res["a"][1])
    for counts in (one, two):
        assert counts["fb_check"] == 1
        assert counts["interp_splat"] == counts["interp_resolve"] == counts["interp_render"] == 2
    # the frames along the estimated flows with the info, and a tuple of flows
    o, _, i = optical_flow.interpolate_frames(im1, im2, 0.5, method, return_info=True)
    assert np.array_equal(o, res["a"][1]) and i.shape == (48, 64)
    assert np.array_equal(optical_flow.interpolate_frames(im1, im2, 0.5, flows=(r.forward, r.backward)), res["a"][1])


# ---- 6. end to end beats averaging -----------------------------------------------
def test_end_to_end_beats_averaging():
    import optical_flow
    H, W = 48, 64
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frame = lambda t: tex(1, yy + 2.0 * t, xx - 4.0 * t)  # noqa: E731  the scene moves (4, -2) px per frame
    im1, im2, mid = frame(0.0), frame(1.0), frame(0.5)
    o = optical_flow.interpolate_frames(im1, im2, 0.5, "classic+nl-fast")
    m = (slice(8, H - 8), slice(8, W - 8))
    e_int, e_avg = np.abs(o - mid)[m].mean(), np.abs(0.5 * (im1 + im2) - mid)[m].mean()
    print(f"48x64 translating scene, interior: mean |interpolated - analytic| {e_int:.3e}, "
          f"mean |average - analytic| {e_avg:.3e}, ratio {e_int / e_avg:.3e}")
    assert e_int < e_avg


# ---- 7. refusals -------------------------------------------------------------------
def test_refusals(pair48):
    import optical_flow
    from optical_flow import _native
    im1, im2 = pair48
    z = np.zeros((48, 64, 2))
    for bad_t in (0.0, 1.0, float("nan"), -0.1, [], [0.5, 1.5]):
        with pytest.raises(ValueError):
            optical_flow.interpolate_frames(im1, im2, bad_t, flows=(z, z))
    for a1 in (-0.01, float("nan")):
        with pytest.raises(ValueError):
            optical_flow.interpolate_frames(im1, im2, 0.5, flows=(z, z), alpha1=a1)
        with pytest.raises(ValueError):
            optical_flow.interpolate_frames(im1, im2, 0.5, alpha1=a1)
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(im1, im2, 0.5, flows=(z, z), alpha2=float("inf"))
    five = np.zeros((48, 64, 5))
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(five, five, 0.5, flows=(z, z))
    with pytest.raises(ValueError):
        optical_flow.warp_image(five, z)
    # the C entries check for themselves
    ctx = _native.context()
    a, b, f = _native.f32(im1), _native.f32(im2), _native.f32(np.zeros((2, 48, 64)))
    out = np.empty((48, 64, 3), np.float32)
    P = optical_flow.load_of_method("classic+nl-fast").to_params()

    def interp(ctx, Cc=3, t=0.5, a1=0.01, n=1):
        tt = (C.c_double * 1)(t)
        return ctx.lib.of_interp_frames(ctx.handle, _native.ptr(a), _native.ptr(b), 48, 64, Cc, _native.ptr(f),
                                        _native.ptr(f), a1, 0.5, n, tt, _native.ptr(out), None, None)

    def estimate(ctx, Cc=3, t=0.5, a1=0.01, n=1):
        tt = (C.c_double * 1)(t)
        return ctx.lib.of_estimate_interp(ctx.handle, C.byref(P), _native.ptr(a), _native.ptr(b), 48, 64, Cc, a1, 0.5,
                                          n, tt, _native.ptr(out), None, None, None, None, None)

    def warp(ctx, Cc=3):
        return ctx.lib.of_warp_image(ctx.handle, _native.ptr(a), 48, 64, Cc, _native.ptr(f), _native.ptr(out), None)

    for kw in ({"t": 0.0}, {"t": 1.0}, {"t": float("nan")}, {"n": 0}, {"a1": -1.0}, {"Cc": 0}, {"Cc": 5}):
        for fn in (interp, estimate):
            with pytest.raises(ValueError):
                ctx.check(fn(ctx, **kw))
    with pytest.raises(ValueError):
        ctx.check(estimate(ctx, Cc=2))
    for Cc in (0, 5):
        with pytest.raises(ValueError):
            ctx.check(warp(ctx, Cc))
    ctx.check(interp(ctx))  # and the good call goes through
    # H * W >= 2^31 does not fit the key's source index: refused before any buffer is read
    tt = (C.c_double * 1)(0.5)
    with pytest.raises(NotImplementedError):
        ctx.check(ctx.lib.of_interp_frames(ctx.handle, _native.ptr(a), _native.ptr(b), 46341, 46341, 1, _native.ptr(f),
                                           _native.ptr(f), 0.01, 0.5, 1, tt, _native.ptr(out), None, None))
    # while a pair stream is open on the context
    with optical_flow.PairStream(48, 64, 3, "classic+nl-fast", lanes=1) as ps:
        for fn in (interp, estimate, warp):
            with pytest.raises(ValueError, match="pair stream is open"):
                ps._ctx.check(fn(ps._ctx))
