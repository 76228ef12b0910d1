"""Global motion estimation and stabilisation on the GPU: of_fit_motion and
of_warp_affine bitwise against the numpy float64 restatement
(tests/motion_numpy.py), the session (of_stab_*) bitwise against its parts run
by hand, its lifecycle, and an end-to-end run on a jittering clip."""
import ctypes as C
import math

import numpy as np
import pytest

import motion_numpy as mn

pytestmark = pytest.mark.gpu

# the reduction's seams: one partial tile; a partial third tile column; a second tile row of one
# row; 72 tiles (two group levels); 4097 tiles (three group levels); the two-layer scene
FIT_SHAPES = [(1, 1), (1, 7), (5, 1), (3, 130), (9, 64), (37, 53), (64, 65), (72, 449), (32776, 1), (120, 160)]
WARP_SHAPES = [(1, 1), (1, 7), (5, 1), (3, 130), (37, 53), (64, 65)]
MODELS = ("translation", "similarity", "affine")


def plant(flow):
    """The interpolation and fusion tests' planted cases in an (H, W, 2)
    float32 flow, returned with the pixels that hold +-1e30."""
    H, W = flow.shape[:2]
    n = H * W
    pix = lambda k: divmod(k, W)  # noqa: E731
    flow[pix(n - 1)] = (-0.0, -0.0)
    huge = []
    if n >= 5:
        flow[0, 0] = (min(1, W - 1), min(1, H - 1))  # an integer displacement
        i, j = pix(1)
        flow[i, j, 0] = np.nan
        i, j = pix(n - 2)
        flow[i, j, 1] = np.inf
        i, j = pix(2)
        flow[i, j, 1] = 1e30
        i, j = pix(3)
        flow[i, j, 0] = -1e30
        huge = [pix(2), pix(3)]
    return flow, huge


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_same_fit(got, want, key):
    """Every number of the fit as bits."""
    for name in ("theta", "matrix", "cutoff", "support", "rms"):
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), \
            (key, name, getattr(got, name), getattr(want, name))
    assert (got.passes, got.degenerate) == (want.passes, want.degenerate), (key, got.passes, got.degenerate)
    bad = np.argwhere(got.inliers.astype(np.float32).view(np.uint32) != want.inliers.view(np.uint32))
    assert bad.size == 0, (key, bad[:5])


@pytest.mark.parametrize("H,W", FIT_SHAPES)
def test_fit_motion_bitwise_vs_numpy(H, W):
    """The three models on a seeded +-6 px flow (the scene's at 120 x 160) with
    the planted cases, in four forms: as it is (the +-1e30 pixels are finite
    and enter the sums: the first cutoff is of their size, and every number
    stays finite); with a weight plane; with a state plane that also masks the
    +-1e30 pixels (the cutoff schedule then runs on the +-6 px data); with
    both."""
    import optical_flow
    rng = np.random.default_rng(1000 * H + W)
    if (H, W) == (120, 160):
        from test_motion_cpu import scene
        base = scene()[0]
    else:
        base = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    flow, huge = plant(base)
    weight = rng.uniform(0, 2, (H, W)).astype(np.float32)
    weight[rng.uniform(size=(H, W)) < 0.1] = 0.0
    state = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    state_h = state.copy()
    for k, p in enumerate(huge):
        state_h[p] = 1 + k
    seen = set()
    for model in MODELS:
        for name, w, s in (("plain", None, None), ("weight", weight, None), ("state", None, state_h),
                           ("both", weight, state)):
            key = (model, name)
            want = mn.fit(flow, model, w, s)
            got = optical_flow.fit_motion(flow, model, w, s, return_inliers=True)
            assert got.matrix.shape == (2, 3) and got.theta.shape == (6,) and got.inliers.dtype == np.float64
            assert_same_fit(got, want, key)
            assert all(math.isfinite(x) for x in (*got.theta, *got.matrix.ravel(), got.cutoff, got.support)), key
            only = optical_flow.fit_motion(flow, model, w, s)
            assert only.inliers is None and np.array_equal(bits(only.theta), bits(got.theta))
            if w is None:  # the inlier plane is the Tukey weight itself
                inl = want.inliers
                seen |= {"masked"} if want.masked.any() else set()
                seen |= {"zero"} if (inl[~want.masked] == 0).any() else set()
                seen |= {"part"} if ((inl > 0) & (inl < 1)).any() else set()
        # other options: no robust pass; a slow decay from a tight start
        for kw in (dict(iters=0), dict(iters=3, kappa=0.7, decay=0.9, c_min=0.125)):
            want = mn.fit(flow, model, None, state_h, **kw)
            got = optical_flow.fit_motion(flow, model, None, state_h, return_inliers=True, **kw)
            assert_same_fit(got, want, (model, tuple(kw.items())))
    if H * W > 1000:
        assert seen == {"masked", "zero", "part"}, seen  # every branch of the weight occurs


def test_fit_motion_scene_and_degenerate_flows():
    import optical_flow
    from test_motion_cpu import TH_SIM, scene
    f, fg = scene()
    for model in ("affine", "similarity"):
        r = optical_flow.fit_motion(f, model, return_inliers=True)
        assert np.abs(r.theta - np.array(TH_SIM)).max() <= 0.01 and r.degenerate == 0
        assert r.inliers[fg].max() == 0.0 and r.inliers[~fg].mean() > 0.7
        assert np.abs(optical_flow.fit_motion(f, model, iters=0).theta - np.array(TH_SIM)).max() > 1.0
    # no support: the fit stops at pass 0 with zero parameters
    for kw in (dict(state=np.ones((120, 160), np.uint8)), dict(weight=np.zeros((120, 160)))):
        r = optical_flow.fit_motion(f, "affine", return_inliers=True, **kw)
        assert_same_fit(r, mn.fit(f, "affine", **kw), tuple(kw))
        assert r.degenerate == 2 and r.passes == 1 and not r.theta.any() and r.support == 0.0 and math.isnan(r.rms)
        assert np.array_equal(r.matrix, [[1, 0, 0], [0, 1, 0]]) and not r.inliers.any()
    r = optical_flow.fit_motion(np.full((9, 70, 2), np.nan), "similarity")
    assert r.degenerate == 2 and not r.theta.any()


def warp_matrices(H, W):
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    a, b = 1.1 * math.cos(0.2), 1.1 * math.sin(0.2)  # a rotation by 0.2 rad and a zoom of 1.1 about the centre
    return {"identity": mn.I6, "half pixel": (1, 0, 0.5, 0, 1, -0.5),
            "rotation and zoom": (a, -b, cx - (a * cx - b * cy), b, a, cy - (b * cx + a * cy)),
            "nan": (1, 0, 0, 0, float("nan"), 0), "outside": (1, 0, 1e6, 0, 1, -1e6),
            "infinite": (float("inf"), 0, 0, 0, 1, 0)}


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", WARP_SHAPES)
def test_warp_affine_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    rng = np.random.default_rng(100 * H + W + Cc)
    im = rng.uniform(0, 255, (H, W) if Cc == 1 else (H, W, Cc)).astype(np.float32)
    for name, A in warp_matrices(H, W).items():
        A = np.reshape(np.array(A, dtype=np.float64), (2, 3))
        want, want_v = mn.warp_affine(im, A)
        out, valid = optical_flow.warp_affine(im, A, return_valid=True)
        assert out.dtype == np.float64 and out.shape == im.shape and valid.dtype == np.uint8 and valid.shape == (H, W)
        assert np.array_equal(valid, want_v), name
        assert np.array_equal(out.astype(np.float32).view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(optical_flow.warp_affine(im, A), out)
        if name == "identity":
            assert valid.all() and np.array_equal(out, im.astype(np.float64))
        if name in ("nan", "outside", "infinite"):
            assert not valid.any() and not out.any()
    if H * W > 1000:
        v = mn.warp_affine(im, np.reshape(warp_matrices(H, W)["rotation and zoom"], (2, 3)))[1]
        assert 0 < v.sum() < H * W  # sources inside and outside the frame


# ---- the session equals its parts ------------------------------------------
RADIUS, SIGMA_T = 2, 3.0


@pytest.fixture(scope="module")
def clip():
    """A 6-frame 48 x 64 clip and (forward flow, forward mask) of every
    adjacent pair from estimate_flow_bidirectional, computed once."""
    import optical_flow
    from test_gpu_fuse import clip_frames
    frames = clip_frames(48, 64, 1, 6, 41, 2.0)
    pairs = []
    for a, b in zip(frames[:-1], frames[1:]):
        r = optical_flow.estimate_flow_bidirectional(a, b, "classic+nl-fast")
        pairs.append((r.forward, r.occ_forward))
    return frames, pairs


def run_session(frames, **kw):
    """[(index, frame, transform, valid)] by index and the motions, from a
    Stabilizer over the frames."""
    import optical_flow
    out, motions, order = {}, [], []
    with optical_flow.Stabilizer(frames[0].shape, "classic+nl-fast", **kw) as st:
        for k, f in enumerate(frames):
            r = st.push(f)
            if k == 0:
                assert st.last_motion is None
            else:
                motions.append(st.last_motion.copy())
            order.append(-1 if r is None else r[0])
            if r is not None:
                out[r[0]] = (r[1], st.last_transform, st.last_valid, st.last_degenerate)
        for r in st.flush():
            assert st.last_motion is None
            order.append(r[0])
            out[r[0]] = (r[1], st.last_transform, st.last_valid, st.last_degenerate)
        assert list(st.flush()) == []
        order.append(-1)
    return out, motions, order


@pytest.mark.parametrize("model", ["similarity", "affine"])
def test_session_equals_its_parts(clip, model):
    import optical_flow
    frames, pairs = clip
    out, motions, order = run_session(frames, model=model, radius=RADIUS, sigma_t=SIGMA_T)
    assert order == [-1, -1, 0, 1, 2, 3, 4, 5, -1]
    # the motions are fit_motion on each pair's forward flow and mask
    assert len(motions) == 5
    for k, (fw, occ) in enumerate(pairs):
        want = optical_flow.fit_motion(fw, model, state=occ)
        assert want.degenerate == 0
        assert np.array_equal(bits(motions[k]), bits(want.matrix)), (k, motions[k], want.matrix)
    # the window moves by (-2, 1) px per frame over the canvas, the content by (2, -1)
    print(f"{model}: motions' translations {np.round([m[:, 2] for m in motions], 3).tolist()}")
    kept = [mn.keep(m)[0] for m in motions]
    pushes, flush = mn.session_schedule(6, RADIUS)
    sched = {t: n for t, n in pushes + flush if t >= 0}
    for t in range(6):
        o, S, valid, deg = out[t]
        want_S = mn.smooth(kept, t, sched[t], RADIUS, SIGMA_T)
        assert np.array_equal(bits(S), bits(want_S)), (t, S, want_S)
        assert deg == 0
        inv = np.reshape(mn.inv(S), (2, 3))
        want_o, want_v = optical_flow.warp_affine(frames[t], inv, return_valid=True)
        assert o.dtype == np.float64 and o.shape == frames[0].shape
        assert np.array_equal(o, want_o), (t, np.abs(o - want_o).max())
        assert np.array_equal(valid, want_v), t
    all_o, all_S = optical_flow.stabilize_frames(frames, "classic+nl-fast", model, RADIUS, SIGMA_T,
                                                 return_transforms=True)
    assert all_o.shape == (6, 48, 64) and all_S.shape == (6, 2, 3) and all_o.dtype == np.float64
    for t in range(6):
        assert np.array_equal(all_o[t], out[t][0]) and np.array_equal(bits(all_S[t]), bits(out[t][1])), t
    assert np.array_equal(optical_flow.stabilize_frames(frames, "classic+nl-fast", model, RADIUS, SIGMA_T), all_o)


def test_session_on_rgb_frames_and_a_clip_shorter_than_the_radius():
    import optical_flow
    from test_gpu_fuse import clip_frames
    frames = clip_frames(32, 40, 3, 3, 43, 2.0)
    out, motions, order = run_session(frames, radius=4)
    assert order == [-1, -1, -1, 0, 1, 2, -1] and len(motions) == 2
    for k in range(2):
        r = optical_flow.estimate_flow_bidirectional(frames[k], frames[k + 1], "classic+nl-fast")
        want = optical_flow.fit_motion(r.forward, "similarity", state=r.occ_forward)
        assert np.array_equal(bits(motions[k]), bits(want.matrix)), k
    kept = [mn.keep(m)[0] for m in motions]
    for t in range(3):
        S = mn.smooth(kept, t, 3, 4, 3.0)
        assert np.array_equal(bits(out[t][1]), bits(S)), t
        want_o = optical_flow.warp_affine(frames[t], np.reshape(mn.inv(S), (2, 3)))
        assert out[t][0].shape == (32, 40, 3) and np.array_equal(out[t][0], want_o), t
    one = optical_flow.stabilize_frames(frames[:1], radius=2)
    assert np.array_equal(one[0], frames[0].astype(np.float32).astype(np.float64))


# ---- lifecycle ---------------------------------------------------------------
def test_lifecycle_and_device_bytes():
    import optical_flow
    from optical_flow import _abi, _native
    from test_gpu_fuse import clip_frames
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    frames = clip_frames(H, W, 1, 4, 8, 2.0)
    f0 = _native.f32(frames[0])
    out = np.empty((H, W), np.float32)
    idx, deg = C.c_int32(0), C.c_int32(0)

    def raw_push():
        return lib.of_stab_push(h, _native.ptr(f0), _native.ptr(out), None, None, None, C.byref(deg), C.byref(idx))

    def raw_flush():
        return lib.of_stab_flush(h, _native.ptr(out), None, None, C.byref(deg), C.byref(idx))

    for rc in (raw_push(), raw_flush(), lib.of_stab_close(h)):
        assert rc == _abi.OF_EINVAL
        with pytest.raises(ValueError, match="no stabiliser"):
            ctx.check(rc)

    base = optical_flow.stabilize_frames(frames, radius=2)  # also grows the arena to what these pairs need
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    watch = []
    with optical_flow.Stabilizer((H, W), radius=2) as st:
        watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        with pytest.raises(ValueError, match="stabiliser is open"):
            optical_flow.Stabilizer((H, W))  # one stabiliser per context
        got = {}
        # a tracker and a denoiser beside it
        with optical_flow.PointTracker((H, W), step=4, min_eig=1.0) as tr, \
                optical_flow.TemporalDenoiser((H, W), sigma=8.0) as dn:
            both = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
            for f in frames:
                r = st.push(f)
                tr.push(f)
                dn.push(f)
                if r:
                    got[r[0]] = r[1]
                watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        got.update(dict(st.flush()))
        with pytest.raises(ValueError, match="flushed"):
            st.push(frames[0])
    # radius + 1 frames, counted from open to close
    assert watch[0] - b0 == 3 * H * W * 4, (b0, watch)
    assert both > watch[0] and all(w == both for w in watch[1:]), (both, watch)
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    for t in range(4):
        assert np.array_equal(got[t], base[t])
    assert lib.of_stab_close(h) == _abi.OF_EINVAL
    # refused while a pair stream is open on the context
    with optical_flow.PairStream(H, W, 1, "classic+nl-fast", lanes=1) as ps:
        with pytest.raises(ValueError, match="pair stream is open"):
            optical_flow.Stabilizer((H, W), context=ps._ctx)
    # the C entries check for themselves
    P = optical_flow.load_of_method("classic+nl-fast").to_params()
    z = _native.f32(np.zeros((2, H, W)))
    fit = _abi.OfMotionFit()

    def mopts(**kw):
        a = dict(model=2, iters=10, kappa=2.0, decay=0.5, c_min=0.5)
        a.update(kw)
        return _abi.OfMotionOpts(*[a[k] for k in ("model", "iters", "kappa", "decay", "c_min")])

    def sopts(fit_kw=None, **kw):
        a = dict(radius=2, sigma_t=3.0, alpha1=0.01, alpha2=0.5)
        a.update(kw)
        return _abi.OfStabOpts(mopts(**(fit_kw or {})), a["radius"], 0, a["sigma_t"], a["alpha1"], a["alpha2"])

    def fit_call(o, weight=None, HH=H, WW=W):
        return lib.of_fit_motion(h, _native.ptr(z), HH, WW, _native.ptr(weight), None, C.byref(o), C.byref(fit), None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(model=-1), dict(model=3), dict(iters=-1), dict(iters=65), dict(kappa=0.0), dict(kappa=nan),
               dict(decay=0.0), dict(decay=1.5), dict(decay=nan), dict(c_min=0.0), dict(c_min=inf)):
        with pytest.raises(ValueError):
            ctx.check(fit_call(mopts(**kw)))
        with pytest.raises(ValueError):
            ctx.check(lib.of_stab_open(h, C.byref(P), H, W, 1, C.byref(sopts(kw))))
    for kw in (dict(radius=0), dict(radius=31), dict(sigma_t=0.0), dict(sigma_t=nan), dict(alpha1=-1.0),
               dict(alpha2=nan)):
        with pytest.raises(ValueError):
            ctx.check(lib.of_stab_open(h, C.byref(P), H, W, 1, C.byref(sopts(**kw))))
    with pytest.raises(ValueError):
        ctx.check(lib.of_stab_open(h, C.byref(P), H, W, 2, C.byref(sopts())))
    for bad in (-1.0, nan, inf):
        w = np.ones((H, W), np.float32)
        w[3, 4] = bad
        with pytest.raises(ValueError, match="weight"):
            ctx.check(fit_call(mopts(), w))
    A = np.array(mn.I6)
    for Cc in (0, 5):
        with pytest.raises(ValueError):
            ctx.check(lib.of_warp_affine(h, _native.ptr(f0), H, W, Cc, _native.dptr(A), _native.ptr(out), None))
    with pytest.raises(NotImplementedError):
        ctx.check(fit_call(mopts(), HH=46341, WW=46341))
    with pytest.raises(NotImplementedError):
        ctx.check(lib.of_warp_affine(h, _native.ptr(f0), 46341, 46341, 1, _native.dptr(A), _native.ptr(out), None))
    ctx.check(fit_call(mopts()))  # and the good call goes through: a zero flow is the identity
    assert list(fit.matrix) == list(mn.I6) and fit.degenerate == 0 and fit.support == H * W
    assert lib.of_stab_close(h) == _abi.OF_EINVAL  # none of the refused opens left a session behind


def test_destroying_a_context_closes_its_open_sessions():
    """of_ctx_destroy frees the sessions still open on the context; the Python
    objects' later close() is then a silent no-op, and a fresh context gives
    the same outputs bitwise."""
    import optical_flow
    from optical_flow import _native
    from test_gpu_fuse import clip_frames
    H, W = 32, 40
    frames = clip_frames(H, W, 1, 4, 8, 2.0)

    def run():
        ctx = _native.Context()
        tr = optical_flow.PointTracker((H, W), step=4, min_eig=1.0, context=ctx)
        dn = optical_flow.TemporalDenoiser((H, W), sigma=8.0, context=ctx)
        st = optical_flow.Stabilizer((H, W), radius=1, context=ctx)
        outs = []
        for f in frames:
            snap, d, s = tr.push(f), dn.push(f), st.push(f)
            outs += [snap.xy, snap.status, snap.start]
            outs += [r[1] for r in (d, s) if r is not None]
        ctx.close()  # with the three still open
        for session in (tr, dn, st):
            session.close()
        return outs

    first, second = run(), run()
    assert len(first) == len(second) == 3 * 4 + 2 * 3
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- end to end ----------------------------------------------------------------
def jitter_clip():
    """Nine 64 x 96 views of one seeded smooth texture whose content sits at
    the integer positions c_k: a slow drift of (1.5, 0.5) px per frame plus a
    jitter of up to +-2 px.  Returns (frames, c (9, 2) as (x, y))."""
    H, W, n = 64, 96, 9
    rng = np.random.default_rng(2025)
    tex = np.kron(rng.uniform(0, 255, (H // 4 + 16, W // 4 + 16)), np.ones((4, 4)))
    for _ in range(3):  # smooth the blocks a little
        tex = (tex + np.roll(tex, 1, 0) + np.roll(tex, 1, 1) + np.roll(tex, (1, 1), (0, 1))) / 4.0
    c = np.round(np.outer(np.arange(n), (1.5, 0.5))).astype(int) + rng.integers(-2, 3, (n, 2))
    # content at +c means the window sits at -c
    frames = [tex[32 - c[k, 1]:32 - c[k, 1] + H, 32 - c[k, 0]:32 - c[k, 0] + W].copy() for k in range(n)]
    return frames, c.astype(np.float64)


def smoothed_path(c, radius, sigma_t):
    """sum g_d c_{t+d} / sum g_d over the offsets inside the clip."""
    n = len(c)
    out = np.empty_like(c)
    for t in range(n):
        ds = [d for d in range(-radius, radius + 1) if 0 <= t + d <= n - 1]
        g = np.array([math.exp(-(d * d) / (2 * sigma_t * sigma_t)) for d in ds])
        out[t] = (g[:, None] * c[[t + d for d in ds]]).sum(0) / g.sum()
    return out


E_GATE = 0.0122  # px: twice the 0.0061 of the first run of this test on the GPU


def test_end_to_end_on_a_jittering_clip():
    """Similarity model, radius 3, sigma_t 3.  e = max_k |translation(M_k) -
    (c_{k+1} - c_k)| is the flow's own accuracy on this clip; its gate is twice
    the first GPU run's value, for other seeds.  Measured: e = 0.0061 px,
    max |translation(S_t) - smoothed path| = 0.0033 px (bound 3 e = 0.0183), mean
    |second difference| of the content position 2.286 -> 0.234 px."""
    import optical_flow
    frames, c = jitter_clip()
    radius, sigma_t = 3, 3.0
    out, motions, order = run_session(frames, model="similarity", radius=radius, sigma_t=sigma_t)
    assert order == [-1, -1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1]
    tr = np.array([m[:, 2] for m in motions])
    e = float(np.abs(tr - np.diff(c, axis=0)).max())
    S_tr = np.array([out[t][1][:, 2] for t in range(9)])
    want = smoothed_path(c, radius, sigma_t) - c
    e_S = float(np.abs(S_tr - want).max())
    d2 = lambda p: float(np.abs(np.diff(p, 2, axis=0)).mean())  # noqa: E731
    shake_in, shake_out = d2(c), d2(c + S_tr)
    print(f"jittering clip: e = {e:.4f} px, max |translation(S_t) - smoothed path| = {e_S:.4f} px "
          f"(bound {radius * e + 1e-9:.4f}), mean |second difference| of the content position "
          f"{shake_in:.3f} -> {shake_out:.3f} px")
    assert all(o[3] == 0 for o in out.values())
    assert e <= E_GATE
    assert e_S <= radius * e + 1e-9
    assert shake_out < 0.5 * shake_in
