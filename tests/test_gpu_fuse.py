"""Temporal denoising on the GPU: of_flow_compose and of_fuse_frames bitwise
against the numpy float64 restatement (tests/fuse_numpy.py), the session
(of_denoise_*) bitwise against its parts run by hand, its lifecycle, the
two-layer occlusion scene and an end-to-end run on a noisy translating clip."""
import ctypes as C

import numpy as np
import pytest

import fuse_numpy as fn

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 1), (3, 130), (37, 53), (64, 65)]
SIGMA = 25.0  # uniform 0..255 frames differ by ~104 rms: 2 s^2 + (4 s)^2 = 11250 straddles 2 * 104^2


def plant(flow):
    """The interpolation test's planted cases in an (H, W, 2) float32 flow."""
    H, W = flow.shape[:2]
    n = H * W
    pix = lambda k: divmod(k, W)  # noqa: E731
    flow[pix(n - 1)] = (-0.0, -0.0)
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
    return flow


def fuse_case(H, W, Cc, n):
    """Seeded random frames, flows in +-6 px (the last neighbour's a tenth of
    that) with the planted cases, and states holding 0, 1 and 2."""
    rng = np.random.default_rng(1000 * H + W + 7 * Cc + 31 * n)
    shp = (H, W) if Cc == 1 else (H, W, Cc)
    center = rng.uniform(0, 255, shp).astype(np.float32)
    neigh = [rng.uniform(0, 255, shp).astype(np.float32) for _ in range(n)]
    flows = [rng.uniform(-6, 6, (H, W, 2)).astype(np.float32) for _ in range(n)]
    flows[0] = plant(flows[0])
    if n > 1:
        flows[n - 1] = plant(flows[n - 1] * np.float32(0.1))  # short flows: most pixels stay inside
    states = [rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W)) for _ in range(n)]
    return center, neigh, flows, states


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_fuse_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    seen = set()
    for n in (1, 4):
        center, neigh, flows, states = fuse_case(H, W, Cc, n)
        for patch in (0, 2, 3):
            for st in (states, None):
                want, want_w = fn.fuse(center, neigh, flows, SIGMA, st, 4.0, patch)
                out, wgt = optical_flow.fuse_frames(center, neigh, flows, SIGMA, st, 4.0, patch, return_weight=True)
                assert out.dtype == np.float64 and out.shape == center.shape
                assert wgt.dtype == np.float64 and wgt.shape == (H, W)
                key = (n, patch, st is None)
                bad = np.argwhere(wgt.astype(np.float32).view(np.uint32) != want_w.view(np.uint32))
                assert bad.size == 0, (key, bad[:5])
                bad = np.argwhere(out.astype(np.float32).view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, (key, bad[:5])
                only = optical_flow.fuse_frames(center, neigh, flows, SIGMA, st, 4.0, patch)
                assert only.dtype == np.float64 and np.array_equal(only, out)
                for vis, _, w in fn.weights(center, neigh, flows, SIGMA, st, 4.0, patch):
                    seen |= {"hidden"} if (~vis).any() else set()
                    seen |= {"zero"} if (w[vis] == 0).any() else set()
                    seen |= {"part"} if ((w > 0) & (w < 1)).any() else set()
                    seen |= {"one"} if (w == 1).any() else set()
    if H * W > 1000:
        assert seen == {"hidden", "zero", "part", "one"}, seen  # every branch of the weight occurs


def test_fuse_other_strength_and_two_channels():
    import optical_flow
    center, neigh, flows, states = fuse_case(37, 53, 2, 8)
    want, want_w = fn.fuse(center, neigh, flows, 40.0, states, 1.5, 1)
    out, wgt = optical_flow.fuse_frames(center, neigh, flows, 40.0, states, 1.5, 1, return_weight=True)
    np.testing.assert_array_equal(out.astype(np.float32).view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(wgt.astype(np.float32).view(np.uint32), want_w.view(np.uint32))
    assert wgt.min() >= 1.0 and wgt.max() <= 9.0 and wgt.max() > 2.0


@pytest.mark.parametrize("H,W", SHAPES)
def test_compose_bitwise_vs_numpy(H, W):
    import optical_flow
    rng = np.random.default_rng(77 * H + W)
    f = plant(rng.uniform(-6, 6, (H, W, 2)).astype(np.float32))
    g = plant(rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)[::-1, ::-1].copy())
    sf = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    sg = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    for a, b in ((sf, sg), (None, None), (sf, None), (None, sg)):
        want, want_s = fn.compose(f, g, a, b)
        out, st = optical_flow.compose_flows(f, g, a, b, return_state=True)
        assert out.dtype == np.float64 and out.shape == (H, W, 2) and st.dtype == np.uint8 and st.shape == (H, W)
        np.testing.assert_array_equal(st, want_s)
        np.testing.assert_array_equal(out.astype(np.float32).view(np.uint32), want.view(np.uint32))
        only = optical_flow.compose_flows(f, g, a, b)
        np.testing.assert_array_equal(only.astype(np.float32).view(np.uint32), want.view(np.uint32))
    if H * W > 1000:
        assert set(np.unique(fn.compose(f, g, sf, sg)[1])) == {0, 1, 2}
    # a zero g returns f, with state 2 exactly where f leaves the frame
    # (as values: -0.0 + 0.0 is +0.0; NaN and Inf components come back as they are)
    out, st = optical_flow.compose_flows(f, np.zeros((H, W, 2)), return_state=True)
    np.testing.assert_array_equal(out.astype(np.float32), f)
    ii, jj = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        r, q = ii + f[..., 1].astype(np.float64), jj + f[..., 0].astype(np.float64)
        leaves = ~(np.isfinite(f).all(-1) & (q >= 0) & (q <= W - 1) & (r >= 0) & (r <= H - 1))
    np.testing.assert_array_equal(st, np.where(leaves, 2, 0))


# ---- the session equals its parts ------------------------------------------
def clip_frames(H, W, Cc, n, seed, noise):
    """n noisy frames: windows of one smooth random canvas, moving by (2, 1) px
    per frame."""
    rng = np.random.default_rng(seed)
    c = np.kron(rng.uniform(0, 255, (H // 4 + 8, W // 4 + 8, Cc)), np.ones((4, 4, 1)))
    for _ in range(3):  # smooth the blocks a little
        c = (c + np.roll(c, 1, 0) + np.roll(c, 1, 1) + np.roll(c, (1, 1), (0, 1))) / 4.0
    x0 = 2 * n + 2
    fr = [c[4 + k:4 + k + H, x0 - 2 * k:x0 - 2 * k + W] + rng.normal(0, noise, (H, W, Cc)) for k in range(n)]
    return [f[..., 0].copy() if Cc == 1 else f.copy() for f in fr]


@pytest.fixture(scope="module")
def clips():
    """Per channel count: a 6-frame 48 x 64 clip and (fw, bw, sf, sb) of every
    adjacent pair from estimate_flow_bidirectional, computed once."""
    import optical_flow
    out = {}
    for Cc in (1, 3):
        frames = clip_frames(48, 64, Cc, 6, 40 + Cc, 6.0)
        pairs = []
        for a, b in zip(frames[:-1], frames[1:]):
            r = optical_flow.estimate_flow_bidirectional(a, b, "classic+nl-fast")
            pairs.append((r.forward, r.backward, r.occ_forward, r.occ_backward))
        out[Cc] = (frames, pairs)
    return out


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("Cc", [1, 3])
def test_session_equals_its_parts(clips, Cc, radius):
    import optical_flow
    frames, pairs = clips[Cc]
    sigma = 6.0
    want = fn.session(
        frames, pairs, sigma, radius, 4.0, 2,
        compose_fn=lambda f, g, a, b: optical_flow.compose_flows(f, g, a, b, return_state=True),
        fuse_fn=lambda c, nb, fl, s, st, strength, patch: optical_flow.fuse_frames(c, nb, fl, s, st, strength, patch,
                                                                                   return_weight=True))
    got = []
    with optical_flow.TemporalDenoiser(frames[0].shape, "classic+nl-fast", sigma=sigma, radius=radius) as dn:
        for k, f in enumerate(frames):
            r = dn.push(f)
            if k < radius:
                assert r is None
            else:
                assert r is not None and r[0] == k - radius
                got.append((r[0], r[1], dn.last_weight))
        for r in dn.flush():
            got.append((r[0], r[1], dn.last_weight))
        assert list(dn.flush()) == []
    assert [g[0] for g in got] == list(range(6))
    for t, o, w in got:
        assert o.dtype == np.float64 and o.shape == frames[0].shape and w.shape == (48, 64)
        assert np.array_equal(o, want[t][0]), (t, np.abs(o - want[t][0]).max())
        assert np.array_equal(w, want[t][1]), t
    all_o, all_w = optical_flow.denoise_frames(frames, "classic+nl-fast", sigma=sigma, radius=radius,
                                               return_weight=True)
    assert all_o.shape == (6,) + frames[0].shape and all_o.dtype == np.float64 and all_w.shape == (6, 48, 64)
    for t in range(6):
        assert np.array_equal(all_o[t], want[t][0]) and np.array_equal(all_w[t], want[t][1]), t
    assert np.array_equal(optical_flow.denoise_frames(frames, "classic+nl-fast", sigma=sigma, radius=radius), all_o)
    # it did fuse: interior frames average more than the clip's ends, and more at radius 2
    means = [float(w.mean()) for _, _, w in got]
    print(f"C={Cc} radius={radius}: mean effective frames per output {np.round(means, 3)}")
    assert means[2] > means[0] > 1.0 and max(means) <= 2 * radius + 1


def test_single_frame_clip_comes_back_unchanged():
    import optical_flow
    f = np.random.default_rng(3).uniform(0, 255, (20, 30, 3))
    out, wgt = optical_flow.denoise_frames([f], sigma=5.0, radius=2, return_weight=True)
    assert np.array_equal(out[0], f.astype(np.float32).astype(np.float64)) and np.all(wgt == 1.0)


# ---- lifecycle ---------------------------------------------------------------
def test_lifecycle_and_device_bytes():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    frames = clip_frames(H, W, 1, 3, 8, 4.0)
    f0 = _native.f32(frames[0])
    out = np.empty((H, W), np.float32)
    idx = C.c_int32(0)

    def raw_push():
        return lib.of_denoise_push(h, _native.ptr(f0), _native.ptr(out), None, C.byref(idx))

    def raw_flush():
        return lib.of_denoise_flush(h, _native.ptr(out), None, C.byref(idx))

    for rc in (raw_push(), raw_flush(), lib.of_denoise_close(h)):
        assert rc == _abi.OF_EINVAL
        with pytest.raises(ValueError, match="no temporal denoiser"):
            ctx.check(rc)

    base = optical_flow.denoise_frames(frames, sigma=8.0)  # also grows the arena to what these pairs need
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    watch = []
    with optical_flow.TemporalDenoiser((H, W), sigma=8.0) as dn:
        watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        with pytest.raises(ValueError, match="denoiser is open"):
            optical_flow.TemporalDenoiser((H, W), sigma=8.0)  # one denoiser per context
        got = {}
        with optical_flow.PointTracker((H, W), step=4, min_eig=1.0) as tr:  # a tracker beside it
            for f in frames:
                r = dn.push(f)
                tr.push(f)
                if r:
                    got[r[0]] = r[1]
                watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
            trk_bytes = watch[-1] - watch[0]
        got.update(dict(dn.flush()))
        with pytest.raises(ValueError, match="flushed"):
            dn.push(frames[0])
    # 3 frames and 2 pairs' flows and states, counted from open to close
    pitch = (W + 63) // 64 * 64
    assert watch[0] - b0 == 3 * H * W * 4 + 2 * (2 * H * pitch * 8 + 2 * H * W), (b0, watch)
    assert trk_bytes > 0 and all(w == watch[1] for w in watch[1:])
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    for t in range(3):
        assert np.array_equal(got[t], base[t])
    assert lib.of_denoise_close(h) == _abi.OF_EINVAL
    # refused while a pair stream is open on the context
    with optical_flow.PairStream(H, W, 1, "classic+nl-fast", lanes=1) as ps:
        with pytest.raises(ValueError, match="pair stream is open"):
            optical_flow.TemporalDenoiser((H, W), sigma=8.0, context=ps._ctx)
    # the C entries check for themselves
    P = optical_flow.load_of_method("classic+nl-fast").to_params()
    z = _native.f32(np.zeros((2, H, W)))

    def opts(**kw):
        a = dict(radius=1, patch=2, sigma=8.0, strength=4.0, alpha1=0.01, alpha2=0.5)
        a.update(kw)
        return _abi.OfFuseOpts(*[a[k] for k in ("radius", "patch", "sigma", "strength", "alpha1", "alpha2")])

    def fuse(o, Cc=1, n=1, HH=H, WW=W):
        return lib.of_fuse_frames(h, _native.ptr(f0), HH, WW, Cc, n, _native.ptr(f0), _native.ptr(z), None,
                                  C.byref(o), _native.ptr(out), None)

    for kw in (dict(radius=0), dict(radius=3), dict(patch=-1), dict(patch=4), dict(sigma=0.0),
               dict(sigma=float("nan")), dict(strength=float("inf")), dict(strength=0.0), dict(alpha1=-1.0),
               dict(alpha2=float("nan"))):
        with pytest.raises(ValueError):
            ctx.check(fuse(opts(**kw)))
        with pytest.raises(ValueError):
            ctx.check(lib.of_denoise_open(h, C.byref(P), H, W, 1, C.byref(opts(**kw))))
    for kw in (dict(Cc=0), dict(Cc=5), dict(n=0), dict(n=9)):
        with pytest.raises(ValueError):
            ctx.check(fuse(opts(), **kw))
    with pytest.raises(ValueError):
        ctx.check(lib.of_denoise_open(h, C.byref(P), H, W, 2, C.byref(opts())))
    with pytest.raises(NotImplementedError):
        ctx.check(fuse(opts(), HH=46341, WW=46341))
    with pytest.raises(NotImplementedError):
        ctx.check(lib.of_flow_compose(h, _native.ptr(z), _native.ptr(z), 46341, 46341, None, None, _native.ptr(z),
                                      None))
    ctx.check(fuse(opts()))  # and the good call goes through
    assert lib.of_denoise_close(h) == _abi.OF_EINVAL  # none of the refused opens left a session behind


# ---- the two-layer scene, noise-free ------------------------------------------
def test_two_layer_scene_noise_free():
    import optical_flow
    from test_gpu_interp import two_layer
    (im0, fg0), (im1, fg1), (im2, fg2) = two_layer(0.0), two_layer(1.0), two_layer(2.0)
    H, W = im1.shape
    to_prev, to_next = np.zeros((H, W, 2)), np.zeros((H, W, 2))
    to_prev[fg1, 0], to_next[fg1, 0] = -8.0, 8.0
    s_prev = (~fg1 & fg0).astype(np.uint8)  # background the foreground covers in the other frame
    s_next = (~fg1 & fg2).astype(np.uint8)
    c32 = im1.astype(np.float32).astype(np.float64)
    out, wgt = optical_flow.fuse_frames(im1, [im0, im2], [to_prev, to_next], 2.0, [s_prev, s_next],
                                        return_weight=True)
    err = np.abs(out - c32).max()
    plain, wgt0 = optical_flow.fuse_frames(im1, [im0, im2], [to_prev, to_next], 2.0, None, return_weight=True)
    err0 = np.abs(plain - c32).max()
    print(f"two-layer scene: max |fused - centre| with masks {err:.3e} (mean weight {wgt.mean():.3f}), "
          f"without {err0:.3e} (mean weight {wgt0.mean():.3f})")
    assert err <= 1e-4
    assert err0 >= err
    assert np.all(wgt[(s_prev == 0) & (s_next == 0)] == 3.0)  # seen in all three frames: the plain mean
    assert np.all(wgt[(s_prev == 1) & (s_next == 0)] == 2.0) and np.all(wgt[(s_prev == 0) & (s_next == 1)] == 2.0)
    want, want_w = fn.fuse(im1, [im0, im2], [to_prev, to_next], 2.0, [s_prev, s_next])
    assert np.array_equal(out.astype(np.float32), want) and np.array_equal(wgt.astype(np.float32), want_w)


# ---- end to end ----------------------------------------------------------------
def test_end_to_end_on_a_noisy_translating_clip():
    """Five 48 x 64 frames of the interpolation test's texture moving (4, -2)
    px per frame, Gaussian noise sigma = 10; the middle frame, 8 px border
    left out.  Measured MSE against the clean frame: noisy 96.35,
    uncompensated 3-frame mean 578.49, denoise_frames 25.52, fuse_frames along
    the analytic flow 31.52 (ideal sigma^2 / 3 = 33.33).  The gates are the
    first two only: the estimator had not been run on these frames before."""
    import optical_flow
    from test_gpu_interp import tex
    H, W, sigma = 48, 64, 10.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    clean = [tex(1, yy + 2.0 * t, xx - 4.0 * t) for t in range(5)]
    rng = np.random.default_rng(99)
    noisy = [c + rng.normal(0, sigma, c.shape) for c in clean]
    out = optical_flow.denoise_frames(noisy, "classic+nl-fast", sigma=sigma, radius=1)
    m = (slice(8, H - 8), slice(8, W - 8))
    mse = lambda a: float(((a - clean[2]) ** 2)[m].mean())  # noqa: E731
    to_prev, to_next = np.zeros((H, W, 2)), np.zeros((H, W, 2))
    to_prev[...], to_next[...] = (-4.0, 2.0), (4.0, -2.0)
    along = optical_flow.fuse_frames(noisy[2], [noisy[1], noisy[3]], [to_prev, to_next], sigma)
    e_out, e_in, e_mean, e_true = mse(out[2]), mse(noisy[2]), mse(np.mean(noisy[1:4], 0)), mse(along)
    print(f"48x64 translating clip, sigma 10, interior MSE: noisy {e_in:.2f}, uncompensated 3-frame mean "
          f"{e_mean:.2f}, denoise_frames {e_out:.2f}, fuse_frames along the analytic flow {e_true:.2f} "
          f"(ideal sigma^2 / 3 = {sigma ** 2 / 3:.2f})")
    assert out.shape == (5, H, W)
    assert e_out < e_in
    assert e_out < e_mean
