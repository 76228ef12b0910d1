"""Blind temporal consistency on the GPU: of_screened_solve and of_consist_step
bitwise against the numpy float64 restatement (tests/screen_numpy.py), the
session bitwise against consistency_step on the flows it used, its lifecycle,
the C entries' own checks and the quality gates of the CPU tests with
estimated flows."""
import ctypes as C

import numpy as np
import pytest

import screen_numpy as sn
from test_gpu_inpaint import plant
from test_screen_cpu import SIGMA, quality_gates

pytestmark = pytest.mark.gpu

# odd sizes, level seams (30 x 30 is the largest single-level frame) and tile seams (32-cell tiles, two tiles across)
SHAPES = [(1, 1), (1, 7), (9, 1), (2, 2), (37, 53), (48, 65), (40, 129)]
ENDS = (dict(cycles=1, sweeps=1, coarse_sweeps=1), dict(cycles=64), dict(sweeps=1, coarse_sweeps=64),
        dict(cycles=2, sweeps=2, coarse_sweeps=7))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def chan(a):
    return a[None] if a.ndim == 2 else np.moveaxis(a, 2, 0)


def back(a, ndim):
    return a[0] if ndim == 2 else np.moveaxis(a, 0, 2)


def weight_planes(H, W, rng):
    ii, jj = np.mgrid[0:H, 0:W]
    one = np.zeros((H, W))
    one[H // 2, W // 2] = 3.0
    return {"all zero": np.zeros((H, W)), "all 1e6": np.full((H, W), 1e6), "random in [0, 2]": rng.uniform(0, 2, (H, W)),
            "zero except one pixel": one, "checkerboard of 0 and 5": 5.0 * ((ii + jj) & 1)}


def check_solve(t, a, w, key, **opts):
    import optical_flow
    want = back(sn.solve(chan(t).astype(np.float64), chan(a), w, cycles=opts.get("cycles", sn.CYCLES),
                         sweeps=opts.get("sweeps", sn.SWEEPS), coarse=opts.get("coarse_sweeps", sn.COARSE)), t.ndim)
    got = optical_flow.screened_poisson(t, a, w, **opts)
    assert got.dtype == np.float64 and got.shape == t.shape, key
    assert np.isfinite(got).all(), key
    bad = np.argwhere(bits64(got) != bits64(want))
    assert bad.size == 0, (key, bad[:5], np.abs(got - want).max())
    return got


@pytest.mark.parametrize("H,W", SHAPES)
def test_screened_poisson_bitwise_vs_numpy(H, W):
    rng = np.random.default_rng(100 * H + W)
    for name, w in weight_planes(H, W, rng).items():
        for Cc in (1, 3, 4):
            shp = (H, W) if Cc == 1 else (H, W, Cc)
            t = rng.uniform(0, 255, shp).astype(np.float32)
            a = rng.uniform(0, 255, shp)
            got = check_solve(t, a, w, (name, Cc))
            if name == "all zero":
                assert np.array_equal(bits64(got), bits64(t.astype(np.float64))), Cc
            if name == "all 1e6":
                assert np.abs(got - a).max() < 1e-2, Cc


@pytest.mark.parametrize("H,W", [(2, 2), (37, 53), (40, 129)])
def test_screened_poisson_options_at_their_ends(H, W):
    import optical_flow
    rng = np.random.default_rng(H + W)
    t = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    a = rng.uniform(0, 255, (H, W, 3))
    w = weight_planes(H, W, rng)["random in [0, 2]"]
    for opts in ENDS:
        check_solve(t, a, w, opts, **opts)
    # 2 channels; float64 and integer inputs give what their float32 values give
    t2 = np.rint(rng.uniform(0, 255, (H, W, 2))).astype(np.float32)
    g = check_solve(t2, a[..., :2], w, "two channels")
    assert np.array_equal(bits64(g), bits64(optical_flow.screened_poisson(t2.astype(np.int32), a[..., :2], w)))


# ---- the consistency step ------------------------------------------------------
def smooth(rng, H, W, Cc):
    """A frame of smooth blocks on 0..255, (H, W) or (H, W, Cc) float32."""
    c = np.kron(rng.uniform(0, 255, (H // 4 + 2, W // 4 + 2, Cc)), np.ones((4, 4, 1)))
    for _ in range(3):
        c = (c + np.roll(c, 1, 0) + np.roll(c, 1, 1) + np.roll(c, (1, 1), (0, 1))) / 4.0
    c = c[:H, :W].astype(np.float32)
    return c[..., 0].copy() if Cc == 1 else c


def step_flows(H, W, rng):
    """name -> (flow, state or None)"""
    rand = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    return {"zero": (np.zeros((H, W, 2), np.float32), None),
            "sub-pixel translation": (np.broadcast_to(np.float32([0.6, -0.3]), (H, W, 2)).copy(), None),
            "random, some leaving the frame": (rand, None),
            "NaN and inf entries": (plant(0.25 * rand), None),
            "a state plane with 30 % set": (0.1 * rand, (rng.uniform(size=(H, W)) < 0.3).astype(np.uint8)
                                            * rng.integers(1, 3, (H, W)).astype(np.uint8))}


def check_step(v, pv, p, po, f, s, key, **kw):
    import optical_flow
    kw = dict(dict(sigma=8.0, patch=1), **kw)
    want, want_w = sn.step(v, pv, p, po, f, s, lam=kw.get("lam", sn.LAMBDA), sigma=kw["sigma"],
                           strength=kw.get("strength", 4.0), patch=kw["patch"], cycles=kw.get("cycles", sn.CYCLES),
                           sweeps=kw.get("sweeps", sn.SWEEPS), coarse=kw.get("coarse_sweeps", sn.COARSE))
    got, w = optical_flow.consistency_step(v, pv, p, po, f, s, return_weight=True, **kw)
    assert got.dtype == np.float64 and got.shape == p.shape and w.shape == v.shape[:2], key
    bad = np.argwhere(bits32(w) != bits32(want_w))
    assert bad.size == 0, (key, "weight", bad[:5])
    bad = np.argwhere(bits32(got) != bits32(want))
    assert bad.size == 0, (key, bad[:5], np.abs(got - want).max())
    fw = optical_flow.fuse_weights(v, [pv], [f], kw["sigma"], [s], kw.get("strength", 4.0), kw["patch"])[0]
    assert np.array_equal(bits32(w), bits32(fw)), key
    only = optical_flow.consistency_step(v, pv, p, po, f, s, **kw)
    assert isinstance(only, np.ndarray) and np.array_equal(only, got), key
    return got, w


@pytest.mark.parametrize("Cc,Cp", [(1, 1), (3, 3), (1, 3)])
@pytest.mark.parametrize("H,W", [s for s in SHAPES if min(s) >= 2])
def test_consistency_step_bitwise_vs_numpy(H, W, Cc, Cp):
    rng = np.random.default_rng(1000 * H + W + 7 * Cc + Cp)
    seen = set()
    for name, (f, s) in step_flows(H, W, rng).items():
        v = smooth(rng, H, W, Cc)
        pv = (v + rng.normal(0, 6.0, v.shape)).astype(np.float32)
        p = smooth(rng, H, W, Cp)
        po = (0.9 * p + 9.0 + rng.normal(0, 2.0, p.shape)).astype(np.float32)
        got, w = check_step(v, pv, p, po, f, s, (name, "defaults"))
        seen |= {"zero weight"} if (w == 0).any() else set()
        seen |= {"full weight"} if (w == 1).any() else set()
        seen |= {"partial weight"} if ((w > 0) & (w < 1)).any() else set()
        off, _ = check_step(v, pv, p, po, f, s, (name, "lam 0"), lam=0.0)
        assert np.array_equal(bits32(off), bits32(p)), name  # the processed frame to the bit
        check_step(v, pv, p, po, f, s, (name, "other options"), lam=7.5, sigma=3.0, strength=2.0, patch=(0, 2, 3)[Cp % 3],
                   cycles=2, sweeps=1, coarse_sweeps=5)
    if H * W > 1000:
        assert seen == {"zero weight", "full weight", "partial weight"}


# ---- the C entries check for themselves -----------------------------------------
def test_the_c_entries_check_for_themselves():
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, hd = ctx.lib, ctx.handle
    H, W = 8, 9
    t = _native.f32(np.ones((H, W)))
    a = np.full((H, W), 2.0)
    w = np.ones((H, W))
    out = np.empty((H, W), np.float64)
    ok = _abi.OfBlendOpts(5, 2, 32, 0)

    def solve(o=ok, t=t, a=a, w=w, HH=H, WW=W, Cc=1, dst=out):
        return lib.of_screened_solve(hd, _native.ptr(t), _native.dptr(a), _native.dptr(w), HH, WW, Cc,
                                     C.byref(o) if o is not None else None, _native.dptr(dst))

    for bad in ((0, 2, 32), (65, 2, 32), (5, 0, 32), (5, 3, 32), (5, 2, 0), (5, 2, 65)):
        with pytest.raises(ValueError):
            ctx.check(solve(_abi.OfBlendOpts(*bad, 0)))
    neg, nan, inf = w.copy(), w.copy(), w.copy()
    neg[3, 4], nan[0, 0], inf[7, 8] = -1e-9, np.nan, np.inf
    for kw in (dict(o=None), dict(t=None), dict(a=None), dict(w=None), dict(dst=None), dict(Cc=0), dict(Cc=5), dict(HH=0),
               dict(WW=-1), dict(w=neg), dict(w=nan), dict(w=inf)):
        with pytest.raises(ValueError):
            ctx.check(solve(**kw))
    with pytest.raises(NotImplementedError):
        ctx.check(solve(HH=46341, WW=46341))
    ctx.check(solve())
    assert np.abs(out - 2.0).max() < 1e-6  # a flat target: q (x - 2) = 0 everywhere

    z = _native.f32(np.zeros((2, H, W)))
    o32 = np.empty((H, W), np.float32)

    def opts(patch=1, sigma=2.0, strength=4.0, a1=0.01, a2=0.5, solve=(5, 2, 32), lam=1.0, radius=0):
        return _abi.OfConsistOpts(_abi.OfFuseOpts(radius, patch, sigma, strength, a1, a2), _abi.OfBlendOpts(*solve, 0), lam)

    def step(o=opts(), v=t, pv=t, p=t, po=t, f=z, Cc=1, Cp=1, HH=H, dst=o32):
        return lib.of_consist_step(hd, _native.ptr(v), _native.ptr(pv), HH, W, Cc, _native.ptr(p), _native.ptr(po), Cp,
                                   _native.ptr(f), None, C.byref(o) if o is not None else None, _native.ptr(dst), None)

    BAD = (dict(patch=-1), dict(patch=4), dict(sigma=0.0), dict(sigma=np.nan), dict(strength=0.0), dict(strength=np.inf),
           dict(a1=-1.0), dict(a2=np.nan), dict(solve=(0, 2, 32)), dict(solve=(5, 3, 32)), dict(solve=(5, 2, 65)),
           dict(lam=-1e-9), dict(lam=np.nan), dict(lam=np.inf))
    for kw in BAD:
        with pytest.raises(ValueError):
            ctx.check(step(opts(**kw)))
    for kw in (dict(o=None), dict(v=None), dict(pv=None), dict(p=None), dict(po=None), dict(f=None), dict(dst=None),
               dict(Cc=0), dict(Cc=5), dict(Cp=0), dict(Cp=5), dict(HH=0)):
        with pytest.raises(ValueError):
            ctx.check(step(**kw))
    o32[:] = -1.0
    ctx.check(step(opts(radius=99)))  # radius is not read
    assert (o32 == 1.0).all()
    # the open checks the same struct, the channel counts and the params
    from optical_flow._session import method_params
    P = method_params("classic+nl-fast", None)[1]
    for kw in BAD:
        o = opts(**kw)
        assert lib.of_consist_open(hd, C.byref(P), H, W, 1, 1, C.byref(o)) == _abi.OF_EINVAL, kw
    good = opts()
    for args in ((H, W, 2, 1), (H, W, 1, 0), (H, W, 1, 5), (0, W, 1, 1)):
        assert lib.of_consist_open(hd, C.byref(P), *args, C.byref(good)) == _abi.OF_EINVAL, args
    assert lib.of_consist_open(hd, None, H, W, 1, 1, C.byref(good)) == _abi.OF_EINVAL
    assert lib.of_consist_open(hd, C.byref(P), H, W, 1, 1, None) == _abi.OF_EINVAL
    assert lib.of_consist_close(hd) == _abi.OF_EINVAL  # none of them opened a session


# ---- the session ----------------------------------------------------------------
@pytest.mark.parametrize("Cc,Cp", [(1, 1), (3, 3), (1, 3)])
def test_session_is_consistency_step_on_its_flows_and_lifecycle(Cc, Cp):
    import optical_flow
    from optical_flow import _abi, _native
    from test_gpu_inpaint import clip_frames
    H, W, T = 48, 64, 4
    frames, _ = clip_frames(H, W, Cc, T, 90 + Cc)
    rng = np.random.default_rng(Cp)
    proc = [smooth(rng, H, W, Cp) * np.float32(1.0 + 0.05 * (-1) ** k) + np.float32(3 * k) for k in range(T)]
    kw = dict(sigma=4.0, lam=1.5, patch=2)
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    pairs = [optical_flow.estimate_flow_bidirectional(frames[k - 1], frames[k], "classic+nl-fast", alpha1=0.02,
                                                      alpha2=0.4) for k in range(1, T)]  # also grows the arena
    want = [proc[0].astype(np.float64)]
    want_w = [np.zeros((H, W))]
    for k in range(1, T):
        o, w = optical_flow.consistency_step(frames[k], frames[k - 1], proc[k], want[-1], pairs[k - 1].backward,
                                             pairs[k - 1].occ_backward, return_weight=True, **kw)
        want.append(o)
        want_w.append(w)
    optical_flow.consistent_frames(frames[:2], proc[:2], alpha1=0.02, alpha2=0.4, **kw)  # the arena at its final size
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    got, got_w = optical_flow.consistent_frames(frames, proc, "classic+nl-fast", alpha1=0.02, alpha2=0.4,
                                                return_weight=True, **kw)
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    assert got.shape == (T,) + proc[0].shape and got.dtype == np.float64 and got_w.shape == (T, H, W)
    assert np.array_equal(bits32(got[0]), bits32(proc[0]))  # push 0: the processed frame to the bit
    for k in range(T):
        assert np.array_equal(bits64(got[k]), bits64(want[k])), (k, np.abs(got[k] - want[k]).max())
        assert np.array_equal(bits64(got_w[k]), bits64(want_w[k])), k
    assert (got_w[1:] > 0).mean() > 0.5  # the flows were good for something

    shape = (H, W) if Cc == 1 else (H, W, 3)
    f32 = _native.f32(frames[0])
    p32 = _native.f32(proc[0])
    o32 = np.empty(proc[0].shape, np.float32)

    def raw_push(f=f32, p=p32, o=o32):
        return lib.of_consist_push(h, _native.ptr(f), _native.ptr(p), _native.ptr(o), None)

    assert raw_push() == _abi.OF_EINVAL and lib.of_consist_close(h) == _abi.OF_EINVAL  # no session is open
    with optical_flow.TemporalConsistency(shape, Cp, alpha1=0.02, alpha2=0.4, **kw) as tc:
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) - b0 == 2 * H * W * Cc * 4 + H * W * Cp * 4
        assert tc.processed_shape == proc[0].shape and tc.lam == 1.5 and tc.sigma == 4.0
        with pytest.raises(ValueError, match="is open"):
            optical_flow.TemporalConsistency(shape, Cp, sigma=4.0)  # one per context
        for bad in (np.zeros((H, W + 1)), np.zeros((H, W, 2)), np.full(shape, np.nan)):
            with pytest.raises(ValueError):
                tc.push(bad, proc[0])
        for bad in (np.zeros((H + 1, W)), np.zeros((H, W, 5)), np.full(proc[0].shape, np.inf)):
            with pytest.raises(ValueError):
                tc.push(frames[0], bad)
        assert tc.frames == 0
        assert raw_push(f=None) == _abi.OF_EINVAL and raw_push(p=None) == _abi.OF_EINVAL
        assert raw_push(o=None) == _abi.OF_EINVAL
        up = _abi.OfUpsampleOpts(2, 0, 20.0)
        for kinds in (8, 16, 64):  # not a kind the flow scale takes
            assert lib.of_session_set_flow_scale(h, kinds, C.byref(up)) == _abi.OF_EINVAL
        for k in range(2):
            o = tc.push(frames[k], proc[k])
            assert np.array_equal(bits64(o), bits64(want[k])), k
            assert np.array_equal(bits64(tc.last_weight), bits64(want_w[k])), k
        assert tc.frames == 2
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    with pytest.raises(ValueError, match="is closed"):
        tc.push(frames[0], proc[0])
    assert raw_push() == _abi.OF_EINVAL and lib.of_consist_close(h) == _abi.OF_EINVAL
    # processed_channels None: as the frames; a destroyed context frees its open session
    c2 = _native.Context()
    tc2 = optical_flow.TemporalConsistency(shape, sigma=4.0, context=c2)
    assert tc2.processed_shape == shape
    assert c2.get_option(_abi.OF_OPT_DEVICE_BYTES) >= 3 * H * W * Cc * 4
    c2.close()
    tc2.close()


# ---- quality with estimated flows ---------------------------------------------
def test_scene_quality_with_estimated_flows():
    """The gates of the issue on inpaint_numpy.scene(0), the flows estimated by
    the session ('classic+nl-fast'), sigma 0.7 (what the scene's frames differ
    by, test_screen_cpu.py), lambda 1; the measures along the true flows over
    the truly visible pixels.  The prototype along the known flows: instability
    81.94 of the processed clip (a) and 0.870 of its result (b), so the gate is
    sqrt(a b) = 8.44; fidelity 0.537, gate 1.07; a processed clip equal to the
    frames comes back with an MSE of 2.50, gate 5.00."""
    import optical_flow
    frames, bw, vis = sn.scene_truth()
    proc = sn.flicker_clip(frames)
    states = [(~v).astype(np.uint8) for v in vis]
    known = (frames, bw, vis, states, proc, sn.clip(frames, proc, bw, states, sigma=SIGMA),
             sn.clip(frames, frames, bw, states, sigma=SIGMA))
    outs = optical_flow.consistent_frames(frames, proc, sigma=SIGMA)
    same = optical_flow.consistent_frames(frames, frames, sigma=SIGMA)
    assert outs.shape == (9, 48, 64) and np.isfinite(outs).all()
    a, b, fid, mse = quality_gates(known, list(outs), list(same), "estimated flows")
    assert abs(a - 81.94) < 0.01 and abs(b - 0.870) < 0.001 and abs(fid - 0.537) < 0.001 and abs(mse - 2.50) < 0.01
