"""Multi-frame super-resolution on the GPU: of_fuse_weights and
of_super_resolve bitwise against the numpy float64 restatements
(tests/fuse_numpy.py, tests/sr_numpy.py), the session (of_sr_*) bitwise against
its parts run by hand, its lifecycle, and an end-to-end run on the prototype
scene with estimated flows."""
import ctypes as C

import numpy as np
import pytest

import fuse_numpy as fn
import sr_numpy as sn
from test_gpu_fuse import SHAPES, SIGMA, clip_frames, fuse_case

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_weights_and_super_resolve_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    seen, grew = set(), False
    for n in (0, 1, 4):
        center, neigh, flows, states = fuse_case(H, W, Cc, max(n, 1))
        if n == 0:
            neigh, flows, states = [], [], []
        wk = None
        if n:
            wk = [w.astype(np.float32) for _, _, w in fn.weights(center, neigh, flows, SIGMA, states, 4.0, 2)]
            got = optical_flow.fuse_weights(center, neigh, flows, SIGMA, states, 4.0, 2)
            assert got.dtype == np.float64 and got.shape == (n, H, W)
            bad = np.argwhere(bits(got) != bits(np.stack(wk)))
            assert bad.size == 0, (n, bad[:5])
        for s in (2, 3, 4):
            alone = sn.super_resolve(center, [], [], s, SIGMA)[1] if n else None
            for reach in (0.75, 1.5):
                for back in (0.0, 0.5):
                    key = (n, s, reach, back)
                    want, want_s = sn.super_resolve(center, neigh, flows, s, SIGMA, states, 4.0, 2, reach, back,
                                                    weights=wk, seen=seen)
                    out, sup = optical_flow.super_resolve(center, neigh, flows, s, SIGMA, states, 4.0, 2, reach,
                                                          back, return_support=True)
                    assert out.dtype == np.float64 and out.shape == (s * H, s * W) + center.shape[2:], key
                    assert sup.dtype == np.float64 and sup.shape == (s * H, s * W), key
                    bad = np.argwhere(bits(sup) != bits(want_s))
                    assert bad.size == 0, (key, bad[:5])
                    bad = np.argwhere(bits(out) != bits(want))
                    assert bad.size == 0, (key, bad[:5])
                    assert np.all(sup > 0)
                    if n and reach == 0.75:
                        grew |= bool((want_s > alone).any())
            only = optical_flow.super_resolve(center, neigh, flows, s, SIGMA, states)
            assert np.array_equal(only, optical_flow.super_resolve(center, neigh, flows, s, SIGMA, states,
                                                                   return_support=True)[0])
    if H * W > 1000:  # every branch occurred, and the neighbours added support somewhere
        assert seen == {"zero", "left", "far", "edge"}, seen
        assert grew


def test_other_options_and_two_channels():
    import optical_flow
    center, neigh, flows, states = fuse_case(37, 53, 2, 8)
    for st in (states, None):
        want, want_s = sn.super_resolve(center, neigh, flows, 3, 40.0, st, 1.5, 1, 1.0, 1.0)
        out, sup = optical_flow.super_resolve(center, neigh, flows, 3, 40.0, st, 1.5, 1, 1.0, 1.0, return_support=True)
        np.testing.assert_array_equal(bits(out), bits(want))
        np.testing.assert_array_equal(bits(sup), bits(want_s))
        got = optical_flow.fuse_weights(center, neigh, flows, 40.0, st, 1.5, 1)
        wk = np.stack([w for _, _, w in fn.weights(center, neigh, flows, 40.0, st, 1.5, 1)])
        np.testing.assert_array_equal(bits(got), bits(wk))


# ---- the session equals its parts ------------------------------------------
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
    sigma = 9.0
    want = fn.session(
        frames, pairs, sigma, radius, 4.0, 2,
        compose_fn=lambda f, g, a, b: optical_flow.compose_flows(f, g, a, b, return_state=True),
        fuse_fn=lambda c, nb, fl, s, st, strength, patch: optical_flow.super_resolve(c, nb, fl, 2, s, st, strength,
                                                                                     patch, return_support=True))
    got = []
    with optical_flow.SuperResolver(frames[0].shape, "classic+nl-fast", factor=2, sigma=sigma, radius=radius) as sr:
        for k, f in enumerate(frames):
            r = sr.push(f)
            if k < radius:
                assert r is None
            else:
                assert r is not None and r[0] == k - radius
                got.append((r[0], r[1], sr.last_support))
        for r in sr.flush():
            got.append((r[0], r[1], sr.last_support))
        assert list(sr.flush()) == []
    assert [g[0] for g in got] == list(range(6))
    for t, o, w in got:
        assert o.dtype == np.float64 and o.shape == (96, 128) + frames[0].shape[2:] and w.shape == (96, 128)
        assert np.array_equal(o, want[t][0]), (t, np.abs(o - want[t][0]).max())
        assert np.array_equal(w, want[t][1]), t
    all_o, all_s = optical_flow.super_resolve_frames(frames, "classic+nl-fast", factor=2, sigma=sigma, radius=radius,
                                                     return_support=True)
    assert all_o.shape == (6, 96, 128) + frames[0].shape[2:] and all_o.dtype == np.float64
    assert all_s.shape == (6, 96, 128)
    for t in range(6):
        assert np.array_equal(all_o[t], want[t][0]) and np.array_equal(all_s[t], want[t][1]), t
    # the neighbours did count: interior frames rest on more than the clip's ends, which rest on more than one frame
    alone = optical_flow.super_resolve(frames[0], [], [], 2, sigma, return_support=True)[1].mean()
    means = [float(w.mean()) for _, _, w in got]
    print(f"C={Cc} radius={radius}: mean support per output {np.round(means, 3)}, single frame {alone:.3f}")
    assert means[2] > means[0] > alone


def test_single_frame_clip_gives_the_single_frame_result():
    import optical_flow
    f = np.random.default_rng(3).uniform(0, 255, (20, 30, 3))
    out, sup = optical_flow.super_resolve_frames([f], factor=3, sigma=5.0, radius=2, return_support=True)
    want, want_s = optical_flow.super_resolve(f, [], [], 3, 5.0, return_support=True)
    assert out.shape == (1, 60, 90, 3) and np.array_equal(out[0], want) and np.array_equal(sup[0], want_s)
    ref, ref_s = sn.super_resolve(f, [], [], 3, 5.0)
    assert np.array_equal(bits(out[0]), bits(ref)) and np.array_equal(bits(sup[0]), bits(ref_s))


# ---- lifecycle ---------------------------------------------------------------
def test_lifecycle_and_device_bytes():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    frames = clip_frames(H, W, 1, 3, 8, 4.0)
    f0 = _native.f32(frames[0])
    out = np.empty((2 * H, 2 * W), np.float32)
    idx = C.c_int32(0)

    def raw_push():
        return lib.of_sr_push(h, _native.ptr(f0), _native.ptr(out), None, C.byref(idx))

    def raw_flush():
        return lib.of_sr_flush(h, _native.ptr(out), None, C.byref(idx))

    for rc in (raw_push(), raw_flush(), lib.of_sr_close(h)):
        assert rc == _abi.OF_EINVAL
        with pytest.raises(ValueError, match="no super-resolver"):
            ctx.check(rc)

    base = optical_flow.super_resolve_frames(frames, sigma=8.0, radius=1)  # also grows the arena to what these pairs need
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    watch = []
    with optical_flow.SuperResolver((H, W), sigma=8.0, radius=1) as sr:
        watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        with pytest.raises(ValueError, match="super-resolver is open"):
            optical_flow.SuperResolver((H, W), sigma=8.0)  # one super-resolver per context
        got = {}
        with optical_flow.TemporalDenoiser((H, W), sigma=8.0) as dn, \
                optical_flow.PointTracker((H, W), step=4, min_eig=1.0) as tr:  # a denoiser and a tracker beside it
            for f in frames:
                r = sr.push(f)
                dn.push(f)
                tr.push(f)
                if r:
                    got[r[0]] = r[1]
                watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
            other_bytes = watch[-1] - watch[0]
            # the flow scale names the other kinds only: 8 stays refused, and the open super-resolver is untouched
            up = _abi.OfUpsampleOpts(2, 0, 20.0)
            assert lib.of_session_set_flow_scale(h, 8, C.byref(up)) == _abi.OF_EINVAL
        got.update(dict(sr.flush()))
        with pytest.raises(ValueError, match="flushed"):
            sr.push(frames[0])
    # 3 frames and 2 pairs' flows and states, counted from open to close
    pitch = (W + 63) // 64 * 64
    assert watch[0] - b0 == 3 * H * W * 4 + 2 * (2 * H * pitch * 8 + 2 * H * W), (b0, watch)
    assert other_bytes > 0 and all(w == watch[1] for w in watch[1:])
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    for t in range(3):
        assert np.array_equal(got[t], base[t])
    assert lib.of_sr_close(h) == _abi.OF_EINVAL
    # refused while a pair stream is open on the context
    with optical_flow.PairStream(H, W, 1, "classic+nl-fast", lanes=1) as ps:
        with pytest.raises(ValueError, match="pair stream is open"):
            optical_flow.SuperResolver((H, W), sigma=8.0, context=ps._ctx)
    # the C entries check for themselves
    P = optical_flow.load_of_method("classic+nl-fast").to_params()
    z = _native.f32(np.zeros((2, H, W)))
    names = ("factor", "radius", "patch", "pad_", "sigma", "strength", "reach", "back", "alpha1", "alpha2")

    def opts(**kw):
        a = dict(factor=2, radius=1, patch=2, pad_=0, sigma=8.0, strength=4.0, reach=0.75, back=0.0, alpha1=0.01,
                 alpha2=0.5)
        a.update(kw)
        return _abi.OfSrOpts(*[a[k] for k in names])

    def resolve(o, Cc=1, n=1, HH=H, WW=W):
        return lib.of_super_resolve(h, _native.ptr(f0), HH, WW, Cc, n, _native.ptr(f0), _native.ptr(z), None,
                                    C.byref(o), _native.ptr(out), None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(factor=1), dict(factor=5), dict(radius=0), dict(radius=3), dict(patch=-1), dict(patch=4),
               dict(sigma=0.0), dict(sigma=nan), dict(strength=inf), dict(strength=0.0), dict(reach=0.7),
               dict(reach=1.6), dict(reach=nan), dict(back=-0.1), dict(back=1.1), dict(back=nan), dict(alpha1=-1.0),
               dict(alpha2=nan)):
        with pytest.raises(ValueError):
            ctx.check(resolve(opts(**kw)))
        with pytest.raises(ValueError):
            ctx.check(lib.of_sr_open(h, C.byref(P), H, W, 1, C.byref(opts(**kw))))
    for kw in (dict(Cc=0), dict(Cc=5), dict(n=-1), dict(n=9)):
        with pytest.raises(ValueError):
            ctx.check(resolve(opts(), **kw))
    with pytest.raises(ValueError):
        ctx.check(lib.of_sr_open(h, C.byref(P), H, W, 2, C.byref(opts())))
    with pytest.raises(NotImplementedError):
        ctx.check(resolve(opts(), HH=46341, WW=46341))
    with pytest.raises(NotImplementedError):
        ctx.check(resolve(opts(factor=4), HH=16384, WW=8192))  # H * W fits, s*s*H*W is 2^31
    with pytest.raises(NotImplementedError):
        ctx.check(lib.of_sr_open(h, C.byref(P), 46341, 46341, 1, C.byref(opts())))
    ctx.check(resolve(opts()))  # and the good call goes through,
    ctx.check(lib.of_super_resolve(h, _native.ptr(f0), H, W, 1, 0, None, None, None, C.byref(opts()),
                                   _native.ptr(out), None))  # with no neighbours and no pointers too
    assert lib.of_sr_close(h) == _abi.OF_EINVAL  # none of the refused opens left a session behind


# ---- end to end ----------------------------------------------------------------
def test_end_to_end_on_the_prototype_scene():
    """The prototype scene as a clip: five 48 x 64 frames, the centre in the
    middle of its four neighbours (high-resolution offsets (1,2), (-2,1),
    (0,0), (3,-1), (-1,-3)), Gaussian noise sigma = 5, `sigma` 7.5, factor 2,
    radius 2; the middle frame, 8 high-resolution pixels of border left out.
    Measured MSE against the high-resolution truth: super_resolve_frames
    12.03, super_resolve along the known flows 12.01 (12.06 in the numpy
    prototype, another noise seed), bilinear upsample of the centre frame
    26.61 (26.91).  The gate is the last one only: the estimator had not been
    run on these frames before."""
    import optical_flow
    truth, center, neigh, flows = sn.scene(2, 5.0)
    clip = [neigh[0], neigh[1], center, neigh[2], neigh[3]]
    out, sup = optical_flow.super_resolve_frames(clip, "classic+nl-fast", factor=2, sigma=7.5, radius=2,
                                                 return_support=True)
    known = optical_flow.super_resolve(center, neigh, flows, 2, 7.5)
    e_out, e_known = sn.interior_mse(out[2], truth, 2), sn.interior_mse(known, truth, 2)
    e_bil = sn.interior_mse(sn.bilinear_upsample(center, 2), truth, 2)
    alone = optical_flow.super_resolve(center, [], [], 2, 7.5, return_support=True)[1]
    print(f"prototype scene as a clip, noise 5, sigma 7.5, factor 2, interior MSE: super_resolve_frames {e_out:.2f}, "
          f"known flows {e_known:.2f}, bilinear {e_bil:.2f}; mean support {sup[2].mean():.3f} "
          f"(single frame {alone.mean():.3f})")
    assert out.shape == (5, 96, 128)
    assert e_out < e_bil
