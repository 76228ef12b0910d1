"""Mask propagation on the GPU: of_mask_advance bitwise against the numpy
float64 restatement (tests/mask_numpy.py), the session (of_masks_*) bitwise
against its parts run by hand, its lifecycle, and end-to-end runs on the
recoloured scene of the CPU tests with estimated flows, alone and chained into
the inpainter."""
import ctypes as C

import numpy as np
import pytest

import mask_numpy as mk
from test_gpu_inpaint import clip_frames, make_masks, plant
from test_mask_cpu import IOU_HELD_STILL, MEAN_HELD_STILL, MEAN_LAYERED

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 1), (3, 130), (37, 53), (64, 65)]
RADII, SMOOTHS, RANGES = (1, 8, 12), (0, 1, 2), (1e-3, 20.0, 1e4)


def advance_case(H, W, Cc, seed):
    """(guide, flow, states): a guide of uniform colours, a flow uniform in
    +-6 with the planted cases, and the two state planes of the tests: None,
    and random over {0, 1, 2, 255} at 30 % (above 1000 pixels with a 4 x 4
    block of untrusted pixels in the middle, whose inside no radius-1 window
    gets out of)."""
    rng = np.random.default_rng(seed)
    G = rng.uniform(0, 255, (H, W) if Cc == 1 else (H, W, Cc)).astype(np.float32)
    flow = plant(rng.uniform(-6, 6, (H, W, 2)).astype(np.float32))
    S = np.where(rng.uniform(size=(H, W)) < 0.3, rng.choice(np.array([1, 2, 255], np.uint8), (H, W)), 0).astype(np.uint8)
    if H * W > 1000:
        S[H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = 1
    return rng, G, flow, (None, S)


def check_advance(M, G, flow, S, seen, key, radii=RADII, ranges=RANGES, smooths=SMOOTHS):
    import optical_flow
    A = mk.carry(M, flow, S)
    for R in radii:
        for rng_ in ranges:
            lab, want_st = mk.vote(A, G, R, rng_, seen)
            for s in smooths:
                want = mk.mode(lab, s, seen)
                out, st = optical_flow.advance_mask(M, G, flow, S, R, rng_, s, return_status=True)
                assert out.dtype == np.uint8 and out.shape == M.shape and st.dtype == np.uint8 and st.shape == M.shape
                bad = np.argwhere(st != want_st)
                assert bad.size == 0, (key, R, rng_, s, bad[:5])
                bad = np.argwhere(out != want)
                assert bad.size == 0, (key, R, rng_, s, bad[:5])


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_advance_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    seen = set()
    rng, G, flow, states = advance_case(H, W, Cc, 1000 * H + W + 7 * Cc)
    for kind in ("random", "empty", "full", "corner"):
        M = make_masks(kind, 1, H, W, rng)[0]
        for k, S in enumerate(states):
            if kind == "random":
                check_advance(M, G, flow, S, seen, (kind, k))
            else:  # the mask changes the carried values only, not who is decided: one radius per range and smooth
                for R, rng_, s in zip(RADII, RANGES, SMOOTHS):
                    check_advance(M, G, flow, S, seen, (kind, k), (R,), (rng_,), (s,))
    only = optical_flow.advance_mask(M, G, flow)
    assert isinstance(only, np.ndarray) and only.dtype == np.uint8
    assert np.array_equal(only, mk.advance(M, G, flow)[0])
    if H * W > 1000:
        assert seen == mk.BRANCHES, mk.BRANCHES - seen  # every branch occurred


def test_advance_two_channels_a_guide_that_is_not_finite_and_other_dtypes():
    import optical_flow
    H, W = 37, 53
    seen = set()
    rng, G, flow, (_, S) = advance_case(H, W, 2, 77)
    M = make_masks("random", 1, H, W, rng)[0]
    check_advance(M, G, flow, S, seen, "two channels", (1, 8), (20.0, 1e4), (1,))
    for Cc, bad in ((3, np.nan), (1, np.inf), (4, np.nan)):
        rng, G, flow, (_, S) = advance_case(H, W, Cc, 78 + Cc)
        G.reshape(H, W, -1)[H // 2 + 3, W // 2 - 5, -1] = bad    # one pixel; a neighbour of the untrusted block
        S[H // 2 + 3, W // 2 - 5] = 0
        check_advance(M, G, flow, S, seen, ("not finite", Cc), (8, 12), (20.0, 1e4), (0, 1))
        S[H // 2 + 3, W // 2 - 5] = 1                              # and undecided itself: no weight at all, so the count
        check_advance(M, G, flow, S, seen, ("not finite, undecided", Cc), (8,), (1e4,), (0,))
    assert seen == mk.BRANCHES, mk.BRANCHES - seen
    a = optical_flow.advance_mask(M, G, flow, S)
    assert np.array_equal(a, optical_flow.advance_mask(M != 0, G.astype(np.float64), flow.astype(np.float64),
                                                       S.astype(np.int64)))
    assert np.array_equal(a, optical_flow.advance_mask(-(M.astype(np.int64)), G, flow, S))


# ---- the session equals its parts ------------------------------------------
def scene_clip(Cc):
    """4 frames of 37 x 53 and their true masks: the first frames of the
    recoloured scene, cropped around the rectangle; for 3 channels the plane
    and two darker copies of it."""
    fr, ms = mk.scene(0)[:2]
    frames = [f[5:42, 2:55].astype(np.float64) for f in fr[:4]]
    if Cc == 3:
        frames = [np.stack([f, 0.5 * f + 40.0, 0.9 * f], axis=2) for f in frames]
    return frames, [m[5:42, 2:55].copy() for m in ms[:4]]


@pytest.mark.parametrize("Cc", [1, 3])
def test_session_equals_its_parts(Cc):
    import optical_flow
    H, W = 37, 53
    frames, masks = scene_clip(Cc)
    keys = [masks[0], None, None, None]

    def pair(a, b):
        r = optical_flow.estimate_flow_bidirectional(a, b, "classic+nl-fast", alpha1=0.02, alpha2=0.4)
        return r.backward, r.occ_backward

    want = mk.session(frames, keys, pair,
                      lambda m, f, bw, sb: optical_flow.advance_mask(m, f, bw, sb, 6, 30.0, 1, return_status=True))
    with optical_flow.MaskPropagator(H, W, Cc, "classic+nl-fast", vote_radius=6, vote_range=30.0, smooth=1, alpha1=0.02,
                                     alpha2=0.4) as mp:
        assert (mp.vote_radius, mp.vote_range, mp.smooth, mp.last_status) == (6, 30.0, 1, None)
        for k, (f, m) in enumerate(zip(frames, keys)):
            got = mp.push(f, m)
            assert got.dtype == np.uint8 and got.shape == (H, W) and mp.last_status.dtype == np.uint8
            assert np.array_equal(mp.last_status, want[k][1]), k
            assert np.array_equal(got, want[k][0]), k
        assert mp.frames == 4
    # the run is not a trivial one: the object is still followed at the last frame, and pixels were voted
    assert mk.iou(want[3][0], masks[3]) > 0.5 and (want[3][1] == mk.VOTED).any()
    out, st = optical_flow.propagate_masks(frames, masks[0], "classic+nl-fast", 6, 30.0, 1, 0.02, 0.4, return_status=True)
    for k in range(4):
        assert np.array_equal(out[k], want[k][0]) and np.array_equal(st[k], want[k][1]), k


# ---- lifecycle ---------------------------------------------------------------
def test_lifecycle_and_device_bytes():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    frames, masks = clip_frames(H, W, 1, 3, 8)
    f0, m0 = _native.f32(frames[0]), masks[0]
    out, st = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)

    def raw_push(mask=m0, dst=out, frame=f0):
        return lib.of_masks_push(h, _native.ptr(frame), _native.u8ptr(mask), _native.u8ptr(dst), _native.u8ptr(st))

    for rc in (raw_push(), lib.of_masks_close(h)):
        assert rc == _abi.OF_EINVAL
        with pytest.raises(ValueError, match="no mask propagator"):
            ctx.check(rc)

    base = optical_flow.propagate_masks(frames, masks[0])  # also grows the arena to what these pairs need
    after_anchor = optical_flow.propagate_masks(frames[1:], masks[1])[1]
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    watch = []
    with optical_flow.MaskPropagator(H, W, 1) as mp:
        watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
        with pytest.raises(ValueError, match="mask propagator is open"):
            optical_flow.MaskPropagator(H, W, 1)  # one per context
        with pytest.raises(ValueError, match="takes a mask"):
            mp.push(frames[0])  # the first push without a mask, refused in Python ...
        assert raw_push(mask=None) == _abi.OF_EINVAL  # ... and by the library
        with pytest.raises(ValueError, match="takes a mask"):
            ctx.check(raw_push(mask=None))
        assert raw_push(dst=None) == _abi.OF_EINVAL and raw_push(frame=None) == _abi.OF_EINVAL
        assert mp.frames == 0
        with optical_flow.VideoInpainter(H, W, 1, radius=1) as vi:  # beside an open inpainter
            got = []
            for k, f in enumerate(frames):
                got.append(mp.push(f, masks[0] if k == 0 else None))
                assert (mp.last_status == _abi.OF_MASK_GIVEN).all() == (k == 0)
                vi.push(f, masks[k])
                watch.append(ctx.get_option(_abi.OF_OPT_DEVICE_BYTES))
            other_bytes = watch[-1] - watch[0]
            # the flow scale names the three older kinds only: this session's bit stays refused
            up = _abi.OfUpsampleOpts(2, 0, 20.0)
            assert lib.of_session_set_flow_scale(h, 32, C.byref(up)) == _abi.OF_EINVAL
        for k in range(3):
            assert np.array_equal(got[k], base[k]), k
        # a re-anchor: the given mask comes back as mask != 0, MASK_GIVEN everywhere, and the next push follows it
        anchor = mp.push(frames[1], masks[1] * 7)
        assert np.array_equal(anchor, masks[1]) and (mp.last_status == optical_flow.MASK_GIVEN).all()
        nxt = mp.push(frames[2])
        assert np.array_equal(nxt, after_anchor)
        assert mp.frames == 5
    # two frames and the mask, counted from open to close
    assert watch[0] - b0 == 2 * H * W * 4 + H * W, (b0, watch)
    assert other_bytes > 0 and all(w == watch[1] for w in watch[1:])
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    with pytest.raises(ValueError, match="mask propagator is closed"):
        mp.push(frames[0], masks[0])  # a push after close, in Python ...
    assert raw_push() == _abi.OF_EINVAL and lib.of_masks_close(h) == _abi.OF_EINVAL  # ... and in the library
    # a destroyed context frees its open session
    c2 = _native.Context()
    mp2 = optical_flow.MaskPropagator(H, W, 1, context=c2)
    assert np.array_equal(mp2.push(frames[0], masks[0]), masks[0])
    c2.close()
    mp2.close()
    # refused while a pair stream is open on the context
    with optical_flow.PairStream(H, W, 1, "classic+nl-fast", lanes=1) as ps:
        with pytest.raises(ValueError, match="pair stream is open"):
            optical_flow.MaskPropagator(H, W, 1, context=ps._ctx)
    # the C entries check for themselves
    P = optical_flow.load_of_method("classic+nl-fast").to_params()
    z = _native.f32(np.zeros((2, H, W)))
    good = (8, 1, 20.0, 0.01, 0.5)

    def advance(o, Cc=1, HH=H, WW=W, mask=m0, guide=f0, flow=z, dst=out):
        return lib.of_mask_advance(h, _native.u8ptr(mask), _native.ptr(guide), HH, WW, Cc, _native.ptr(flow), None,
                                   C.byref(_abi.OfMaskOpts(*o)), _native.u8ptr(dst), None)

    nan, inf = float("nan"), float("inf")
    for bad in ((0, 1, 20.0, 0.01, 0.5), (13, 1, 20.0, 0.01, 0.5), (8, -1, 20.0, 0.01, 0.5), (8, 3, 20.0, 0.01, 0.5),
                (8, 1, 0.0, 0.01, 0.5), (8, 1, -1.0, 0.01, 0.5), (8, 1, nan, 0.01, 0.5), (8, 1, inf, 0.01, 0.5),
                (8, 1, 20.0, -0.01, 0.5), (8, 1, 20.0, 0.01, nan)):
        with pytest.raises(ValueError):
            ctx.check(advance(bad))
        with pytest.raises(ValueError):
            ctx.check(lib.of_masks_open(h, C.byref(P), H, W, 1, C.byref(_abi.OfMaskOpts(*bad))))
    for kw in (dict(Cc=0), dict(Cc=5), dict(mask=None), dict(guide=None), dict(flow=None), dict(dst=None), dict(HH=0)):
        with pytest.raises(ValueError):
            ctx.check(advance(good, **kw))
    with pytest.raises(ValueError):
        ctx.check(lib.of_masks_open(h, C.byref(P), H, W, 2, C.byref(_abi.OfMaskOpts(*good))))
    with pytest.raises(NotImplementedError):
        ctx.check(advance(good, HH=46341, WW=46341))
    with pytest.raises(NotImplementedError):
        ctx.check(lib.of_masks_open(h, C.byref(P), 46341, 46341, 1, C.byref(_abi.OfMaskOpts(*good))))
    ctx.check(advance((8, 0, 20.0, 0.01, 0.5)))  # and the good call goes through: zero flow, no smoothing
    assert np.array_equal(out, m0)
    assert lib.of_masks_close(h) == _abi.OF_EINVAL  # none of the refused opens left a session behind


# ---- end to end ----------------------------------------------------------------
@pytest.fixture(scope="module")
def the_scene():
    return mk.scene(0)


@pytest.fixture(scope="module")
def followed(the_scene):
    """propagate_masks of the scene from the mask of frame 0, once for the tests that use it."""
    import optical_flow
    return optical_flow.propagate_masks(the_scene[0], the_scene[1][0], return_status=True)


def _gates(got, masks, key, name):
    """Per-frame IoU above the mask of the keyframe held still, and the mean
    over the other 8 frames at least halfway from the held-still mean to the
    layered-flow mean of the CPU test."""
    others = [s for s in range(9) if s != key]
    ious = [mk.iou(got[s], masks[s]) for s in others]
    held = [mk.iou(masks[key], masks[s]) for s in others]
    print(f"{name}: IoU {[round(v, 3) for v in ious]} mean {np.mean(ious):.4f}; held still {[round(v, 3) for v in held]} "
          f"mean {np.mean(held):.4f}")
    assert np.array_equal(got[key], masks[key])
    for s, a, b in zip(others, ious, held):
        assert a > b, (s, a, b)
    assert np.mean(ious) >= 0.5 * (np.mean(held) + MEAN_LAYERED), np.mean(ious)
    return held


def test_end_to_end_on_the_scene(the_scene, followed):
    """The recoloured scene of the CPU tests (mask_numpy.scene: 9 frames of
    48 x 64, a bright 14 x 18 rectangle crossing a darker moving background)
    through a MaskPropagator at the defaults from the mask of frame 0, the
    flows estimated.  Gates: at every frame the IoU against the true mask is
    above that of the mask held still (0.647, 0.370, 0.203, 0.068, 0, 0, 0, 0),
    and the mean over frames 1 .. 8 is at least halfway between the held-still
    mean (0.161) and the mean along the true layered flows (0.981, pinned in
    tests/test_mask_cpu.py), that is 0.571: an estimate that loses more than
    half of what the motion gives is not following the object."""
    import optical_flow
    frames, masks = the_scene[0], the_scene[1]
    got, sts = [], []
    with optical_flow.MaskPropagator(48, 64, 1) as mp:
        for s, f in enumerate(frames):
            got.append(mp.push(f, masks[0] if s == 0 else None))
            sts.append(mp.last_status)
    held = _gates(got, masks, 0, "keyframe 0, forward")
    assert np.allclose(held, IOU_HELD_STILL, atol=5e-4) and abs(np.mean(held) - MEAN_HELD_STILL) < 5e-4
    assert (sts[0] == optical_flow.MASK_GIVEN).all() and all((st != optical_flow.MASK_GIVEN).all() for st in sts[1:])
    # propagate_masks is that loop
    assert np.array_equal(followed[0], np.stack(got)) and np.array_equal(followed[1], np.stack(sts))


def test_end_to_end_backward_from_the_last_frame(the_scene):
    """The same with the mask of frame 8 as the only keyframe, propagated
    backward by propagate_masks; held still now means the mask of frame 8, and
    the layered-flow mean is the forward one (the scene is the same motion run
    the other way)."""
    import optical_flow
    frames, masks = the_scene[0], the_scene[1]
    got, st = optical_flow.propagate_masks(frames, {8: masks[8]}, return_status=True)
    assert got.shape == (9, 48, 64) and got.dtype == np.uint8 and st.shape == (9, 48, 64)
    assert (st[8] == optical_flow.MASK_GIVEN).all() and (st[:8] != optical_flow.MASK_GIVEN).all()
    _gates(got, masks, 8, "keyframe 8, backward")


def test_chain_into_the_inpainter(the_scene, followed):
    """inpaint_frames with the propagated masks against inpaint_frames with
    the mask of frame 0 held still in every frame, radius 6, grow 2: the MSE
    against the recoloured truth over the true rectangle's pixels, all frames
    together, must be lower with the propagated masks."""
    import optical_flow
    frames, masks, _, _, truth = the_scene

    def mse(out):
        err = n = 0
        for o, m, tr in zip(out, masks, truth):
            hole = m != 0
            err += float(((o - tr.astype(np.float64)) ** 2)[hole].sum())
            n += int(hole.sum())
        return err / n

    chained = optical_flow.inpaint_frames(frames, followed[0], radius=6, grow=2)
    still = optical_flow.inpaint_frames(frames, [masks[0]] * 9, radius=6, grow=2)
    print(f"MSE over the rectangle: propagated masks {mse(chained):.2f}, mask held still {mse(still):.2f}, "
          f"untouched {mse([f.astype(np.float64) for f in frames]):.1f}")
    assert chained.shape == (9, 48, 64)
    assert mse(chained) < mse(still)
