"""GPU tests of the reduced-resolution flow (include/optflow.h, "Reduced-
resolution flow with edge-aware upsampling"): of_reduce_frame and
of_flow_upsample bitwise against the numpy restatement (tests/upsample_numpy.py)
at tile-seam and degenerate shapes, the one-call scaled entries against the
composition of the stage entries, the three sessions with scale=2 against
their parts, and the accuracy of the scaled estimate end to end."""
import ctypes as C

import numpy as np
import pytest

import fuse_numpy as fn
import motion_numpy as mn
import upsample_numpy as un

pytestmark = pytest.mark.gpu

METHOD = "classic+nl-fast"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_f32(got, want):
    """float32 arrays equal bit for bit, NaN matching NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) \
        and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---- the stage entries, bitwise ----------------------------------------------
def stage_case(H, W, Cc, s, seed):
    """A guide with one NaN pixel, its clean reduction and a low flow with NaN
    / Inf specks and a +-1e30 value."""
    rng = np.random.default_rng(seed)
    hs, ws = un.low_shape(H, W, s)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.where((xx + yy) % 11 < 5, 60.0, 150.0)[..., None] + rng.uniform(-12, 12, (H, W, Cc))
    guide = base.astype(np.float32)
    guide = guide[..., 0] if Cc == 1 else guide
    f = rng.normal(0, 3, (hs, ws, 2)).astype(np.float32)
    f[(hs // 2) % hs, (ws // 3) % ws, 0] = np.nan
    f[(hs // 3) % hs, (2 * ws // 3) % ws, 1] = np.inf
    f[hs - 1, ws - 1, 0] = -np.inf
    f[0, (ws // 2) % ws] = (1e30, -1e30)
    return guide, f


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 64), (9, 65), (17, 129), (67, 131)])
def test_reduce_and_upsample_bitwise_vs_numpy(H, W):
    import optical_flow
    for s in (2, 3, 4):
        for Cc in (1, 3, 4):
            guide, f = stage_case(H, W, Cc, s, 1000 * s + Cc)
            want_L = un.reduce_frame(guide, s)
            got_L = optical_flow.reduce_frame(guide, s)
            assert got_L.dtype == np.float64 and same_f32(got_L, want_L), (s, Cc)
            guide[H // 2, W // 2] = np.nan     # one pixel the low guide does not know about
            for rng_ in (20.0, 7.5):
                want, want_i = un.upsample(f, want_L, guide, s, rng_)
                got, got_i = optical_flow.upsample_flow(f, guide, s, rng_, guide_lo=want_L, return_info=True)
                assert got.dtype == np.float64 and got_i.dtype == np.uint8
                assert same_f32(got, want), (s, Cc, rng_,
                                             np.flatnonzero(bits(got.astype(np.float32)) != bits(want))[:8])
                assert np.array_equal(got_i, want_i), (s, Cc, rng_)
            assert want_i[H // 2, W // 2] != 0
            # without return_info, and with the low guide left to the library
            with np.errstate(invalid="ignore"):
                auto = optical_flow.upsample_flow(f, guide, s, 7.5)
            assert same_f32(auto, un.upsample(f, un.reduce_frame(guide, s), guide, s, 7.5)[0]), (s, Cc)


def test_stage_entries_refuse_bad_arguments_in_c():
    from optical_flow import _abi, _native as nat
    ctx = nat.context()
    im = np.zeros((8, 9, 3), np.float32)
    lo = np.zeros((4, 5, 3), np.float32)
    f = np.zeros((2, 4, 5), np.float32)
    out = np.zeros((2, 8, 9), np.float32)
    for scale in (1, 5, 0):
        assert ctx.lib.of_reduce_frame(ctx.handle, nat.ptr(im), 8, 9, 3, scale, nat.ptr(lo)) == _abi.OF_EINVAL
    assert ctx.lib.of_reduce_frame(ctx.handle, nat.ptr(im), 8, 9, 5, 2, nat.ptr(lo)) == _abi.OF_EINVAL
    assert ctx.lib.of_reduce_frame(ctx.handle, nat.ptr(im), 1 << 16, 1 << 15, 1, 2, nat.ptr(lo)) == _abi.OF_ENOTSUP
    for scale, rng_ in ((1, 20.0), (5, 20.0), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        up = _abi.OfUpsampleOpts(scale, 0, rng_)
        rc = ctx.lib.of_flow_upsample(ctx.handle, nat.ptr(f), nat.ptr(lo), nat.ptr(im), 8, 9, 3, C.byref(up),
                                      nat.ptr(out), None)
        assert rc == _abi.OF_EINVAL, (scale, rng_)
    up = _abi.OfUpsampleOpts(2, 0, 20.0)
    assert ctx.lib.of_flow_upsample(ctx.handle, nat.ptr(f), nat.ptr(lo), nat.ptr(im), 1 << 16, 1 << 15, 3,
                                    C.byref(up), nat.ptr(out), None) == _abi.OF_ENOTSUP


# ---- the one-call entries are the composition of the stages -------------------
def c_bidir(a, b, up=None, alpha1=0.01, alpha2=0.5):
    """of_estimate_flow_bidir[_scaled] through the C ABI: (fw, bw, sf, sb,
    stats_fw, stats_bw), flows (H, W, 2) float64."""
    from optical_flow import _abi, _native as nat
    from optical_flow._session import method_params
    P = method_params(METHOD, None)[1]
    a, b = nat.f32(a), nat.f32(b)
    H, W = a.shape[:2]
    Cc = 3 if a.ndim == 3 else 1
    of, ob = np.empty((2, H, W), np.float32), np.empty((2, H, W), np.float32)
    sf, sb = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)
    tf, tb = _abi.OfStats(), _abi.OfStats()
    ctx = nat.context()
    if up is None:
        ctx.check(ctx.lib.of_estimate_flow_bidir(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc, None, None,
                                                 nat.ptr(of), nat.ptr(ob), alpha1, alpha2, nat.u8ptr(sf), nat.u8ptr(sb),
                                                 C.byref(tf), C.byref(tb)))
    else:
        ctx.check(ctx.lib.of_estimate_flow_bidir_scaled(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, Cc,
                                                        C.byref(up), alpha1, alpha2, nat.ptr(of), nat.ptr(ob),
                                                        nat.u8ptr(sf), nat.u8ptr(sb), C.byref(tf), C.byref(tb)))
    return nat.interleaved(of), nat.interleaved(ob), sf, sb, tf.as_dict(), tb.as_dict()


def level_sizes(st):
    return [(lv["h"], lv["w"], lv["stage"]) for lv in st["levels"]]


def test_bidir_scaled_is_the_composition_of_the_stage_entries():
    import optical_flow
    from optical_flow import _abi, _native as nat
    from optical_flow._session import method_params
    from optical_flow.utils.synthetic import synth_pair
    H, W, s, rng_ = 67, 131, 2, 20.0
    im1, im2, _ = synth_pair(H, W, seed=7)
    up = _abi.OfUpsampleOpts(s, 0, rng_)
    fw, bw, sf, sb, tf, tb = c_bidir(im1, im2, up)
    # the composition, through the host
    L1, L2 = optical_flow.reduce_frame(im1, s), optical_flow.reduce_frame(im2, s)
    assert L1.shape == (34, 66, 3)
    lf, lb, _, _, ltf, ltb = c_bidir(L1, L2)
    want_fw = optical_flow.upsample_flow(lf, im1, s, rng_, guide_lo=L1)
    want_bw = optical_flow.upsample_flow(lb, im2, s, rng_, guide_lo=L2)
    assert np.array_equal(fw, want_fw) and np.array_equal(bw, want_bw)
    assert np.array_equal(sf, optical_flow.forward_backward_check(want_fw, want_bw))
    assert np.array_equal(sb, optical_flow.forward_backward_check(want_bw, want_fw))
    assert level_sizes(tf) == level_sizes(ltf) and level_sizes(tb) == level_sizes(ltb) and len(tf["levels"]) > 0
    assert all(h <= 34 and w <= 66 for h, w, _ in level_sizes(tf))
    for k in ("solves", "solver_iters_total", "solver_iters_max", "solves_not_converged"):
        assert tf[k] == ltf[k] and tb[k] == ltb[k], k
    # the one-direction entry is the forward half; the Python keywords make these calls
    P = method_params(METHOD, None)[1]
    out = np.empty((2, H, W), np.float32)
    st = _abi.OfStats()
    ctx = nat.context()
    a, b = nat.f32(im1), nat.f32(im2)
    ctx.check(ctx.lib.of_estimate_flow_scaled(ctx.handle, C.byref(P), nat.ptr(a), nat.ptr(b), H, W, 3, C.byref(up),
                                              nat.ptr(out), C.byref(st)))
    assert np.array_equal(nat.interleaved(out), fw) and level_sizes(st.as_dict()) == level_sizes(tf)
    assert np.array_equal(optical_flow.estimate_flow(im1, im2, METHOD, scale=s), fw)
    r = optical_flow.estimate_flow_bidirectional(im1, im2, METHOD, scale=s, upsample_range=rng_)
    assert np.array_equal(r.forward, fw) and np.array_equal(r.backward, bw)
    assert np.array_equal(r.occ_forward, sf) and np.array_equal(r.occ_backward, sb)
    # gray frames, another scale and range: still the composition
    g1, g2 = im1[..., 1], im2[..., 1]
    r = optical_flow.estimate_flow_bidirectional(g1, g2, METHOD, scale=3, upsample_range=12.0)
    G1, G2 = optical_flow.reduce_frame(g1, 3), optical_flow.reduce_frame(g2, 3)
    low = optical_flow.estimate_flow_bidirectional(G1, G2, METHOD)
    assert np.array_equal(r.forward, optical_flow.upsample_flow(low.forward, g1, 3, 12.0))
    assert np.array_equal(r.backward, optical_flow.upsample_flow(low.backward, g2, 3, 12.0))
    # interpolate_frames with scale estimates the same flows
    mid = optical_flow.interpolate_frames(im1, im2, 0.5, METHOD, scale=s)
    assert np.array_equal(mid, optical_flow.interpolate_frames(im1, im2, 0.5, flows=(fw, bw)))


# ---- the sessions --------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    """A 4-frame 48 x 80 RGB clip and (fw, bw, sf, sb) of every adjacent pair
    from the one-call scaled entry at scale 2, computed once."""
    import optical_flow
    from test_gpu_fuse import clip_frames
    frames = clip_frames(48, 80, 3, 4, 61, 3.0)
    pairs = []
    for a, b in zip(frames[:-1], frames[1:]):
        r = optical_flow.estimate_flow_bidirectional(a, b, METHOD, scale=2)
        pairs.append((r.forward, r.backward, r.occ_forward, r.occ_backward))
    return frames, pairs


def test_tracker_with_scale_pushes_the_scaled_pair(clip):
    import optical_flow
    frames, pairs = clip
    prev = None
    with optical_flow.PointTracker(frames[0].shape, METHOD, scale=2) as tr:
        for k, f in enumerate(frames):
            snap = tr.push(f, return_flows=True)
            if k == 0:
                assert snap.forward is None and len(snap.xy) > 0
            else:
                fw, bw, sf, sb = pairs[k - 1]
                assert np.array_equal(snap.forward, fw) and np.array_equal(snap.backward, bw), k
                assert np.array_equal(snap.occ_forward, sf) and np.array_equal(snap.occ_backward, sb), k
                assert all(lv["h"] <= 24 and lv["w"] <= 40 for lv in tr.last_stats[0]["levels"])
                # the table moved along those full-resolution flows
                want_xy, want_st = optical_flow.advance_points(prev.xy, fw, bw, prev.status)
                n = len(prev.xy)
                assert np.array_equal(snap.xy[:n], want_xy) and np.array_equal(snap.status[:n], want_st), k
            prev = snap


def test_denoiser_with_scale_equals_its_parts(clip):
    import optical_flow
    frames, pairs = clip
    sigma = 3.0
    want = fn.session(
        frames, pairs, sigma, 1, 4.0, 2,
        compose_fn=lambda f, g, a, b: optical_flow.compose_flows(f, g, a, b, return_state=True),
        fuse_fn=lambda c, nb, fl, s, st, strength, patch: optical_flow.fuse_frames(c, nb, fl, s, st, strength, patch,
                                                                                   return_weight=True))
    out, wgt = optical_flow.denoise_frames(frames, METHOD, sigma=sigma, radius=1, return_weight=True, scale=2)
    for t in range(4):
        assert np.array_equal(out[t], want[t][0]), (t, np.abs(out[t] - want[t][0]).max())
        assert np.array_equal(wgt[t], want[t][1]), t
    assert wgt[1].mean() > 1.5   # it did fuse along the upsampled flows


def test_stabiliser_with_scale_equals_its_parts(clip):
    import optical_flow
    frames, pairs = clip
    R, sigma_t = 1, 2.0
    motions, out = [], {}
    with optical_flow.Stabilizer(frames[0].shape, METHOD, radius=R, sigma_t=sigma_t, scale=2) as st:
        for k, f in enumerate(frames):
            r = st.push(f)
            if k > 0:
                motions.append(st.last_motion.copy())
            if r is not None:
                out[r[0]] = (r[1], st.last_transform)
        for r in st.flush():
            out[r[0]] = (r[1], st.last_transform)
    for k, (fw, _, sf, _) in enumerate(pairs):
        want = optical_flow.fit_motion(fw, "similarity", state=sf)
        assert np.array_equal(bits(motions[k]), bits(want.matrix)), k
    kept = [mn.keep(m)[0] for m in motions]
    pushes, flush = mn.session_schedule(4, R)
    sched = {t: n for t, n in pushes + flush if t >= 0}
    assert sorted(out) == [0, 1, 2, 3]
    for t in range(4):
        S = mn.smooth(kept, t, sched[t], R, sigma_t)
        assert np.array_equal(bits(out[t][1]), bits(S)), t
        want_o = optical_flow.warp_affine(frames[t], np.reshape(mn.inv(S), (2, 3)))
        assert np.array_equal(out[t][0], want_o), t


def test_scale_1_is_the_session_without_the_keyword(clip):
    import optical_flow
    frames = clip[0][:3]
    a = optical_flow.track_points(frames, METHOD)
    b = optical_flow.track_points(frames, METHOD, scale=1, upsample_range=5.0)
    assert np.array_equal(bits(a.xy), bits(b.xy)) and np.array_equal(a.status, b.status)
    a = optical_flow.denoise_frames(frames, METHOD, sigma=3.0)
    b = optical_flow.denoise_frames(frames, METHOD, sigma=3.0, scale=1)
    assert np.array_equal(a, b)
    a = optical_flow.stabilize_frames(frames, METHOD, radius=1)
    b = optical_flow.stabilize_frames(frames, METHOD, radius=1, scale=1)
    assert np.array_equal(a, b)
    # and the scale does change the flows
    c = optical_flow.denoise_frames(frames, METHOD, sigma=3.0, scale=2)
    assert not np.array_equal(a, c)
    r1 = optical_flow.estimate_flow_bidirectional(frames[0], frames[1], METHOD, scale=1)
    r0 = optical_flow.estimate_flow_bidirectional(frames[0], frames[1], METHOD)
    assert np.array_equal(r1.forward, r0.forward) and np.array_equal(r1.occ_backward, r0.occ_backward)
    assert not np.array_equal(r0.forward, clip[1][0][0])


def test_set_flow_scale_lifecycle_and_device_bytes(clip):
    import optical_flow
    from optical_flow import _abi, _native as nat
    frames = clip[0]
    shape = frames[0].shape
    ctx = nat.Context(0)
    try:
        up = _abi.OfUpsampleOpts(2, 0, 20.0)
        off = _abi.OfUpsampleOpts(1, 0, 0.0)
        kinds = {"t": _abi.OF_SESSION_TRACKS, "d": _abi.OF_SESSION_DENOISE, "s": _abi.OF_SESSION_STAB}

        def set_scale(k, o):
            return ctx.lib.of_session_set_flow_scale(ctx.handle, k, C.byref(o))

        # no session of that kind open, or no kind at all
        for k in list(kinds.values()) + [7, 0, 8, -1]:
            assert set_scale(k, up) == _abi.OF_EINVAL, k
        # grow the arena to what the full-resolution pair needs, so that it stays flat below
        with optical_flow.PointTracker(shape, METHOD, context=ctx) as tr:
            tr.push(frames[0])
            tr.push(frames[1])
        b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
        with optical_flow.PointTracker(shape, METHOD, context=ctx):
            b_plain = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
        with optical_flow.PointTracker(shape, METHOD, context=ctx, scale=2) as tr:
            assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b_plain > b0
            # bad options change nothing; another kind is still not open
            for o in (_abi.OfUpsampleOpts(5, 0, 20.0), _abi.OfUpsampleOpts(0, 0, 20.0), _abi.OfUpsampleOpts(2, 0, 0.0),
                      _abi.OfUpsampleOpts(2, 0, float("nan"))):
                assert set_scale(kinds["t"], o) == _abi.OF_EINVAL
            assert set_scale(kinds["t"] | kinds["d"], up) == _abi.OF_EINVAL
            tr.push(frames[0])
            assert set_scale(kinds["t"], off) == _abi.OF_OK     # still before the first pair: clear ...
            assert set_scale(kinds["t"], up) == _abi.OF_OK      # ... and set again
            s1 = tr.push(frames[1], return_flows=True)
            assert np.array_equal(s1.forward, clip[1][0][0])
            assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b_plain
            assert set_scale(kinds["t"], up) == _abi.OF_EINVAL  # after the second push
            assert set_scale(kinds["t"], off) == _abi.OF_EINVAL
            assert b"second push" in ctx.lib.of_last_error(ctx.handle)
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
        # several kinds in one call
        with optical_flow.TemporalDenoiser(shape, METHOD, sigma=3.0, context=ctx) as dn, \
                optical_flow.Stabilizer(shape, METHOD, radius=1, context=ctx) as st:
            assert set_scale(kinds["d"] | kinds["s"], up) == _abi.OF_OK
            assert set_scale(7, up) == _abi.OF_EINVAL          # the tracker is not open
            dn.push(frames[0])
            dn.push(frames[1])
            # the denoiser has its pair: neither session changes
            assert set_scale(kinds["d"] | kinds["s"], off) == _abi.OF_EINVAL
            st.push(frames[0])
            r = st.push(frames[1])
            want = optical_flow.fit_motion(clip[1][0][0], "similarity", state=clip[1][0][2])
            assert np.array_equal(bits(st.last_motion), bits(want.matrix)) and r is not None
    finally:
        ctx.close()


# ---- accuracy, end to end -----------------------------------------------------
def test_scaled_estimate_keeps_the_motion_boundary_better_than_a_plain_resize():
    """96 x 128 two-layer pair, background (0.5, 0), rectangle (3, -2); AEPE
    over all pixels and over the band within 2 pixels of the rectangle's
    outline, of the full-resolution estimate, the scale-2 estimate and the
    same low flow resized bilinearly (of_resample_flow, x2)."""
    import optical_flow
    from optical_flow.utils.synthetic import two_layer_pair
    from optical_flow.utils.warping import resample_flow
    H, W, s = 96, 128, 2
    im1, im2, gt, mask = two_layer_pair(H, W, seed=5)
    band = un.outline_band(mask, s)

    def aepe(uv):
        e = np.sqrt(((uv - gt) ** 2).sum(-1))
        return float(e.mean()), float(e[band].mean())

    full = aepe(optical_flow.estimate_flow(im1, im2, METHOD))
    scaled = aepe(optical_flow.estimate_flow(im1, im2, METHOD, scale=s))
    low = optical_flow.estimate_flow(optical_flow.reduce_frame(im1, s), optical_flow.reduce_frame(im2, s), METHOD)
    plain = aepe(resample_flow(low, (H, W)))
    print(f"AEPE all / band: full {full[0]:.4f} / {full[1]:.4f}, scale 2 {scaled[0]:.4f} / {scaled[1]:.4f}, "
          f"bilinear {plain[0]:.4f} / {plain[1]:.4f}; scaled / full {scaled[0] / full[0]:.4f}")
    assert scaled[1] < plain[1]
    # Measured on an MI355X: full 0.1940 / 0.8070, scale 2 0.2332 / 0.7063,
    # bilinear 0.2581 / 1.0491 (all pixels / band).  The gate against the
    # full-resolution estimate is the measured ratio of the all-pixel AEPEs,
    # 0.2332 / 0.1940 = 1.2017, plus a quarter of it for the solver's rounding
    # between machines: 1.2017 * 1.25 = 1.502.
    assert scaled[0] <= 1.502 * full[0]
