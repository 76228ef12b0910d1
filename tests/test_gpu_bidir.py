"""Bidirectional flow with forward-backward occlusion masks on the GPU:
of_fb_consistency (k_fb_check) and of_estimate_flow_bidir (include/optflow.h).

The check kernel is compared bitwise with the numpy float64 restatement below,
which follows the header's formula operation for operation (the kernel runs
it in double with no fma contraction).  The bidirectional call is compared
bitwise with two estimate_flow calls: the kernels are deterministic and every
stage the two directions share treats the two frames' planes alike."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def fb_numpy(fw, bw, alpha1=0.01, alpha2=0.5):
    """of_fb_consistency in numpy float64: (state uint8, err float32)."""
    fw = np.asarray(fw, dtype=np.float32)
    bw = np.asarray(bw, dtype=np.float32)
    H, W = fw.shape[:2]
    ii, jj = np.mgrid[0:H, 0:W]
    u = fw[..., 0].astype(np.float64)
    v = fw[..., 1].astype(np.float64)
    B = bw.astype(np.float64)
    with np.errstate(all="ignore"):
        q = jj.astype(np.float64) + u
        r = ii.astype(np.float64) + v
        inside = (q >= 0) & (q <= W - 1) & (r >= 0) & (r <= H - 1)
        q = np.where(inside, q, 0.0)
        r = np.where(inside, r, 0.0)
        qf, rf = np.floor(q), np.floor(r)
        j0, i0 = qf.astype(np.int64), rf.astype(np.int64)
        fc, fr = q - qf, r - rf
        j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
        b = []
        for k in range(2):
            b.append((1.0 - fr) * ((1.0 - fc) * B[i0, j0, k] + fc * B[i0, j1, k])
                     + fr * ((1.0 - fc) * B[i1, j0, k] + fc * B[i1, j1, k]))
        bu, bv = b
        du, dv = u + bu, v + bv
        err = du * du + dv * dv
        thr = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2
        state = np.where(inside, (err > thr).astype(np.uint8), np.uint8(2)).astype(np.uint8)
        err = np.where(inside, err, np.inf).astype(np.float32)
    return state, err


def planted_flows(H, W):
    """Seeded flows in +-6 px (some targets leave the frame) with the edge
    cases planted in fw: an exact integer displacement, -0.0, a target exactly
    on column W-1 and row H-1, one NaN and one Inf component."""
    rng = np.random.default_rng(1000 * H + W)
    fw = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    bw = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    n = H * W
    pix = lambda k: divmod(k, W)  # noqa: E731
    i, j = pix(n - 1)  # -0.0: the last pixel maps onto itself, i1 / j1 clamped, weight 0
    fw[i, j] = (-0.0, -0.0)
    bw[i, j] = (0.5, -0.5)  # err 0.5: state 0 with the defaults (thr 0.505), 1 with (0, 0.25)
    if n >= 5:
        fw[0, 0] = (min(1, W - 1), min(1, H - 1))  # integer displacement
        i, j = pix(n // 2)
        fw[i, j] = (W - 1 - j, H - 1 - i)  # exactly the last column and row
        i, j = pix(1)
        fw[i, j, 0] = np.nan
        i, j = pix(n - 2)
        fw[i, j, 1] = np.inf
    return fw, bw


SHAPES = [(1, 1), (1, 7), (5, 1), (37, 53), (3, 130), (64, 65)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_check_kernel_bitwise_vs_numpy(H, W):
    from optical_flow import forward_backward_check
    fw, bw = planted_flows(H, W)
    ref_s, ref_e = fb_numpy(fw, bw)
    s, e = forward_backward_check(fw, bw, return_error=True)
    assert s.dtype == np.uint8 and e.dtype == np.float32 and s.shape == (H, W) and e.shape == (H, W)
    assert np.array_equal(s, ref_s) and np.array_equal(e, ref_e)
    # the planted entries
    n = H * W
    assert s[H - 1, W - 1] == 0 and e[H - 1, W - 1] == 0.5
    if n >= 5:
        assert s[0, 0] != 2
        i, j = divmod(n // 2, W)
        assert s[i, j] != 2 and np.isfinite(e[i, j])
        for k in (1, n - 2):
            i, j = divmod(k, W)
            assert s[i, j] == 2 and e[i, j] == np.inf
    if n > 1000:
        assert all((s == k).any() for k in (0, 1, 2))
    # other thresholds
    ref_s2, ref_e2 = fb_numpy(fw, bw, 0.0, 0.25)
    s2, e2 = forward_backward_check(fw, bw, 0.0, 0.25, return_error=True)
    assert np.array_equal(s2, ref_s2) and np.array_equal(e2, ref_e2)
    assert s2[H - 1, W - 1] == 1
    # err = NULL
    s3 = forward_backward_check(fw, bw)
    assert np.array_equal(s3, ref_s)
    # the backward mask is the same kernel with the roles swapped
    fwc = np.nan_to_num(fw, nan=0.0, posinf=0.0)
    sb, eb = forward_backward_check(bw, fwc, return_error=True)
    rb = fb_numpy(bw, fwc)
    assert np.array_equal(sb, rb[0]) and np.array_equal(eb, rb[1])


def test_check_analytic():
    from optical_flow import forward_backward_check
    H, W = 20, 30
    fw = np.empty((H, W, 2))
    fw[..., 0], fw[..., 1] = 2.0, -1.0
    bw = -fw
    s, e = forward_backward_check(fw, bw, return_error=True)
    ii, jj = np.mgrid[0:H, 0:W]
    inside = (jj + 2 <= W - 1) & (ii - 1 >= 0)
    assert np.array_equal(s, np.where(inside, 0, 2))
    assert np.all(e[inside] == 0.0) and np.all(e[~inside] == np.inf)
    bw[..., 1] = 3.0  # |fw + bw|^2 = 4 > 0.01 * (5 + 13) + 0.5
    s = forward_backward_check(fw, bw)
    assert np.array_equal(s, np.where(inside, 1, 2))


def _gray(im):
    return np.floor(im.mean(axis=2) + 0.5)


_CASES = [
    ("rgb48", "classic+nl-fast", None),
    ("rgb48", "classic-c", {"solver": "pcg"}),
    ("rgb48", "hs-brightness", None),
    ("gray48", "classic+nl-fast", None),
    ("rgb45", "classic+nl-fast", None),
]


@pytest.fixture(scope="module")
def pairs():
    from optical_flow.utils.synthetic import synth_pair
    a, b, _ = synth_pair(48, 64, seed=3)
    c, d, _ = synth_pair(45, 67, seed=5)
    return {"rgb48": (a, b), "gray48": (_gray(a), _gray(b)), "rgb45": (c, d)}


@pytest.mark.parametrize("inp,method,params", _CASES)
def test_bidirectional_equals_two_calls_bitwise(pairs, inp, method, params):
    import optical_flow
    im1, im2 = pairs[inp]
    fw = optical_flow.estimate_flow(im1, im2, method, params)
    bw = optical_flow.estimate_flow(im2, im1, method, params)
    r = optical_flow.estimate_flow_bidirectional(im1, im2, method, params)
    assert r.forward.dtype == np.float64 and r.forward.shape == im1.shape[:2] + (2,)
    assert r.occ_forward.dtype == np.uint8 and r.occ_forward.shape == im1.shape[:2]
    dfw, dbw = np.abs(r.forward - fw).max(), np.abs(r.backward - bw).max()
    print(f"{inp} {method}: max |forward - one call| {dfw:.3e}, max |backward - one call| {dbw:.3e}")
    assert np.array_equal(r.forward, fw)
    assert np.array_equal(r.backward, bw)
    assert np.array_equal(r.occ_forward, optical_flow.forward_backward_check(fw, bw))
    assert np.array_equal(r.occ_backward, optical_flow.forward_backward_check(bw, fw))
    # other thresholds reach the kernel
    r2 = optical_flow.estimate_flow_bidirectional(im1, im2, method, params, alpha1=0.0, alpha2=1e-4)
    assert np.array_equal(r2.forward, fw)
    assert np.array_equal(r2.occ_forward, optical_flow.forward_backward_check(fw, bw, 0.0, 1e-4))


@pytest.mark.parametrize("nch,method", [(2, "hs-brightness"), (1, "classic+nl-fast")])
def test_one_and_two_channel_frames_take_the_compute_flow_route(pairs, nch, method):
    """(H, W, 1) and (H, W, 2) frames go through compute_flow as in
    estimate_flow (the weighted median takes a 1- or 3-channel guide only, so
    the 2-channel case runs a method without one)."""
    import optical_flow
    a, b = pairs["rgb48"]
    im1, im2 = a[:, :, :nch], b[:, :, :nch]
    r = optical_flow.estimate_flow_bidirectional(im1, im2, method)
    fw = optical_flow.estimate_flow(im1, im2, method)
    bw = optical_flow.estimate_flow(im2, im1, method)
    assert np.array_equal(r.forward, fw) and np.array_equal(r.backward, bw)
    assert np.array_equal(r.occ_backward, optical_flow.forward_backward_check(bw, fw))


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


def test_preprocessing_is_shared(pairs):
    import optical_flow
    im1, im2 = pairs["rgb48"]
    one = _launch_counts(lambda: optical_flow.estimate_flow(im1, im2, "classic+nl-fast"))
    both = _launch_counts(lambda: optical_flow.estimate_flow_bidirectional(im1, im2, "classic+nl-fast"))
    assert one["rof_iters"] > 0 and one["wmf"] > 0
    assert both["rof_iters"] == one["rof_iters"]
    assert both["wmf"] == 2 * one["wmf"]
    assert both["fb_check"] == 1 and "fb_check" not in one


def test_mask_separates_the_error_on_rubberwhale(rubberwhale):
    import optical_flow
    im1, im2, gt = rubberwhale
    r = optical_flow.estimate_flow_bidirectional(im1, im2, "classic+nl-fast")
    known = (np.abs(gt[..., 0]) < 1e9) & (np.abs(gt[..., 1]) < 1e9)
    epe = np.sqrt(((r.forward - gt) ** 2).sum(-1))
    s = r.occ_forward
    all_, ok, bad = epe[known].mean(), epe[known & (s == 0)].mean(), epe[known & (s == 1)].mean()
    share = [(s == k).mean() for k in (0, 1, 2)]
    print(f"RubberWhale: AEPE all {all_:.5f}, consistent {ok:.5f} ({100 * share[0]:.2f} %), "
          f"inconsistent {bad:.4f} ({100 * share[1]:.2f} %), out of frame {100 * share[2]:.2f} %")
    assert share[0] >= 0.95
    assert ok < all_ < bad


def test_refusals(pairs):
    import optical_flow
    from optical_flow import _native
    im1, im2 = pairs["rgb48"]
    fw = np.zeros((6, 7, 2))
    for a1 in (-0.01, float("nan")):
        with pytest.raises(ValueError):
            optical_flow.forward_backward_check(fw, fw, alpha1=a1)
        with pytest.raises(ValueError):
            optical_flow.estimate_flow_bidirectional(im1, im2, alpha1=a1)
    with pytest.raises(ValueError):
        optical_flow.forward_backward_check(fw, fw, alpha2=float("inf"))
    # while a pair stream is open on the context
    with optical_flow.PairStream(48, 64, 3, "classic+nl-fast", lanes=1) as ps:
        ctx = ps._ctx
        f = _native.f32(np.zeros((2, 6, 7)))
        st = np.empty((6, 7), np.uint8)
        with pytest.raises(ValueError, match="pair stream is open"):
            ctx.check(ctx.lib.of_fb_consistency(ctx.handle, _native.ptr(f), _native.ptr(f), 6, 7, 0.01, 0.5,
                                                _native.u8ptr(st), None))
        P = optical_flow.load_of_method("classic+nl-fast").to_params()
        a, b = _native.f32(im1), _native.f32(im2)
        out = np.empty((2, 2, 48, 64), np.float32)
        with pytest.raises(ValueError, match="pair stream is open"):
            ctx.check(ctx.lib.of_estimate_flow_bidir(ctx.handle, C.byref(P), _native.ptr(a), _native.ptr(b), 48, 64, 3,
                                                     None, None, _native.ptr(out[0]), _native.ptr(out[1]), 0.01, 0.5,
                                                     None, None, None, None))
