"""Noise-level estimation: what can be checked without a GPU -- the Python
surface, the argument checks, the C ABI mirror, the lower-median rule of the
numpy restatement (tests/noise_numpy.py) and the restatement's accuracy on the
scenes the estimators were prototyped on, with flows from the CPU oracle."""
import ctypes

import numpy as np
import pytest

import noise_numpy as nn


def test_package_exports_noise_api():
    import optical_flow
    from optical_flow import noise
    for name in ("estimate_noise", "NoiseEstimate"):
        assert getattr(optical_flow, name) is getattr(noise, name)
        assert name in optical_flow.__all__
    assert optical_flow.NoiseEstimate._fields == ("sigma", "per_channel", "used")


def test_c_abi_mirror_declares_the_noise_entries():
    from optical_flow import _abi, _native
    E = _abi.OfNoiseEstimate
    assert ctypes.sizeof(E) == 48
    assert [(f, getattr(E, f).offset) for f, _ in E._fields_] == [("sigma", 0), ("sigma_c", 8), ("n", 40)]
    fp, u8p, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
    i, vp = ctypes.c_int, ctypes.c_void_p
    S = _native._SIGS
    assert S["of_estimate_noise_pair"] == ([vp, fp, fp, i, i, i, fp, u8p, ctypes.POINTER(E)], i)
    assert S["of_estimate_noise"] == ([vp, fp, i, i, i, ctypes.POINTER(E)], i)
    assert S["of_denoise_open_auto"] == ([vp, ctypes.POINTER(_abi.OfParams), i, i, i,
                                          ctypes.POINTER(_abi.OfFuseOpts), ctypes.c_double], i)
    assert S["of_denoise_last_sigma"] == ([vp, dp], i)
    # what the automatic mode leaves alone
    assert S["of_denoise_open"] == ([vp, ctypes.POINTER(_abi.OfParams), i, i, i, ctypes.POINTER(_abi.OfFuseOpts)], i)
    assert ctypes.sizeof(_abi.OfFuseOpts) == 40 and _abi.OF_ABI_VERSION == 3


def test_struct_layout_matches_the_header():
    import os
    import subprocess
    import tempfile
    from conftest import ROOT
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n",'
           'sizeof(of_noise_estimate), offsetof(of_noise_estimate, sigma_c), offsetof(of_noise_estimate, n),'
           'sizeof(of_fuse_opts));}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [48, 8, 40, 40]


@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


IM = np.zeros((8, 9))
Z = np.zeros((8, 9, 2))


@pytest.mark.parametrize("kw", [
    dict(im=np.zeros(8)), dict(im=np.zeros((8, 9, 5))), dict(im=np.zeros((0, 9))), dict(im=np.zeros((8, 9, 0))),
    dict(im=np.zeros((8, 9), dtype=complex)), dict(im=np.zeros((2, 2, 2, 2))), dict(im=np.zeros((1, 7))),
    dict(im=np.zeros((7, 1, 3))), dict(im2=IM), dict(flow=Z), dict(state=np.zeros((8, 9), np.uint8)),
    dict(im2=np.zeros((8, 10)), flow=Z), dict(im2=np.zeros((8, 9, 1)), flow=Z), dict(im2=IM, flow=np.zeros((8, 9))),
    dict(im2=IM, flow=np.zeros((8, 10, 2))), dict(im2=IM, flow=np.zeros((8, 9, 3))),
    dict(im2=IM, flow=Z, state=np.zeros((8, 10), np.uint8)), dict(im2=IM, flow=Z, state=np.zeros((8, 9))),
    dict(im2=IM, flow=Z, state=np.full((8, 9), 256))])
def test_estimate_noise_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(im=IM)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.estimate_noise(**a)


@pytest.mark.parametrize("kw", [
    dict(sigma=None), dict(sigma="Auto"), dict(sigma="automatic"), dict(sigma=""), dict(sigma=b"auto"),
    dict(sigma="auto", noise_floor=0.0), dict(sigma="auto", noise_floor=-1.0),
    dict(sigma="auto", noise_floor=float("nan")), dict(sigma="auto", noise_floor=float("inf")),
    dict(sigma="auto", noise_floor=None), dict(sigma="auto", noise_floor="auto"), dict(sigma="auto", radius=3),
    dict(sigma="auto", patch=4), dict(sigma="auto", strength=0.0), dict(sigma="auto", alpha1=-1.0),
    dict(sigma="auto", shape=(8, 9, 2)), dict(sigma="auto", method="nonexistent_method")])
def test_auto_sigma_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(shape=(8, 9))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.TemporalDenoiser(**a)
    if "shape" not in kw:
        with pytest.raises(ValueError):
            optical_flow.denoise_frames([IM, IM], **kw)


def test_fuse_frames_keeps_its_required_number(no_library):
    import optical_flow
    with pytest.raises(ValueError, match="sigma"):
        optical_flow.fuse_frames(IM, [IM], [Z], sigma="auto")


# ---- the restatement ---------------------------------------------------------
def test_lower_median_rule_against_partition():
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 5, 8, 9, 100, 101, 4096, 4097):
        k = (rng.normal(0, 3, n) ** 2).astype(np.float32)
        if n > 4:
            k[rng.integers(0, n, n // 3)] = k[0]  # duplicates
        if n > 8:
            k[1], k[2] = np.inf, 0.0
        r = (n - 1) // 2
        want = np.partition(k, r)[r]
        got = nn.lower_median(k)
        assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), n
        # lower: for even n the smaller of the two middle keys, never their mean
        s = np.sort(k)
        assert got == s[r] and (n % 2 or got == s[n // 2 - 1])
    assert nn.lower_median(np.array([4.0, 1.0], np.float32)) == 1.0
    assert nn.lower_median(np.array([np.inf, np.inf, 1.0], np.float32)) == np.inf


def test_hand_made_keys():
    # integer flow: g = 2; half-pixel flow in x: g = 1.5; in both: g = 1.25
    H, W = 4, 6
    a = np.zeros((H, W), np.float32)
    b = np.full((H, W), 3.0, np.float32)
    for (u, v), g in (((1.0, 0.0), 2.0), ((0.5, 0.0), 1.5), ((0.5, 0.5), 1.25), ((-0.0, -0.0), 2.0)):
        f = np.zeros((H, W, 2), np.float32)
        f[..., 0], f[..., 1] = u, v
        k = nn.pair_keys(a, b, f)
        assert k.dtype == np.float32 and k.shape[1] == 1 and np.all(k == np.float32(9.0 / g)), (u, v, k[:3])
        inside = (np.arange(W) + u <= W - 1).sum() * (np.arange(H) + v <= H - 1).sum()
        assert k.shape[0] == inside
    # states, non-finite flows and values
    f = np.zeros((H, W, 2), np.float32)
    st = np.zeros((H, W), np.uint8)
    st[0, 0], st[0, 1] = 1, 2
    f[1, 0, 0], f[1, 1, 1], f[1, 2, 0] = np.nan, np.inf, 1e30
    f[2, 0, 0] = W - 1  # lands exactly on the last column: inside
    f[2, 1, 0] = W - 1  # one past it: outside
    b2 = b.copy()
    b2[3, 3] = np.nan
    a2 = a.copy()
    a2[3, 4] = np.inf
    # out: the two states, the three non-finite flows, the one outside, the Inf of frame 1 and the four pixels
    # with the NaN of frame 2 among their taps, (2, 2), (2, 3), (3, 2), (3, 3), at whatever weight
    assert nn.pair_keys(a2, b2, f, st).shape[0] == H * W - 11
    assert nn.estimate_pair(a, b, f, np.ones((H, W), np.uint8)).used == 0
    e = nn.estimate_pair(a, b, f * np.nan)
    assert e.used == 0 and np.isnan(e.sigma) and np.isnan(e.per_channel[0])
    # single frame: x in the top-left of every block gives key (float)(x^2 / 4); odd edges left out
    im = np.zeros((5, 7), np.float32)
    im[0:4:2, 0:6:2] = 6.0
    im[4, :], im[:, 6] = 1e6, -1e6
    k = nn.single_keys(im)
    assert k.shape == (6, 1) and np.all(k == 9.0)
    e = nn.estimate_single(np.stack([im, 2 * im], -1))
    assert e.used == 6 and e.per_channel == (3.0 / nn.MAD_TO_SIGMA, 6.0 / nn.MAD_TO_SIGMA)
    assert e.sigma == np.sqrt((e.per_channel[0] ** 2 + e.per_channel[1] ** 2) / 2)
    im[1, 1] = np.nan
    assert nn.single_keys(im).shape == (5, 1)
    assert nn.estimate_single(np.full((2, 2), 3e38)).sigma == 0.0
    big = np.zeros((2, 2), np.float32)
    big[0, 0], big[0, 1] = 3e38, -3e38  # d = 3e38: d * d rounds to +Inf and stays in
    assert nn.estimate_single(big).sigma == np.inf


def test_session_rule():
    E = nn.Estimate
    H, W = 10, 10
    est = [E(3.0, (3.0,), 100), E(50.0, (50.0,), 24), E(4.0, (4.0,), 25)]  # pair 1: a cut, 24 < 100 / 4
    single = lambda t: E(7.0 + t, (7.0 + t,), 25)  # noqa: E731
    sig = [nn.session_sigma(t, 4, H, W, est, single, 0.25) for t in range(4)]
    assert sig == [np.sqrt(9.0 / 1), np.sqrt(9.0 / 1), np.sqrt(16.0 / 1), np.sqrt(16.0 / 1)]
    est[0] = E(3.0, (3.0,), 0)
    assert nn.session_sigma(0, 4, H, W, est, single, 0.25) == 7.0      # no qualifying pair: the single frame
    assert nn.session_sigma(1, 4, H, W, est, single, 0.25) == 8.0
    est[0], est[1] = E(3.0, (3.0,), 100), E(4.0, (4.0,), 100)
    assert nn.session_sigma(1, 4, H, W, est, single, 0.25) == np.sqrt((9.0 + 16.0) / 2)
    assert nn.session_sigma(0, 1, H, W, [], single, 0.25) == 7.0       # a clip of one frame
    assert nn.session_sigma(0, 1, 1, 9, [], single, 0.25) == 0.25      # no 2 x 2 block: the floor
    assert nn.session_sigma(0, 1, H, W, [], lambda t: E(0.0, (0.0,), 25), 0.25) == 0.25
    assert nn.session_sigma(0, 1, H, W, [], lambda t: E(float("nan"), (float("nan"),), 0), 0.25) == 0.25


# ---- accuracy on the prototype scenes ----------------------------------------
# Where the margins come from: the MAD's sampling error is about 1.16 / sqrt(n), roughly 1 % for the canvas
# scene's 11 900 samples and 2.2 % for the tex scene's 2 800, more in fact, since neighbouring residuals share
# bilinear taps; 8 % and 10 % leave about three standard deviations.
def noisy_pair(frames, sigma):
    rng = np.random.default_rng(5)
    return [f + rng.normal(0, sigma, f.shape) for f in frames]  # frame 1 first


def oracle_flows(a, b):
    import oracle
    fw = oracle.estimate_flow(a, b, "classic+nl-fast")
    bw = oracle.estimate_flow(b, a, "classic+nl-fast")
    return fw, nn.fb_state(fw, bw, 0.01, 0.5)


def constant_flow(H, W, u, v):
    f = np.zeros((H, W, 2))
    f[..., 0], f[..., 1] = u, v
    return f


def canvas_scene():
    from test_gpu_fuse import clip_frames
    return clip_frames(96, 128, 1, 2, 41, 0.0)  # moving (2, -1) px per frame


def tex_scene(H, W, u, v):
    from test_gpu_interp import tex
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return [tex(1, yy - v * t, xx - u * t) for t in range(2)]


def test_canvas_scene_true_flow():
    """Measured (sigma: single frame / pair along the true flow):
    2: 4.27 / 2.04, 5: 6.71 / 5.09, 10: 10.93 / 10.18, 20: 20.46 / 20.36."""
    clean = canvas_scene()
    flow = constant_flow(96, 128, 2.0, -1.0)
    for sigma in (2.0, 5.0, 10.0, 20.0):
        a, b = noisy_pair(clean, sigma)
        pair, single = nn.estimate_pair(a, b, flow), nn.estimate_single(a)
        print(f"canvas 96x128, sigma {sigma:g}: single frame {single.sigma:.2f}, pair along the true flow "
              f"{pair.sigma:.2f} (n = {pair.used})")
        assert pair.used == 95 * 126
        assert abs(pair.sigma - sigma) <= 0.08 * sigma


@pytest.mark.parametrize("sigma", [2.0, 20.0])
def test_canvas_scene_estimated_flow(sigma):
    """The two ends of the range (a pair of oracle flows at 96 x 128 takes about
    ten seconds).  Measured with the estimated flows, sigma 2 / 5 / 10 / 20:
    2.04 / 5.06 / 10.16 / 20.14 (n = 11 890 .. 11 901); single frame 4.27 /
    6.71 / 10.93 / 20.46."""
    a, b = noisy_pair(canvas_scene(), sigma)
    fw, st = oracle_flows(a, b)
    pair, single = nn.estimate_pair(a, b, fw, st), nn.estimate_single(a)
    print(f"canvas 96x128, sigma {sigma:g}: single frame {single.sigma:.2f}, pair along the estimated flow "
          f"{pair.sigma:.2f} (n = {pair.used})")
    assert abs(pair.sigma - sigma) <= 0.08 * sigma
    if sigma == 2.0:
        assert abs(pair.sigma - 2.0) < abs(single.sigma - 2.0)


@pytest.mark.parametrize("sigma", [5.0, 10.0, 20.0])
def test_tex_scene(sigma):
    """Measured, sigma 5 / 10 / 20: estimated flow 5.24 / 10.01 / 19.54, true
    flow 5.14 / 10.28 / 20.56, single frame 5.26 / 10.30 / 20.43 (sigma 2: 2.07
    / 2.06 / 2.39)."""
    a, b = noisy_pair(tex_scene(48, 64, 4.0, -2.0), sigma)
    fw, st = oracle_flows(a, b)
    est, true = nn.estimate_pair(a, b, fw, st), nn.estimate_pair(a, b, constant_flow(48, 64, 4.0, -2.0))
    print(f"tex 48x64, sigma {sigma:g}: single frame {nn.estimate_single(a).sigma:.2f}, pair along the estimated "
          f"flow {est.sigma:.2f} (n = {est.used}), along the true flow {true.sigma:.2f} (n = {true.used})")
    assert abs(est.sigma - sigma) <= 0.10 * sigma
    assert abs(true.sigma - sigma) <= 0.10 * sigma


def test_low_sigma_bias_reads_high():
    """tex at 96 x 128 moving (1.3, -0.7), sigma 2, along the true flow: 2.18.
    The bilinear sample interpolates the picture too; that error is independent
    of the noise and adds to the residual's variance, so below the picture's
    interpolation error the estimate is high, never low."""
    a, b = noisy_pair(tex_scene(96, 128, 1.3, -0.7), 2.0)
    e = nn.estimate_pair(a, b, constant_flow(96, 128, 1.3, -0.7))
    print(f"tex 96x128 moving (1.3, -0.7), sigma 2: pair along the true flow {e.sigma:.2f} (n = {e.used})")
    assert e.sigma > 2.0
    # the signal's share alone: the same frames without noise
    c = tex_scene(96, 128, 1.3, -0.7)
    e0 = nn.estimate_pair(c[0], c[1], constant_flow(96, 128, 1.3, -0.7))
    print(f"  ... and without noise {e0.sigma:.2f}")
    assert 0.0 < e0.sigma < e.sigma


def test_rubberwhale_true_flow(rubberwhale):
    """The committed RubberWhale pair along its ground-truth flow.  Measured:
    untouched 1.04 pooled over R, G, B (0.96 / 0.98 / 1.17; single frame 1.76);
    with added noise of sigma 5 / 10 / 20: 5.26 / 10.17 / 20.11 (single frame
    5.60 / 10.39 / 20.19).  n is about 222 000, a sampling error of 0.25 %; the
    pair's own noise of about 1 adds in quadrature (sqrt(26.1) = 5.11 at sigma
    5), so 10 % holds with room."""
    im1, im2, gt = rubberwhale
    e, s = nn.estimate_pair(im1, im2, gt), nn.estimate_single(im1)
    print(f"RubberWhale untouched: pair {e.sigma:.2f} per channel {np.round(e.per_channel, 2)} (n = {e.used}), "
          f"single frame {s.sigma:.2f}")
    assert e.sigma < s.sigma
    for sigma in (5.0, 10.0, 20.0):
        a, b = noisy_pair([im1, im2], sigma)
        e, s = nn.estimate_pair(a, b, gt), nn.estimate_single(a)
        print(f"RubberWhale + sigma {sigma:g}: pair {e.sigma:.2f}, single frame {s.sigma:.2f}")
        assert abs(e.sigma - sigma) <= 0.10 * sigma
