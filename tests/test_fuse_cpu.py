"""Temporal denoising: what can be checked without a GPU -- the Python surface,
the argument checks, and the numpy restatement (tests/fuse_numpy.py) on
hand-made cases and on the two-layer scene it was prototyped on."""
import numpy as np
import pytest

import fuse_numpy as fn


def test_package_exports_temporal_api():
    import optical_flow
    from optical_flow import temporal
    for name in ("compose_flows", "fuse_frames", "TemporalDenoiser", "denoise_frames"):
        assert getattr(optical_flow, name) is getattr(temporal, name)
        assert name in optical_flow.__all__


def test_c_abi_mirror_declares_the_six_entries():
    import ctypes
    from optical_flow import _abi, _native
    want = {"of_flow_compose": 9, "of_fuse_frames": 12, "of_denoise_open": 6, "of_denoise_push": 5,
            "of_denoise_flush": 4, "of_denoise_close": 1}
    for name, n in want.items():
        assert len(_native._SIGS[name][0]) == n, name
    O = _abi.OfFuseOpts
    assert ctypes.sizeof(O) == 40
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [
        ("radius", 0), ("patch", 4), ("sigma", 8), ("strength", 16), ("alpha1", 24), ("alpha2", 32)]
    u8p, fp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)
    assert _native._SIGS["of_flow_compose"][0][5:] == [u8p, u8p, fp, u8p]
    assert _native._SIGS["of_fuse_frames"][0][8:10] == [u8p, ctypes.POINTER(O)]
    assert _native._SIGS["of_denoise_push"][0][4] == ctypes.POINTER(ctypes.c_int32)
    assert _abi.OF_ABI_VERSION == 3


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
    dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=None),
    dict(sigma="x"), dict(patch=4), dict(patch=-1), dict(patch=1.0), dict(strength=0.0), dict(strength=float("nan")),
    dict(neighbours=[], flows=[]), dict(neighbours=[IM] * 9, flows=[Z] * 9),
    dict(center=np.zeros((8, 9, 5)), neighbours=[np.zeros((8, 9, 5))]), dict(center=np.zeros(8)),
    dict(center=np.zeros((0, 9)), neighbours=[np.zeros((0, 9))], flows=[np.zeros((0, 9, 2))]),
    dict(neighbours=[np.zeros((8, 10))]), dict(neighbours=[np.zeros((8, 9, 1))]), dict(flows=[Z, Z]),
    dict(flows=[np.zeros((8, 10, 2))]), dict(flows=[np.zeros((8, 9, 3))]), dict(flows=[np.zeros((8, 9))]),
    dict(states=[np.zeros((8, 10), np.uint8)]), dict(states=[np.zeros((8, 9))]), dict(states=[None, None]),
    dict(states=[np.full((8, 9), 256)])])
def test_fuse_frames_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(center=IM, neighbours=[IM], flows=[Z], sigma=5.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.fuse_frames(**a)


def test_fuse_frames_missing_sigma_raises_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError, match="sigma"):
        optical_flow.fuse_frames(IM, [IM], [Z])
    with pytest.raises(ValueError, match="sigma"):
        optical_flow.TemporalDenoiser((8, 9))
    with pytest.raises(ValueError, match="sigma"):
        optical_flow.denoise_frames([IM, IM])


@pytest.mark.parametrize("kw", [
    dict(f=np.zeros((8, 9))), dict(f=np.zeros((8, 9, 3))), dict(g=np.zeros((8, 10, 2))),
    dict(f=np.zeros((8, 9, 2), dtype=complex)), dict(f=np.zeros((0, 9, 2)), g=np.zeros((0, 9, 2))),
    dict(state_f=np.zeros((8, 10), np.uint8)), dict(state_g=np.zeros((8, 9))), dict(state_g=np.full((8, 9), -1))])
def test_compose_flows_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(f=Z, g=Z)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.compose_flows(**a)


@pytest.mark.parametrize("kw", [
    dict(shape=(8,)), dict(shape=(8, 9, 2)), dict(shape=(8, 9, 5)), dict(shape=(8, 9, 1)), dict(shape=(0, 9)),
    dict(method="nonexistent_method"), dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=-2.0), dict(radius=0),
    dict(radius=3), dict(radius=1.0), dict(radius=True), dict(patch=4), dict(strength=-1.0), dict(alpha1=-0.5),
    dict(alpha2=float("inf"))])
def test_temporal_denoiser_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(shape=(8, 9), sigma=5.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.TemporalDenoiser(**a)
    if "shape" not in kw:
        b = dict(sigma=5.0)
        b.update(kw)
        with pytest.raises(ValueError):
            optical_flow.denoise_frames([IM, IM], **b)


def test_denoise_frames_bad_frames_raise_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.denoise_frames([], sigma=5.0)
    with pytest.raises(ValueError):
        optical_flow.denoise_frames([np.zeros((8, 9)), np.zeros((8, 10))], sigma=5.0)
    with pytest.raises(ValueError):
        optical_flow.denoise_frames([np.zeros((8, 9, 5))], sigma=5.0)


# ---- the restatement on hand-made cases ------------------------------------
def shifted_frames(H, W, C, shifts, seed):
    """A random canvas seen through windows moved by integer (dx, dy): frame k
    shows at (i, j) what the centre frame shows at (i - dy, j - dx)."""
    rng = np.random.default_rng(seed)
    canvas = rng.uniform(0, 255, (H + 16, W + 16) + ((C,) if C > 1 else ())).astype(np.float32)
    return [canvas[8 - dy:8 - dy + H, 8 - dx:8 - dx + W].copy() for dx, dy in shifts]


@pytest.mark.parametrize("C", [1, 3])
def test_integer_flows_and_large_sigma_give_the_in_order_mean(C):
    H, W = 12, 17
    shifts = [(0, 0), (2, 1), (-1, 2), (3, -2)]
    rng = np.random.default_rng(3)
    clean = shifted_frames(H, W, C, shifts, 4)
    fr = [(f + rng.normal(0, 10, f.shape)).astype(np.float32) for f in clean]
    flows = [np.zeros((H, W, 2)) + np.array([dx, dy], float) for dx, dy in shifts[1:]]
    out, wgt = fn.fuse(fr[0], fr[1:], flows, sigma=1e4, patch=2)
    ii, jj = np.mgrid[0:H, 0:W]
    acc = fr[0].astype(np.float64)
    cnt = np.ones((H, W))
    for (dx, dy), f in zip(shifts[1:], fr[1:]):
        ok = (ii + dy >= 0) & (ii + dy <= H - 1) & (jj + dx >= 0) & (jj + dx <= W - 1)
        al = f.astype(np.float64)[np.clip(ii + dy, 0, H - 1), np.clip(jj + dx, 0, W - 1)]
        okc = ok if C == 1 else ok[..., None]
        acc = np.where(okc, acc + al, acc)
        cnt = cnt + ok
    want = (acc / (cnt if C == 1 else cnt[..., None])).astype(np.float32)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(wgt, cnt.astype(np.float32))
    inner = (slice(3, H - 3), slice(3, W - 3))
    assert np.all(wgt[inner] == 4.0)  # n + 1 wherever every neighbour is in the frame
    assert out.dtype == np.float32 and out.shape == fr[0].shape and wgt.dtype == np.float32


def test_masked_nonfinite_and_out_of_frame_neighbours_count_for_nothing():
    H, W = 10, 12
    rng = np.random.default_rng(5)
    I = rng.uniform(0, 255, (H, W)).astype(np.float32)
    N = rng.uniform(0, 255, (H, W)).astype(np.float32)
    N2 = I.copy()
    flow = np.zeros((H, W, 2), np.float32)
    state = np.zeros((H, W), np.uint8)
    state[2, 3] = 1
    state[2, 4] = 2
    flow[5, 5, 0] = np.nan
    flow[5, 6, 1] = np.inf
    flow[7, 2] = (-3.0, 0.0)   # lands at column -1
    flow[7, 9, 1] = 1e30
    bad = [(2, 3), (2, 4), (5, 5), (5, 6), (7, 2), (7, 9)]
    (vis, _, w), = fn.weights(I, [N2], [flow], 5.0, [state], patch=1)
    for p in bad:
        assert not vis[p] and w[p] == 0.0
    assert vis.sum() == H * W - len(bad)
    out, wgt = fn.fuse(I, [N2], [flow], 5.0, [state], patch=1)
    for p in bad:
        assert wgt[p] == 1.0 and out[p] == I[p]
    assert np.all(wgt[vis] == 2.0)  # identical frames elsewhere: full weight
    # ... and they are left out of their neighbours' window counts: plant a large difference at
    # the masked pixels only; every visible pixel still has weight exactly 1
    N3 = I.copy()
    for p in bad:
        N3[p] += 200.0
    (vis3, _, w3), = fn.weights(I, [N3], [flow], 5.0, [state], patch=1)
    assert np.all(w3[vis3] == 1.0)
    # with the mask dropped, the window around (2, 3) sees the difference
    (_, _, w4), = fn.weights(I, [N3], [flow], 5.0, None, patch=1)
    assert w4[2, 3] < 1.0 and w4[1, 2] < 1.0 and w4[7, 2] == 0.0
    # a random neighbour is rejected outright (mean squared difference ~ 10^4 >> 2 s^2 + h2 = 450)
    (_, _, w5), = fn.weights(I, [N], [np.zeros((H, W, 2))], 5.0, None, patch=2)
    assert np.all(w5 == 0.0)


def test_weight_is_exactly_one_then_falls_to_exactly_zero_at_h2():
    H, W = 6, 7
    I = np.zeros((H, W), np.float32)
    z = np.zeros((H, W, 2))
    # sigma 2, strength 4: two_s2 = 8, h2 = 64; a constant difference `diff` gives d = diff^2
    for diff, want in ((2.0, 1.0), (2.5, 1.0), (6.0, (1.0 - 28.0 / 64.0) ** 2), (8.5, 0.0), (100.0, 0.0)):
        for patch in (0, 2):
            N = np.full((H, W), diff, np.float32)
            (vis, _, w), = fn.weights(I, [N], [z], 2.0, None, 4.0, patch=patch)
            assert vis.all() and np.all(w == want), (diff, w[0, 0], want)
    # sigma 2, strength 0.5: h2 = 1; diff 3 gives e = 9 - 8 = 1 = h2 exactly
    (_, _, w), = fn.weights(I, [np.full((H, W), 3.0, np.float32)], [z], 2.0, None, 0.5, patch=1)
    assert np.all(w == 0.0)
    (_, _, w), = fn.weights(I, [np.full((H, W), 2.875, np.float32)], [z], 2.0, None, 0.5, patch=1)
    assert np.all((w > 0.0) & (w < 1.0))  # e = 0.265625, just inside


def test_compose_restatement():
    H, W = 9, 11
    f = np.zeros((H, W, 2), np.float32)
    f[..., 0] = 2.0
    g = np.zeros((H, W, 2), np.float32)
    g[..., 1] = 1.5
    sf = np.zeros((H, W), np.uint8)
    sg = np.zeros((H, W), np.uint8)
    sf[1, 1] = 1
    sg[4, 6] = 2   # reached from (4, 4)
    sg[5, 6] = 1
    sf[5, 4] = 1
    f[3, 3, 1] = np.nan
    out, st = fn.compose(f, g, sf, sg)
    assert np.all(st[:, W - 2:] == 2) and np.all(out[:, W - 2:] == f[:, W - 2:])
    assert st[1, 1] == 1 and st[4, 4] == 2 and st[5, 4] == 1 and st[3, 3] == 2 and st[0, 0] == 0
    assert np.isnan(out[3, 3, 1]) and out[3, 3, 0] == 2.0
    np.testing.assert_array_equal(out[0, 0], [2.0, 1.5])
    out0, st0 = fn.compose(f, np.zeros_like(g))
    np.testing.assert_array_equal(out0.view(np.uint32), f.view(np.uint32))
    assert np.array_equal(st0 == 2, ~fn._landing(f)[4])


# ---- the prototype scene -----------------------------------------------------
def tex(s, y, x):
    return 128 + 60 * np.sin(0.37 * x + 0.21 * y + s) * np.cos(0.29 * y - 0.17 * x + 2 * s)


def layer_scene(k, speed=4.0):
    """Frame k of a 40 x 64 two-layer scene: static background tex(1), a
    foreground tex(5) rectangle moving `speed` px in +x per frame.  Returns
    (frame, foreground mask)."""
    H, W = 40, 64
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = speed * k
    fg = (xx - d >= 12) & (xx - d <= 31) & (yy >= 10) & (yy <= 29)
    return np.where(fg, tex(5, yy, xx - d), tex(1, yy, xx)), fg


def exact_flow_and_mask(k_from, k_to, speed=4.0):
    """The exact flow frame k_from -> k_to of layer_scene and its exact
    visibility mask (0: the pixel's surface is seen in frame k_to, 1: covered
    there, 2: it leaves the frame)."""
    _, fg0 = layer_scene(k_from, speed)
    _, fg1 = layer_scene(k_to, speed)
    H, W = fg0.shape
    d = speed * (k_to - k_from)
    flow = np.zeros((H, W, 2))
    flow[fg0, 0] = d
    state = np.zeros((H, W), np.uint8)
    state[~fg0 & fg1] = 1  # background covered by the foreground in the other frame
    jj = np.mgrid[0:H, 0:W][1]
    state[fg0 & ((jj + d < 0) | (jj + d > W - 1))] = 2
    return flow, state


def test_two_layer_scene_beats_the_input_and_the_plain_mean():
    """sigma = 10, radius 1, patch 2, strength 4, exact flows and masks.
    Measured: noisy input MSE 96.73 (28.28 dB), plain 3-frame mean 113.49
    (27.58 dB), fused 32.87 (32.96 dB); ideal sigma^2 / 3 = 33.33 (32.90 dB);
    zero flows and no masks 46.30 (31.48 dB)."""
    sigma = 10.0
    rng = np.random.default_rng(2024)
    clean = [layer_scene(k)[0] for k in range(3)]
    noisy = [(c + rng.normal(0, sigma, c.shape)).astype(np.float32) for c in clean]
    f_prev, s_prev = exact_flow_and_mask(1, 0)
    f_next, s_next = exact_flow_and_mask(1, 2)
    out, wgt = fn.fuse(noisy[1], [noisy[0], noisy[2]], [f_prev, f_next], sigma, [s_prev, s_next])
    mse = lambda a: float(((np.asarray(a, np.float64) - clean[1]) ** 2).mean())  # noqa: E731
    m_in, m_mean, m_out = mse(noisy[1]), mse(np.mean([n.astype(np.float64) for n in noisy], 0)), mse(out)
    psnr = lambda m: 10 * np.log10(255.0 ** 2 / m)  # noqa: E731
    print(f"MSE noisy {m_in:.2f} ({psnr(m_in):.2f} dB), plain mean {m_mean:.2f} ({psnr(m_mean):.2f} dB), "
          f"fused {m_out:.2f} ({psnr(m_out):.2f} dB); ideal {sigma ** 2 / 3:.2f} ({psnr(sigma ** 2 / 3):.2f} dB); "
          f"mean weight {wgt.mean():.3f}")
    assert m_out < m_in
    assert m_out < m_mean
    assert m_out <= 1.5 * sigma ** 2 / 3
    # wrong (zero) flows and no masks: the photometric rejection alone keeps the output at or above the input
    z = np.zeros((40, 64, 2))
    out0, _ = fn.fuse(noisy[1], [noisy[0], noisy[2]], [z, z], sigma)
    print(f"zero flows, no masks: MSE {mse(out0):.2f} ({psnr(mse(out0)):.2f} dB)")
    assert mse(out0) <= m_in
