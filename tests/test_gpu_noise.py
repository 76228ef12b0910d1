"""Noise-level estimation on the GPU: of_estimate_noise_pair and
of_estimate_noise bitwise against the numpy float64 restatement
(tests/noise_numpy.py), the exact selection on planted key distributions
against np.partition, the denoiser's automatic sigma bitwise against its parts
run by hand, its other cases, its lifecycle and an end-to-end run."""
import ctypes as C

import numpy as np
import pytest

import fuse_numpy as fn
import noise_numpy as nn

pytestmark = pytest.mark.gpu

# 1 x 1: one sample; 2 x 2: one block; 3 x 5: the odd row and column left out; 9 x 65 crosses a workgroup seam of
# the key kernels (256 pixels, 1-D) inside a row; 67 x 131: no multiple of anything, 35 workgroups, 2145 blocks
SHAPES = [(1, 1), (2, 2), (3, 5), (1, 7), (9, 65), (67, 131)]


def same(a, b):
    """Equal as float64 values, NaN equal to NaN."""
    a, b = np.float64(a), np.float64(b)
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def assert_estimate(got, want, what):
    assert got.used == want.used, (what, got, want)
    assert len(got.per_channel) == len(want.per_channel), what
    assert same(got.sigma, want.sigma), (what, got, want)
    for g, w in zip(got.per_channel, want.per_channel):
        assert same(g, w), (what, got, want)


def frames_for(H, W, Cc, seed):
    rng = np.random.default_rng(seed)
    shp = (H, W) if Cc == 1 else (H, W, Cc)
    a = rng.uniform(0, 255, shp).astype(np.float32)
    b = (a + rng.normal(0, 5, shp)).astype(np.float32)
    return a, b, rng


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_pair_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    from test_gpu_fuse import plant
    a, b, rng = frames_for(H, W, Cc, 100 * H + W + Cc)
    flows = {"short": plant(rng.uniform(-0.6, 0.6, (H, W, 2)).astype(np.float32)),
             "long": plant(rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)),
             "zero": np.zeros((H, W, 2), np.float32)}
    whole = np.zeros((H, W, 2), np.float32)  # integer displacements, every row landing exactly on column W - 1
    whole[..., 0] = W - 1 - np.arange(W)
    flows["to the last column"] = whole
    state = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    if H * W > 100:  # non-finite values in both frames
        a[1, 2], b[2, 3] = np.inf, np.nan
        b[H - 1, W - 1] = -np.inf
    used = []
    for name, f in flows.items():
        for st in (None, state):
            want = nn.estimate_pair(a, b, f, st)
            got = optical_flow.estimate_noise(a, b, f, st)
            assert isinstance(got, optical_flow.NoiseEstimate) and isinstance(got.used, int)
            assert_estimate(got, want, (name, st is None))
            used.append(got.used)
    last = nn.estimate_pair(a, b, flows["to the last column"]).used  # column W - 1 is inside
    assert last == H * W if H * W <= 100 else last >= (H - 3) * W
    if H * W == 1:
        assert used[0] == 1 and np.isfinite(optical_flow.estimate_noise(a, b, flows["short"]).sigma)
    if H * W > 100:
        assert 0 < min(used) < max(used) < H * W
    # an all-masked field, and one that lands nowhere
    for f, st in ((flows["zero"], np.full((H, W), 1, np.uint8)), (flows["zero"], np.full((H, W), 2, np.uint8)),
                  (np.full((H, W, 2), 1e30, np.float32), None), (np.full((H, W, 2), np.nan, np.float32), None)):
        got = optical_flow.estimate_noise(a, b, f, st)
        assert got.used == 0 and np.isnan(got.sigma) and all(np.isnan(x) for x in got.per_channel)
        assert len(got.per_channel) == Cc


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_single_bitwise_vs_numpy(H, W, Cc):
    import optical_flow
    a, _, rng = frames_for(H, W, Cc, 300 * H + W + Cc)
    if H < 2 or W < 2:
        from optical_flow import _abi, _native
        with pytest.raises(ValueError):
            optical_flow.estimate_noise(a)
        ctx = _native.context()
        est = _abi.OfNoiseEstimate()
        rc = ctx.lib.of_estimate_noise(ctx.handle, _native.ptr(_native.f32(a)), H, W, Cc, C.byref(est))
        assert rc == _abi.OF_EINVAL
        with pytest.raises(ValueError, match="H and W >= 2"):
            ctx.check(rc)
        return
    smooth = (a * np.float32(0.01) + np.float32(100)).astype(np.float32)  # small details: other bins
    for name, im in (("uniform", a), ("smooth", smooth)):
        want = nn.estimate_single(im)
        got = optical_flow.estimate_noise(im)
        assert_estimate(got, want, name)
        assert got.used == (H // 2) * (W // 2)
    if H * W > 100:
        a[0, 0], a[H - 1 - H % 2, W - 1 - W % 2], a[3, 4] = np.nan, np.inf, -np.inf
        want = nn.estimate_single(a)
        assert want.used == (H // 2) * (W // 2) - 3
        assert_estimate(optical_flow.estimate_noise(a), want, "non-finite")
    got = optical_flow.estimate_noise(np.full(a.shape, np.nan))
    assert got.used == 0 and np.isnan(got.sigma) and len(got.per_channel) == Cc


def test_other_channel_counts_and_integer_frames():
    import optical_flow
    rng = np.random.default_rng(4)
    for Cc in (2, 4):
        a = rng.integers(0, 256, (21, 34, Cc)).astype(np.uint8)
        b = rng.integers(0, 256, (21, 34, Cc)).astype(np.uint8)
        f = rng.uniform(-2, 2, (21, 34, 2))
        assert_estimate(optical_flow.estimate_noise(a, b, f), nn.estimate_pair(a, b, f), Cc)
        assert_estimate(optical_flow.estimate_noise(a), nn.estimate_single(a), Cc)


# ---- the selection, through the single-frame entry ---------------------------
def planted(x):
    """An image whose 2 x 2 blocks hold x (Hb, Wb[, C]) in their top-left and
    0 elsewhere, one odd row and column of junk added: key (float)(x^2 / 4)."""
    x = np.asarray(x, dtype=np.float32)
    Hb, Wb = x.shape[:2]
    im = np.zeros((2 * Hb + 1, 2 * Wb + 1) + x.shape[2:], np.float32)
    im[0:2 * Hb:2, 0:2 * Wb:2] = x
    im[2 * Hb], im[:, 2 * Wb] = 1e6, -1e6
    return im


def x_for_keys(k):
    """x whose key (float)(x^2 / 4) is k, or within an ulp or two of it."""
    return (2.0 * np.sqrt(np.asarray(k, dtype=np.float64))).astype(np.float32)


def check_selection(x, what):
    """The entry on planted(x) against np.partition of the restatement's keys,
    bit for bit; returns the keys (n, C)."""
    import optical_flow
    im = planted(x)
    keys = nn.single_keys(im)
    n, Cc = keys.shape
    assert n == x.shape[0] * x.shape[1]
    r = (n - 1) // 2
    with np.errstate(over="ignore"):
        want_c = [np.sqrt(np.float64(np.partition(keys[:, c], r)[r])) / 0.6744897501960817 for c in range(Cc)]
        want = np.sqrt(sum(w * w for w in want_c) / Cc)
    got = optical_flow.estimate_noise(im)
    assert got.used == n, what
    for c in range(Cc):
        assert same(got.per_channel[c], want_c[c]), (what, c, got, want_c)
    assert same(got.sigma, want), (what, got, want)
    return keys


@pytest.mark.parametrize("Hb,Wb", [(2, 2), (3, 3), (16, 33), (17, 33)])  # n = 4, 9, 528, 561: even and odd
def test_selection_on_planted_keys(Hb, Wb):
    n = Hb * Wb
    rng = np.random.default_rng(n)
    shape = lambda v: np.asarray(v, dtype=np.float32).reshape(Hb, Wb)  # noqa: E731
    # all keys equal
    k = check_selection(shape(np.full(n, 6.0)), "equal")
    assert np.all(k == 9.0)
    # one top bin, spread over the lowest 10 bits: targets 100 .. 900 ulps into a 1024-ulp window
    base = np.float32(1000.0).view(np.uint32) & np.uint32(0xfffffc00)
    tgt = (base + rng.integers(100, 900, n).astype(np.uint32)).view(np.float32)
    k = check_selection(shape(x_for_keys(tgt)), "low bits")
    kb = k[:, 0].view(np.uint32)
    assert np.all(kb >> 10 == kb[0] >> 10) and np.unique(kb).size > min(n, 200) // 2
    # keys equal except one, below and above
    for odd in (1.0, 50.0):
        x = np.full(n, 6.0)
        x[rng.integers(0, n)] = odd
        check_selection(shape(x), ("one other", odd))
    # duplicates of the median straddling the rank: a third below, a third equal, a third above, shuffled
    x = np.concatenate([np.full(n // 3, 2.0), np.full(n - 2 * (n // 3), 4.0), np.full(n // 3, 8.0)])
    k = check_selection(shape(rng.permutation(x)), "straddling")
    # a zero key: the median itself, then one among larger keys
    x = rng.permutation(np.concatenate([np.zeros(n // 2 + 1), np.full(n - n // 2 - 1, 3.0)]))
    k = check_selection(shape(x), "zero median")
    assert np.sort(k[:, 0])[(n - 1) // 2] == 0.0
    x = np.abs(rng.normal(0, 8, n)) + 0.5
    x[0] = 0.0
    check_selection(shape(x), "a zero")
    # +Inf keys stay in: above the median, then the median itself
    x = np.abs(rng.normal(0, 8, n)) + 0.5
    x[n - 1] = 3e38
    k = check_selection(shape(x), "an inf")
    assert np.isinf(k).sum() == 1
    if n > 4:
        x[:n // 2 + 2] = 3e38
        k = check_selection(shape(rng.permutation(x)), "inf median")
        assert np.sort(k[:, 0])[(n - 1) // 2] == np.inf
    # wide: keys over many orders of magnitude, denormals included; three channels of their own
    x = np.stack([np.exp(rng.uniform(-60, 40, n)), np.abs(rng.normal(0, 1e-3, n)), rng.integers(0, 4, n) * 1.0], -1)
    check_selection(np.asarray(x, np.float32).reshape(Hb, Wb, 3), "wide")


# ---- the session equals its parts --------------------------------------------
FLOOR = 0.25


def bidir_pairs(frames):
    import optical_flow
    pairs = []
    for a, b in zip(frames[:-1], frames[1:]):
        r = optical_flow.estimate_flow_bidirectional(a, b, "classic+nl-fast")
        pairs.append((r.forward, r.backward, r.occ_forward, r.occ_backward))
    return pairs


def rule_sigmas(frames, pairs, floor=FLOOR):
    """The automatic session's sigma of every frame from the package's parts,
    and the pairs' estimates."""
    import optical_flow
    H, W = frames[0].shape[:2]
    est = [optical_flow.estimate_noise(a, b, p[0], p[2]) for a, b, p in zip(frames[:-1], frames[1:], pairs)]
    sig = [nn.session_sigma(t, len(frames), H, W, est, lambda s: optical_flow.estimate_noise(frames[s]), floor)
           for t in range(len(frames))]
    return sig, est


def run_auto(frames, radius=1, floor=FLOOR):
    """(sigma, frame, weight) per frame index from a TemporalDenoiser(sigma='auto')."""
    import optical_flow
    got = {}
    with optical_flow.TemporalDenoiser(frames[0].shape, "classic+nl-fast", sigma="auto", radius=radius,
                                       noise_floor=floor) as dn:
        assert dn.last_sigma is None
        for f in frames:
            r = dn.push(f)
            if r is not None:
                got[r[0]] = (dn.last_sigma, r[1], dn.last_weight)
        for r in dn.flush():
            got[r[0]] = (dn.last_sigma, r[1], dn.last_weight)
    assert sorted(got) == list(range(len(frames)))
    return [got[t] for t in range(len(frames))]


def fused_by_hand(frames, pairs, t, sigma, radius):
    import optical_flow
    return fn.session(
        frames, pairs, sigma, radius, 4.0, 2,
        compose_fn=lambda f, g, a, b: optical_flow.compose_flows(f, g, a, b, return_state=True),
        fuse_fn=lambda c, nb, fl, s, st, strength, patch: optical_flow.fuse_frames(c, nb, fl, s, st, strength, patch,
                                                                                   return_weight=True))[t]


@pytest.fixture(scope="module")
def clips():
    """Per channel count: the fusion test's 6-frame 48 x 64 clip, the flows and
    masks of its adjacent pairs and the rule's sigmas, computed once."""
    from test_gpu_fuse import clip_frames
    out = {}
    for Cc in (1, 3):
        frames = clip_frames(48, 64, Cc, 6, 40 + Cc, 6.0)
        pairs = bidir_pairs(frames)
        out[Cc] = (frames, pairs) + rule_sigmas(frames, pairs)
    return out


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("Cc", [1, 3])
def test_auto_session_equals_its_parts(clips, Cc, radius):
    """Bitwise, not accuracy: the clip's noise is sigma 6 and the frames read
    5.90 .. 6.16 for C = 1 but 6.61 .. 6.74 for C = 3, where the flow comes
    from the gray mix of three independent canvases and is off by 0.16 px in
    the median (0.06 for C = 1): a flow error in the bulk of the pixels, times
    the picture's gradient, counts as noise.  Along the true flow the first
    pair reads 6.22 and 6.09 (the restatement, on the CPU oracle's flows)."""
    import optical_flow
    frames, pairs, sig, est = clips[Cc]
    assert all(4 * e.used >= 48 * 64 for e in est)  # every pair of this clip qualifies
    got = run_auto(frames, radius)
    print(f"C={Cc} radius={radius}: true sigma 6, pairs {np.round([e.sigma for e in est], 3)}, "
          f"frames {np.round([g[0] for g in got], 3)}")
    for t, (s, o, w) in enumerate(got):
        assert s == sig[t], (t, s, sig[t])
        want_o, want_w = fused_by_hand(frames, pairs, t, s, radius)
        assert np.array_equal(o, want_o), (t, np.abs(o - want_o).max())
        assert np.array_equal(w, want_w), t
    # the same through denoise_frames
    all_o, all_w, all_s = optical_flow.denoise_frames(frames, "classic+nl-fast", sigma="auto", radius=radius,
                                                      return_weight=True, return_sigma=True)
    assert all_s.shape == (6,) and all_s.dtype == np.float64 and list(all_s) == sig
    for t in range(6):
        assert np.array_equal(all_o[t], got[t][1]) and np.array_equal(all_w[t], got[t][2])
    only_o, only_s = optical_flow.denoise_frames(frames, "classic+nl-fast", sigma="auto", radius=radius,
                                                 return_sigma=True)
    assert np.array_equal(only_o, all_o) and np.array_equal(only_s, all_s)
    assert np.array_equal(optical_flow.denoise_frames(frames, "classic+nl-fast", sigma="auto", radius=radius), all_o)


def test_fixed_sigma_reports_itself(clips):
    import optical_flow
    frames = clips[1][0][:3]
    with optical_flow.TemporalDenoiser(frames[0].shape, sigma=7.5) as dn:
        assert dn.push(frames[0]) is None and dn.last_sigma is None
        assert dn.push(frames[1]) is not None and dn.last_sigma == 7.5
    out, sig = optical_flow.denoise_frames(frames, sigma=7.5, return_sigma=True)
    assert list(sig) == [7.5] * 3 and np.array_equal(out, optical_flow.denoise_frames(frames, sigma=7.5))


def test_single_frame_clip_falls_back_to_the_single_frame_estimate():
    import optical_flow
    f = np.random.default_rng(3).uniform(0, 255, (20, 30, 3))
    (s, o, w), = run_auto([f], radius=2)
    assert s == optical_flow.estimate_noise(f).sigma and s > FLOOR
    assert np.array_equal(o, f.astype(np.float32).astype(np.float64)) and np.all(w == 1.0)
    # no 2 x 2 block: the floor
    (s, o, w), = run_auto([f[:1]], floor=1.5)
    assert s == 1.5 and np.array_equal(o, f[:1].astype(np.float32).astype(np.float64))


def cut_clip():
    """Two frames of the fusion test's canvas, then two of an unrelated fine
    texture moving 1 px per frame; noise of sigma 3.  On the CPU oracle's flows
    the pairs keep 2880 / 429 / 2979 consistent pixels of 3072."""
    from test_gpu_fuse import clip_frames
    from test_gpu_interp import tex
    H, W = 48, 64
    A = clip_frames(H, W, 1, 2, 41, 3.0)
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return [A[0], A[1]] + [tex(5, 3 * yy, 3 * (xx - t)) + rng.normal(0, 3, (H, W)) for t in range(2)]


def test_a_cut_does_not_set_the_level():
    import optical_flow
    frames = cut_clip()
    pairs = bidir_pairs(frames)
    sig, est = rule_sigmas(frames, pairs)
    print(f"cut clip: pairs' sigma {np.round([e.sigma for e in est], 2)} on {[e.used for e in est]} of 3072 pixels; "
          f"frames' sigma {np.round(sig, 3)}")
    assert 4 * est[1].used < 48 * 64 <= 4 * min(est[0].used, est[2].used)  # what the scene is for
    assert est[1].sigma > 5 * max(est[0].sigma, est[2].sigma)
    got = run_auto(frames)
    assert [g[0] for g in got] == sig
    # frames 1 and 2 border the cut and take their other pair alone
    assert sig[1] == np.sqrt(est[0].sigma * est[0].sigma / 1) and sig[2] == np.sqrt(est[2].sigma * est[2].sigma / 1)
    for t in (1, 2):
        want_o, want_w = fused_by_hand(frames, pairs, t, sig[t], 1)
        assert np.array_equal(got[t][1], want_o) and np.array_equal(got[t][2], want_w)
    # the cut alone: both frames fall back to their single-frame estimates
    two = frames[1:3]
    got2 = run_auto(two)
    assert [g[0] for g in got2] == [optical_flow.estimate_noise(f).sigma for f in two]
    assert all(g[0] < est[1].sigma / 3 for g in got2)


def test_a_constant_clip_is_fused_at_the_floor():
    frames = [np.full((16, 24, 3), 100.0)] * 3
    for floor in (FLOOR, 2.0):
        got = run_auto(frames, floor=floor)
        for s, o, w in got:
            assert s == floor and np.array_equal(o, frames[0])


# ---- end to end ----------------------------------------------------------------
def test_end_to_end_auto_on_the_noisy_translating_clip():
    """The fusion test's end-to-end scene (five 48 x 64 frames of the
    interpolation test's texture moving (4, -2) px per frame, sigma = 10, seed
    99, the middle frame, 8 px border left out) with sigma='auto'."""
    import optical_flow
    from test_gpu_interp import tex
    H, W, sigma = 48, 64, 10.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    clean = [tex(1, yy + 2.0 * t, xx - 4.0 * t) for t in range(5)]
    rng = np.random.default_rng(99)
    noisy = [c + rng.normal(0, sigma, c.shape) for c in clean]
    out, sig = optical_flow.denoise_frames(noisy, "classic+nl-fast", sigma="auto", radius=1, return_sigma=True)
    fixed = optical_flow.denoise_frames(noisy, "classic+nl-fast", sigma=sigma, radius=1)
    m = (slice(8, H - 8), slice(8, W - 8))
    mse = lambda a: float(((a - clean[2]) ** 2)[m].mean())  # noqa: E731
    e_out, e_fixed, e_in, e_mean = mse(out[2]), mse(fixed[2]), mse(noisy[2]), mse(np.mean(noisy[1:4], 0))
    print(f"48x64 translating clip, sigma 10: estimated per frame {np.round(sig, 3)}; interior MSE: noisy {e_in:.2f}, "
          f"uncompensated 3-frame mean {e_mean:.2f}, sigma='auto' {e_out:.2f}, sigma=10 {e_fixed:.2f}")
    assert out.shape == (5, H, W) and sig.shape == (5,)
    assert np.all(np.abs(sig - sigma) <= 0.10 * sigma), sig
    assert e_out < e_in
    assert e_out < e_mean


# ---- lifecycle -----------------------------------------------------------------
def test_lifecycle_of_the_new_entries():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    rng = np.random.default_rng(12)
    frames = [rng.uniform(0, 255, (H, W)) for _ in range(3)]
    f0 = _native.f32(frames[0])
    z = _native.f32(np.zeros((2, H, W)))
    est = _abi.OfNoiseEstimate()
    sigma = C.c_double(-1.0)
    P = optical_flow.load_of_method("classic+nl-fast").to_params()

    def opts(**kw):
        a = dict(radius=1, patch=2, sigma=8.0, strength=4.0, alpha1=0.01, alpha2=0.5)
        a.update(kw)
        return _abi.OfFuseOpts(*[a[k] for k in ("radius", "patch", "sigma", "strength", "alpha1", "alpha2")])

    def pair(Cc=1, HH=H, WW=W, a=f0, b=f0, f=z, out=est):
        return lib.of_estimate_noise_pair(h, _native.ptr(a), _native.ptr(b), HH, WW, Cc, _native.ptr(f), None,
                                          C.byref(out) if out is not None else None)

    def single(Cc=1, HH=H, WW=W, a=f0, out=est):
        return lib.of_estimate_noise(h, _native.ptr(a), HH, WW, Cc, C.byref(out) if out is not None else None)

    # the estimators refuse what the fusion's stage entries refuse
    for kw in (dict(Cc=0), dict(Cc=5), dict(HH=0), dict(WW=-1), dict(a=None), dict(out=None)):
        for call in (pair, single):
            with pytest.raises(ValueError):
                ctx.check(call(**kw))
    for kw in (dict(b=None), dict(f=None)):
        with pytest.raises(ValueError):
            ctx.check(pair(**kw))
    for call in (pair, single):
        with pytest.raises(NotImplementedError):
            ctx.check(call(HH=46341, WW=46341))
    with pytest.raises(ValueError):
        ctx.check(single(HH=1, WW=H * W))
    ctx.check(pair())
    assert est.n == H * W and est.sigma == 0.0 and np.isnan(est.sigma_c[1])
    ctx.check(single())
    assert est.n == H * W // 4 and est.sigma > 0

    # no session: last_sigma refuses like push, flush and close
    rc = lib.of_denoise_last_sigma(h, C.byref(sigma))
    assert rc == _abi.OF_EINVAL
    with pytest.raises(ValueError, match="no temporal denoiser"):
        ctx.check(rc)
    # of_denoise_open_auto: the floor and every option but sigma are checked, nothing is left open
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="floor"):
            ctx.check(lib.of_denoise_open_auto(h, C.byref(P), H, W, 1, C.byref(opts()), floor))
    for kw in (dict(radius=0), dict(radius=3), dict(patch=-1), dict(patch=4), dict(strength=float("inf")),
               dict(strength=0.0), dict(alpha1=-1.0), dict(alpha2=float("nan"))):
        with pytest.raises(ValueError):
            ctx.check(lib.of_denoise_open_auto(h, C.byref(P), H, W, 1, C.byref(opts(**kw)), 0.25))
    with pytest.raises(ValueError):
        ctx.check(lib.of_denoise_open_auto(h, C.byref(P), H, W, 2, C.byref(opts()), 0.25))
    with pytest.raises(ValueError):
        ctx.check(lib.of_denoise_open_auto(h, C.byref(P), H, W, 1, None, 0.25))
    with pytest.raises(ValueError):
        ctx.check(lib.of_denoise_open_auto(h, None, H, W, 1, C.byref(opts()), 0.25))
    assert lib.of_denoise_close(h) == _abi.OF_EINVAL
    # ... and sigma is not read, while of_denoise_open still refuses it
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(ValueError):
            ctx.check(lib.of_denoise_open(h, C.byref(P), H, W, 1, C.byref(opts(sigma=bad))))
        ctx.check(lib.of_denoise_open_auto(h, C.byref(P), H, W, 1, C.byref(opts(sigma=bad)), 0.25))
        ctx.check(lib.of_denoise_close(h))

    # the automatic session holds what the fixed one holds; one denoiser per context, of either kind
    base = optical_flow.denoise_frames(frames, sigma="auto")  # also grows the arena to what these pairs need
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    out = np.empty((H, W), np.float32)
    idx = C.c_int32(0)
    with optical_flow.TemporalDenoiser((H, W), sigma="auto") as dn:
        pitch = (W + 63) // 64 * 64
        held = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
        assert held - b0 == 3 * H * W * 4 + 2 * (2 * H * pitch * 8 + 2 * H * W)
        for kind in (dict(sigma="auto"), dict(sigma=8.0)):
            with pytest.raises(ValueError, match="denoiser is open"):
                optical_flow.TemporalDenoiser((H, W), **kind)
        assert lib.of_denoise_last_sigma(h, C.byref(sigma)) == _abi.OF_EINVAL  # nothing emitted yet
        assert dn.push(frames[0]) is None
        rc = lib.of_denoise_last_sigma(h, C.byref(sigma))
        assert rc == _abi.OF_EINVAL and sigma.value == -1.0
        with pytest.raises(ValueError, match="not emitted"):
            ctx.check(rc)
        assert lib.of_denoise_last_sigma(h, None) == _abi.OF_EINVAL
        r = dn.push(frames[1])
        assert r[0] == 0 and lib.of_denoise_last_sigma(h, C.byref(sigma)) == _abi.OF_OK
        assert sigma.value == dn.last_sigma > 0.25
        assert np.array_equal(r[1], base[0])
        assert lib.of_denoise_last_sigma(h, None) == _abi.OF_EINVAL
        dn.push(frames[2])
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == held  # the keys are arena memory, already there
        got = dict(dn.flush())
        assert np.array_equal(got[2], base[2])
        with pytest.raises(ValueError, match="flushed"):
            dn.push(frames[0])
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    assert lib.of_denoise_last_sigma(h, C.byref(sigma)) == _abi.OF_EINVAL
    # refused while a pair stream is open on the context
    with optical_flow.PairStream(H, W, 1, "classic+nl-fast", lanes=1) as ps:
        with pytest.raises(ValueError, match="pair stream is open"):
            optical_flow.TemporalDenoiser((H, W), sigma="auto", context=ps._ctx)
        rc = ps._ctx.lib.of_estimate_noise(ps._ctx.handle, _native.ptr(f0), H, W, 1, C.byref(est))
        assert rc == _abi.OF_EINVAL
