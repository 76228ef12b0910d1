"""Gradient-domain blending on the GPU: of_poisson_solve and of_inpaint_blend
bitwise against the numpy float64 restatement (tests/poisson_numpy.py), the
session with blending bitwise against blend_fill on the flows it used, its
lifecycle, and the quality gates of the CPU tests with estimated flows."""
import ctypes as C

import numpy as np
import pytest

import inpaint_numpy as ip
import poisson_numpy as pn
from test_gpu_inpaint import clip_frames, fill_case, make_masks
from test_poisson_cpu import quality_gates

pytestmark = pytest.mark.gpu

# odd sizes, level seams (30 x 30 is the largest single-level frame) and tile seams (32-cell tiles, 64-wide rows)
SHAPES = [(1, 1), (1, 7), (9, 1), (2, 2), (37, 53), (48, 65), (40, 129)]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def holes(H, W, rng):
    """name -> (unknown, excluded or None)"""
    z = lambda: np.zeros((H, W), bool)  # noqa: E731
    out = {}
    m = z()
    m[H // 2, W // 2] = True
    out["single pixel"] = (m, None)
    m = z()
    m[H // 3, :] = True
    m[:, W // 3] = True
    out["one-pixel lines across the frame"] = (m, None)
    ii, jj = np.mgrid[0:H, 0:W]
    out["checkerboard"] = (((ii + jj) & 1) == 0, None)
    m = z()
    m[0:max(H // 2, 1), 0:max(W // 3, 1)] = True
    m[H - 1, :] = True
    out["corner and border"] = (m, None)
    out["all unknown"] = (~z(), None)
    out["none"] = (z(), None)
    m, e = z(), z()
    m[H // 2, W // 2] = True
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        if 0 <= H // 2 + di < H and 0 <= W // 2 + dj < W:
            e[H // 2 + di, W // 2 + dj] = True
    m[0, W - 1] = m[0, W - 1] or not e[0, W - 1]
    out["isolated by excluded pixels"] = (m, e)
    m = rng.uniform(size=(H, W)) < 0.5
    m[H // 4:H // 4 + H // 2 + 1, W // 4:W // 4 + W // 2 + 1] = True
    out["blob with random rim and excluded pixels"] = (m, (rng.uniform(size=(H, W)) < 0.15) & ~m)
    return out


def check_poisson(v, unknown, excluded, s, h, key, **opts):
    import optical_flow
    lab = np.where(unknown, pn.UNKNOWN, pn.FIXED).astype(np.uint8)
    if excluded is not None:
        lab[excluded] = pn.EXCLUDED
    chan = (lambda a: a[None]) if v.ndim == 2 else (lambda a: np.moveaxis(a, 2, 0))
    back = (lambda a: a[0]) if v.ndim == 2 else (lambda a: np.moveaxis(a, 0, 2))
    want = back(pn.solve(lab, chan(v).astype(np.float64), None if s is None else chan(s).astype(np.float64), h,
                         cycles=opts.get("cycles", pn.CYCLES), sweeps=opts.get("sweeps", pn.SWEEPS),
                         coarse=opts.get("coarse_sweeps", pn.COARSE)))
    got = optical_flow.poisson_fill(v, unknown, s, h, excluded, **opts)
    assert got.dtype == np.float64 and got.shape == v.shape, key
    assert np.isfinite(got).all(), key
    bad = np.argwhere(bits64(got) != bits64(want))
    assert bad.size == 0, (key, bad[:5], np.abs(got - want).max())
    keep = lab != pn.UNKNOWN
    assert np.array_equal(bits64(got[keep]), bits64(v[keep].astype(np.float64))), key
    return got


@pytest.mark.parametrize("H,W", SHAPES)
def test_poisson_fill_bitwise_vs_numpy(H, W):
    rng = np.random.default_rng(100 * H + W)
    for k, (name, (unknown, excluded)) in enumerate(holes(H, W, rng).items()):
        Cc = (1, 3, 4)[k % 3]
        shp = (H, W) if Cc == 1 else (H, W, Cc)
        v = rng.uniform(0, 255, shp).astype(np.float32)
        s = rng.uniform(0, 255, shp).astype(np.float32)
        h = rng.uniform(size=(H, W)) < 0.8
        got = check_poisson(v, unknown, excluded, None, None, (name, Cc, "membrane"))
        check_poisson(v, unknown, excluded, s, h, (name, Cc, "guided"))
        if name == "none":
            assert np.array_equal(bits64(got), bits64(v.astype(np.float64)))
        if name == "isolated by excluded pixels" and H >= 3 and W >= 3:
            assert got[H // 2, W // 2].tolist() == v[H // 2, W // 2].astype(np.float64).tolist()  # deg 0


@pytest.mark.parametrize("H,W", [(2, 2), (37, 53), (40, 129)])
def test_poisson_fill_options_at_their_ends(H, W):
    rng = np.random.default_rng(H + W)
    unknown, excluded = holes(H, W, rng)["blob with random rim and excluded pixels"]
    v = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    s = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    h = rng.uniform(size=(H, W)) < 0.8
    for opts in (dict(cycles=1, sweeps=1, coarse_sweeps=1), dict(cycles=64), dict(sweeps=1, coarse_sweeps=64),
                 dict(cycles=2, sweeps=2, coarse_sweeps=7)):
        check_poisson(v, unknown, excluded, s, h, opts, **opts)
    # 2 channels, float64 and integer inputs, bool and integer masks
    v2 = rng.uniform(0, 255, (H, W, 2)).astype(np.float32)
    a = check_poisson(v2, unknown, excluded, None, None, "two channels")
    import optical_flow
    b = optical_flow.poisson_fill(v2.astype(np.float64), unknown.astype(np.int32) * 5, excluded=excluded.astype(np.uint8))
    assert np.array_equal(bits64(a), bits64(b))


def test_the_c_entries_check_for_themselves():
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, hd = ctx.lib, ctx.handle
    H, W = 8, 9
    lab = np.zeros((H, W), np.uint8)
    lab[3, 4] = 1
    v = _native.f32(np.ones((H, W)))
    out = np.empty((H, W), np.float64)
    ok = _abi.OfBlendOpts(8, 2, 32, 0)

    def solve(o=ok, lab=lab, v=v, s=None, h=None, HH=H, WW=W, Cc=1, dst=out):
        return lib.of_poisson_solve(hd, _native.u8ptr(lab), _native.ptr(v), _native.ptr(s), _native.u8ptr(h), HH, WW, Cc,
                                    C.byref(o) if o is not None else None, _native.dptr(dst))

    for bad in ((0, 2, 32), (65, 2, 32), (8, 0, 32), (8, 3, 32), (8, 2, 0), (8, 2, 65)):
        with pytest.raises(ValueError):
            ctx.check(solve(_abi.OfBlendOpts(*bad, 0)))
    three = lab.copy()
    three[0, 0] = 3
    for kw in (dict(o=None), dict(lab=None), dict(v=None), dict(dst=None), dict(s=v), dict(h=lab), dict(Cc=0),
               dict(Cc=5), dict(HH=0), dict(lab=three)):
        with pytest.raises(ValueError):
            ctx.check(solve(**kw))
    with pytest.raises(NotImplementedError):
        ctx.check(solve(HH=46341, WW=46341))
    ctx.check(solve())
    assert out[3, 4] == 1.0 and (out == 1.0).all()
    # of_inpaint_blend: both option structs are checked
    fr = _native.f32(np.zeros((2, H, W)))
    mk = np.zeros((2, H, W), np.uint8)
    z = _native.f32(np.zeros((1, 2, H, W)))
    o32 = np.empty((H, W), np.float32)

    def blend(io, bo):
        return lib.of_inpaint_blend(hd, _native.ptr(fr), _native.u8ptr(mk), _native.ptr(z), _native.ptr(z), 2, H, W, 1,
                                    0, C.byref(io), C.byref(bo) if bo is not None else None, _native.ptr(o32), None)

    good = _abi.OfInpaintOpts(2, 1, 3, 0)
    for io, bo in ((good, None), (good, _abi.OfBlendOpts(0, 2, 32, 0)), (_abi.OfInpaintOpts(0, 1, 3, 0), ok),
                   (_abi.OfInpaintOpts(2, 9, 3, 0), ok)):
        with pytest.raises(ValueError):
            ctx.check(blend(io, bo))
    ctx.check(blend(good, ok))
    ctx.check(blend(_abi.OfInpaintOpts(2, 8, 3, 0), ok))  # grow 8: the fill's masks are grown by 9


# ---- the blended fill ---------------------------------------------------------
def check_blend(frames, masks, fw, bw, t, radius, grow, key, **opts):
    import optical_flow
    want, want_st = pn.blend(frames, masks, fw, bw, t, radius, grow, cycles=opts.get("cycles", pn.CYCLES),
                             sweeps=opts.get("sweeps", pn.SWEEPS), coarse=opts.get("coarse_sweeps", pn.COARSE))
    got, st = optical_flow.blend_fill(frames, masks, fw, bw, t, radius, grow, return_status=True, **opts)
    assert got.dtype == np.float64 and got.shape == frames[0].shape and st.dtype == np.uint8, key
    bad = np.argwhere(st != want_st)
    assert bad.size == 0, (key, bad[:5])
    bad = np.argwhere(bits32(got) != bits32(want))
    assert bad.size == 0, (key, bad[:5])
    Om = ip.grow(masks[t], grow) != 0
    assert not (st == ip.UNFILLED).any() and np.array_equal(st != ip.KEPT, Om), key
    assert np.array_equal(bits32(got[~Om]), bits32(np.asarray(frames[t], np.float32)[~Om])), key  # untouched pixels
    only = optical_flow.blend_fill(frames, masks, fw, bw, t, radius, grow, **opts)
    assert isinstance(only, np.ndarray) and np.array_equal(only, got), key
    return st


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 7), (2, 2), (37, 53), (48, 65)])
def test_blend_fill_bitwise_vs_numpy(H, W, Cc):
    seen = set()
    for T, ts in ((1, (0,)), (5, (0, 2))):
        frames, fw, bw, rng = fill_case(H, W, Cc, T, 1000 * H + W + 7 * Cc + 31 * T)
        for kind in ("random", "empty", "full", "corner", "block"):
            if kind == "block":
                masks = [np.zeros((H, W), np.uint8) for _ in range(T)]
                for s, m in enumerate(masks):
                    m[H // 4 + s:H // 4 + s + H // 3 + 1, W // 4 + 2 * s:W // 4 + 2 * s + W // 3 + 1] = 1
            else:
                masks = make_masks(kind, T, H, W, rng)
            for t in ts:
                for radius, grow in ((1, 0), (3, 1)) + (((16, 8),) if kind in ("corner", "block") else ()):
                    st = check_blend(frames, masks, fw, bw, t, radius, grow, (T, t, kind, radius, grow))
                    seen |= set(np.unique(st).tolist())
    if H * W > 1000:
        assert seen == {ip.KEPT, ip.FILLED, pn.SPATIAL}
    frames, fw, bw, rng = fill_case(H, W, Cc, 3, 5)
    masks = make_masks("corner", 3, H, W, rng)
    check_blend(frames, masks, fw, bw, 1, 2, 2, "few cycles", cycles=1, sweeps=1, coarse_sweeps=3)


def test_blend_fill_four_channels_on_the_scene_is_the_restatement():
    frames, masks, fw, bw, _ = ip.scene(0)
    f4 = [np.stack([f, 255.0 - f, 0.5 * f, f + 3.0], axis=2).astype(np.float32) for f in frames]
    for t, radius in ((0, 6), (4, 1), (8, 2)):
        check_blend(f4, masks, fw, bw, t, radius, 1, (t, radius))


# ---- the session ----------------------------------------------------------------
def pair(a, b, w):
    import optical_flow
    return (optical_flow.estimate_flow(a, b, "classic+nl-fast", data_weight=w),
            optical_flow.estimate_flow(b, a, "classic+nl-fast", data_weight=w))


def flows_of(frames, masks, grow, margin):
    """The flows the session estimates, by hand (test_gpu_inpaint checks that they are)."""
    import optical_flow
    fw, bw = [], []
    for j in range(len(frames) - 1):
        f, b = pair(frames[j], frames[j + 1], optical_flow.pair_weight(masks[j], masks[j + 1], grow, margin))
        fw.append(f)
        bw.append(b)
    return fw, bw


@pytest.fixture(scope="module")
def scene_flows():
    frames, masks, _, _, truth = ip.scene(0)
    return frames, masks, truth, flows_of(frames, masks, 1, 4)


def test_session_with_blending_is_blend_fill_on_its_flows(scene_flows):
    import optical_flow
    frames, masks, _, (fw, bw) = scene_flows
    out, st = optical_flow.inpaint_frames(frames, masks, "classic+nl-fast", radius=6, grow=1, return_status=True,
                                          blend=True)
    assert out.shape == (9, 48, 64) and out.dtype == np.float64 and st.shape == (9, 48, 64)
    for t in range(9):
        want, want_st = optical_flow.blend_fill(frames, masks, fw, bw, t, 6, 1, return_status=True)
        assert np.array_equal(st[t], want_st), t
        assert np.array_equal(bits64(out[t]), bits64(want)), (t, np.abs(out[t] - want).max())
    # other options reach the solver
    few = optical_flow.inpaint_frames(frames[:3], masks[:3], radius=1, grow=1, blend=True, cycles=1, sweeps=1,
                                      coarse_sweeps=2)
    for t in range(3):
        want = optical_flow.blend_fill(frames[:3], masks[:3], fw[:2], bw[:2], t, 1, 1, cycles=1, sweeps=1,
                                       coarse_sweeps=2)
        assert np.array_equal(bits64(few[t]), bits64(want)), t


@pytest.mark.parametrize("Cc", [1, 3])
def test_session_without_blending_is_the_plain_fill_and_lifecycle(Cc):
    import optical_flow
    from optical_flow import _abi, _native
    H, W, R = 37, 53, 1
    frames, masks = clip_frames(H, W, Cc, 4, 60 + Cc)
    fw, bw = flows_of(frames, masks, 1, 3)
    plain = [optical_flow.propagate_fill(frames, masks, fw, bw, t, R, 1, return_status=True) for t in range(4)]
    off, off_st = optical_flow.inpaint_frames(frames, masks, radius=R, grow=1, margin=3, return_status=True,
                                              blend=False)
    for t in range(4):
        assert np.array_equal(off_st[t], plain[t][1]) and np.array_equal(bits64(off[t]), bits64(plain[t][0])), t
    ctx = _native.context()
    lib, hd = ctx.lib, ctx.handle
    bo = _abi.OfBlendOpts(8, 2, 32, 0)
    assert lib.of_inpaint_set_blend(hd, C.byref(bo)) == _abi.OF_EINVAL  # no session is open
    with pytest.raises(ValueError, match="no inpainter"):
        ctx.check(lib.of_inpaint_set_blend(hd, C.byref(bo)))
    optical_flow.inpaint_frames(frames, masks, radius=R, grow=1, margin=3, blend=True)  # grows the arena
    b0 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
    px = H * W
    with optical_flow.VideoInpainter(H, W, Cc, radius=R, grow=1, margin=3) as vi:
        b1 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
        for bad in ((0, 2, 32), (8, 3, 32), (8, 2, 65)):
            assert lib.of_inpaint_set_blend(hd, C.byref(_abi.OfBlendOpts(*bad, 0))) == _abi.OF_EINVAL
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b1
        ctx.check(lib.of_inpaint_set_blend(hd, C.byref(bo)))
        b2 = ctx.get_option(_abi.OF_OPT_DEVICE_BYTES)
        assert b2 - b1 == (2 * R + 1) * px  # the masks grown by one more
        ctx.check(lib.of_inpaint_set_blend(hd, None))  # off again: the pushes are the plain ones
        ctx.check(lib.of_inpaint_set_blend(hd, C.byref(bo)))
        ctx.check(lib.of_inpaint_set_blend(hd, None))
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b2
        got = {}
        for k, (f, m) in enumerate(zip(frames, masks)):
            r = vi.push(f, m)
            if r:
                got[r[0]] = (r[1], vi.last_status)
            # refused from the first push on
            assert lib.of_inpaint_set_blend(hd, C.byref(bo)) == _abi.OF_EINVAL
            assert lib.of_inpaint_set_blend(hd, None) == _abi.OF_EINVAL
        for r in vi.flush():
            got[r[0]] = (r[1], vi.last_status)
        with pytest.raises(ValueError, match="before the first push"):
            ctx.check(lib.of_inpaint_set_blend(hd, C.byref(bo)))
        assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b2
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    for t in range(4):
        assert np.array_equal(got[t][1], plain[t][1]) and np.array_equal(bits64(got[t][0]), bits64(plain[t][0])), t
    with optical_flow.VideoInpainter(H, W, Cc, radius=R, grow=1, margin=3, blend=True) as vi:
        assert vi.blend and ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b2
        res = [vi.push(f, m) for f, m in zip(frames, masks)]
        res = [r for r in res if r] + list(vi.flush())
    assert ctx.get_option(_abi.OF_OPT_DEVICE_BYTES) == b0
    for t, o in res:
        assert np.array_equal(bits64(o), bits64(optical_flow.blend_fill(frames, masks, fw, bw, t, R, 1))), t


def test_quality_gates_with_estimated_flows(scene_flows):
    """The gates of test_poisson_cpu.test_scene_quality_along_the_known_flows
    with flows estimated under the pair weight (grow 1, margin 4), per drift
    from the drifting frames themselves.  Measured on one MI355X: d = 0.03:
    plain MSE 89.57, blended 22.58; no drift: 0.420 and 0.412; radius 1: 612
    sourced pixels, plain 0.553, blended 0.235; 1656 spatial pixels, MSE 968.8
    against the truth's variance of 1719.9 over them."""
    import optical_flow
    frames, masks, truth, flows0 = scene_flows
    T = len(frames)
    cache = {}

    def flows(fr):
        key = float(fr[0][0, 0])
        if key not in cache:
            cache[key] = flows0 if all(np.array_equal(a, b) for a, b in zip(fr, frames)) else flows_of(fr, masks, 1, 4)
        return cache[key]

    def plain(fr, radius):
        fw, bw = flows(fr)
        res = [optical_flow.propagate_fill(fr, masks, fw, bw, t, radius, 1, return_status=True) for t in range(T)]
        return [r[0] for r in res], [r[1] for r in res]

    def blended(fr, radius):
        fw, bw = flows(fr)
        res = [optical_flow.blend_fill(fr, masks, fw, bw, t, radius, 1, return_status=True) for t in range(T)]
        return [r[0] for r in res], [r[1] for r in res]

    quality_gates(frames, masks, truth, plain, blended, "estimated flows,")
