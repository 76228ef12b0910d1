"""Layered motion segmentation on the GPU: of_segment_motion bitwise against
the numpy float64 restatement (tests/layers_numpy.py) over the reduction's
seams, the input forms and the option sets, every branch of the algorithm
seen; the quality gates of tests/test_layers_cpu.py through the package; the
entry's own argument checks; and of_fit_motion undisturbed by it."""
import ctypes as C

import numpy as np
import pytest

import layers_numpy as ln
from test_layers_cpu import MODELS, SCENES, TRUTH, SIGMA, affine_flow, check_gates, layered_scene

pytestmark = pytest.mark.gpu

# one partial tile; a second tile row of one row; a partial third tile column; five tile rows of one
# cell each; 16 tiles; 72 tiles (a two-level tree, cells of more than one tile); the scenes' size
SHAPES = [(1, 1), (5, 1), (3, 130), (37, 53), (64, 65), (72, 449), (120, 160)]
BRANCHES = {"stop", "discard", "none", "mode", "nohyp"}


def plant(flow):
    """The interpolation and fusion tests' planted cases in an (H, W, 2)
    float32 flow, returned with the pixels that hold +-1e30."""
    H, W = flow.shape[:2]
    n = H * W
    pix = lambda k: divmod(k, W)  # noqa: E731
    flow[pix(n - 1)] = (-0.0, -0.0)
    huge = []
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
        huge = [pix(2), pix(3)]
    return flow, huge


def two_layer_flow(H, W, model, rng):
    """Two motions of `model` split at 0.55 of the longer side, each sent
    through float32, with noise of SIGMA px and the planted cases."""
    a, b = (affine_flow(H, W, th).astype(np.float32) for th in TRUTH[model][:2])
    ii, jj = np.mgrid[0:H, 0:W]
    first = (jj < 0.55 * W) if W >= H else (ii < 0.55 * H)
    f = np.where(first[..., None], a, b) + rng.normal(0.0, SIGMA, (H, W, 2)).astype(np.float32)
    return plant(f.astype(np.float32))[0]


def one_layer_flow(H, W, model, rng):
    """One motion of `model` with noise of SIGMA px, nothing planted."""
    return (affine_flow(H, W, TRUTH[model][0]) + rng.normal(0.0, SIGMA, (H, W, 2))).astype(np.float32)


def shrinking_flow(H, W, rng):
    """One region of two interleaved motions 1.2 px apart, 60 % and 40 %: every
    cell's least-squares hypothesis lies between them and counts both, the
    Tukey passes settle on the larger one and lose the other's pixels."""
    f = rng.normal(0.0, 0.02, (H, W, 2)).astype(np.float32)
    f[:, np.arange(W) % 5 < 2, 0] += np.float32(1.2)
    return f


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_same(got, want, key):
    """labels, labels_raw, n and every number of every layer as bits."""
    assert got.n == want.n == len(got.layers), (key, got.n, want.n)
    for name in ("labels_raw", "labels"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == np.uint8 and g.shape == w.shape
        bad = np.argwhere(g != w)
        assert bad.size == 0, (key, name, len(bad), bad[:5])
    for l, (g, w) in enumerate(zip(got.layers, want.layers)):
        for name in ("theta", "matrix", "support", "rms"):
            assert np.array_equal(bits(getattr(g, name)), bits(getattr(w, name))), \
                (key, l, name, getattr(g, name), getattr(w, name))
        assert (g.pixels, g.degenerate) == (w.pixels, w.degenerate), (key, l, g.pixels, g.degenerate)
        assert g.matrix.shape == (2, 3) and g.theta.shape == (6,)


OPTION_SETS = [dict(grid=1), dict(grid=16), dict(passes=0), dict(rounds=0), dict(smooth=0), dict(smooth=3),
               dict(max_layers=1), dict(min_support=1.0), dict(cutoff=0.4, min_support=0.2, max_layers=8)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_segment_motion_bitwise_vs_numpy(H, W):
    """The three models on a two-layer flow with the planted cases in four
    forms: plain; with a weight plane (a tenth of it zero); with a state plane
    that also masks the first 16 x 64 pixels, so that a cell has no hypothesis;
    with both.  Then the other option sets, and a flow whose refitted layer
    falls below the support it was picked with."""
    import optical_flow
    rng = np.random.default_rng(1000 * H + W)
    weight = rng.uniform(0, 2, (H, W)).astype(np.float32)
    weight[rng.uniform(size=(H, W)) < 0.1] = 0.0
    state = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    if H > 16:
        state[:16, :64] = 1
    seen = set()

    def both(key, flow, model, w=None, s=None, **kw):
        want = ln.segment(flow, model, weight=w, state=s, **kw)
        got = optical_flow.segment_motion(flow, model, weight=w, state=s, return_raw=True, **kw)
        assert_same(got, want, key)
        seen.update(want.seen)
        return want, got

    for model in MODELS:
        flow = two_layer_flow(H, W, model, rng)
        for name, w, s in (("plain", None, None), ("weight", weight, None), ("state", None, state),
                           ("both", weight, state)):
            want, got = both((model, name), flow, model, w, s)
        only = optical_flow.segment_motion(flow, model, weight=weight, state=state)
        assert only.labels_raw is None and np.array_equal(only.labels, got.labels) and only.n == got.n
    for k, kw in enumerate(OPTION_SETS):
        model = MODELS[k % 3]
        want, _ = both((model, tuple(kw.items())), two_layer_flow(H, W, model, rng), model, **kw)
        if "min_support" in kw and kw["min_support"] == 1.0 and H * W >= 5:   # the NaN pixels are not explained
            assert want.n == 0 and np.all(want.labels == ln.NONE)
        if kw == dict(max_layers=1):
            assert want.n <= 1
    for model in MODELS:
        want, _ = both((model, "shrinking"), shrinking_flow(H, W, rng), model, min_support=0.8)
        if H * W > 1000:
            assert want.n == 0 and "discard" in want.seen, (model, want.seen)
        # one cell of all the tiles, and nothing after its solve: the layer is that hypothesis
        want, _ = both((model, "one cell"), one_layer_flow(H, W, model, rng), model, grid=1, passes=0, rounds=0)
        assert want.n == 1
    if H * W > 1000:
        assert seen == BRANCHES, seen  # every branch of the algorithm occurred


def test_a_cell_of_4097_tiles():
    """32776 x 1 with grid 1: the cell's reduction has three levels."""
    import optical_flow
    flow = one_layer_flow(32776, 1, "similarity", np.random.default_rng(5))
    kw = dict(grid=1, passes=0, rounds=0, smooth=1)
    want = ln.segment(flow, "similarity", **kw)
    assert_same(optical_flow.segment_motion(flow, "similarity", return_raw=True, **kw), want, "4097 tiles")
    assert want.n == 1 and want.layers[0].pixels > 32000


@pytest.mark.parametrize("kind,model", SCENES)
def test_segment_motion_meets_the_quality_gates(kind, model):
    import optical_flow
    f, gt, ths = layered_scene(kind, model)
    check_gates(optical_flow.segment_motion(f, model), gt, ths, (kind, model))


def test_argument_checks_and_degenerate_flows():
    import optical_flow
    from optical_flow import _abi, _native
    ctx = _native.context()
    lib, h = ctx.lib, ctx.handle
    H, W = 32, 40
    z = _native.f32(np.zeros((2, H, W)))
    fits = (_abi.OfMotionLayer * 8)()
    n = C.c_int32(-1)
    labels = np.empty((H, W), np.uint8)

    def lopts(**kw):
        a = dict(model=2, max_layers=4, grid=8, passes=4, rounds=3, smooth=2, cutoff=1.0, min_support=0.03)
        a.update(kw)
        return _abi.OfLayersOpts(*[a[k] for k, _ in _abi.OfLayersOpts._fields_])

    def call(o, weight=None, HH=H, WW=W):
        return lib.of_segment_motion(h, _native.ptr(z), HH, WW, _native.ptr(weight), None, C.byref(o), fits,
                                     C.byref(n), _native.u8ptr(labels), None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(model=-1), dict(model=3), dict(max_layers=0), dict(max_layers=9), dict(grid=0), dict(grid=17),
               dict(passes=-1), dict(passes=17), dict(rounds=-1), dict(rounds=17), dict(smooth=-1), dict(smooth=4),
               dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=nan), dict(cutoff=inf), dict(min_support=0.0),
               dict(min_support=1.5), dict(min_support=nan), dict(min_support=inf)):
        assert call(lopts(**kw)) == _abi.OF_EINVAL, kw
        with pytest.raises(ValueError):
            ctx.check(call(lopts(**kw)))
    for bad in (-1.0, nan, inf):
        w = np.ones((H, W), np.float32)
        w[3, 4] = bad
        with pytest.raises(ValueError, match="weight"):
            ctx.check(call(lopts(), w))
    with pytest.raises(NotImplementedError):
        ctx.check(call(lopts(), HH=46341, WW=46341))
    assert lib.of_segment_motion(h, _native.ptr(z), H, W, None, None, None, fits, C.byref(n), _native.u8ptr(labels),
                                 None) == _abi.OF_EINVAL
    ctx.check(call(lopts()))  # and the good call goes through: a zero flow is one layer, the identity
    assert n.value == 1 and np.all(labels == 0) and fits[0].pixels == H * W and fits[0].support == H * W
    assert list(fits[0].matrix) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] and fits[0].degenerate == 0
    # nothing usable: no layer, every label NONE
    for kw in (dict(flow=np.full((9, 70, 2), np.nan)), dict(flow=np.zeros((9, 70, 2)), weight=np.zeros((9, 70))),
               dict(flow=np.ones((9, 70, 2)), state=np.ones((9, 70), np.uint8))):
        r = optical_flow.segment_motion(return_raw=True, **kw)
        assert r.n == 0 and r.layers == [] and np.all(r.labels == ln.NONE) and np.all(r.labels_raw == ln.NONE)


def test_fit_motion_returns_the_same_bits_before_and_after_a_segmentation():
    import optical_flow
    f, _, _ = layered_scene("three", "affine")
    fit = lambda: optical_flow.fit_motion(f, "affine", return_inliers=True)  # noqa: E731
    before = fit()
    seg = optical_flow.segment_motion(f, "affine")
    after = fit()
    assert seg.n == 3
    for name in ("theta", "matrix", "cutoff", "support", "rms", "inliers"):
        assert np.array_equal(bits(getattr(before, name)), bits(getattr(after, name))), name
    assert (before.passes, before.degenerate) == (after.passes, after.degenerate)
