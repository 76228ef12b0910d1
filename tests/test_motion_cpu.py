"""Global motion estimation and stabilisation: what can be checked without a
GPU -- the Python surface, the C ABI mirror, the argument checks, and the
numpy restatement (tests/motion_numpy.py) on hand-made cases, on the two-layer
scene it was prototyped on, and its path smoothing."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import motion_numpy as mn
from conftest import ROOT


def test_package_exports_motion_api():
    import optical_flow
    from optical_flow import motion
    for name in ("fit_motion", "warp_affine", "Stabilizer", "stabilize_frames", "MotionFit"):
        assert getattr(optical_flow, name) is getattr(motion, name)
        assert name in optical_flow.__all__
    assert optical_flow.MotionFit._fields == ("matrix", "theta", "cutoff", "support", "rms", "passes", "degenerate",
                                              "inliers")


def test_c_abi_mirror_declares_the_six_entries_and_three_structs(tmp_path):
    from optical_flow import _abi, _native
    want = {"of_fit_motion": 9, "of_warp_affine": 8, "of_stab_open": 6, "of_stab_push": 8, "of_stab_flush": 6,
            "of_stab_close": 1}
    for name, n in want.items():
        assert len(_native._SIGS[name][0]) == n, name
    offs = lambda S: [(f, getattr(S, f).offset) for f, _ in S._fields_]  # noqa: E731
    assert ctypes.sizeof(_abi.OfMotionOpts) == 32
    assert offs(_abi.OfMotionOpts) == [("model", 0), ("iters", 4), ("kappa", 8), ("decay", 16), ("c_min", 24)]
    assert ctypes.sizeof(_abi.OfMotionFit) == 128
    assert offs(_abi.OfMotionFit) == [("theta", 0), ("matrix", 48), ("cutoff", 96), ("support", 104), ("rms", 112),
                                      ("passes", 120), ("degenerate", 124)]
    assert ctypes.sizeof(_abi.OfStabOpts) == 64
    assert offs(_abi.OfStabOpts) == [("fit", 0), ("radius", 32), ("pad_", 36), ("sigma_t", 40), ("alpha1", 48),
                                     ("alpha2", 56)]
    dp, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    assert _native._SIGS["of_fit_motion"][0][6:8] == [ctypes.POINTER(_abi.OfMotionOpts),
                                                      ctypes.POINTER(_abi.OfMotionFit)]
    assert _native._SIGS["of_warp_affine"][0][5] == dp
    assert _native._SIGS["of_stab_push"][0][4:] == [dp, dp, i32p, i32p]
    assert _abi.OF_ABI_VERSION == 3
    assert _abi.MOTION_MODEL == {"translation": 0, "similarity": 1, "affine": 2}
    # ... and the C compiler lays the header's structs out the same way
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu '
           '%d %d\\n", sizeof(of_motion_opts), sizeof(of_motion_fit), sizeof(of_stab_opts), '
           'offsetof(of_motion_fit, passes), offsetof(of_stab_opts, sigma_t), offsetof(of_motion_opts, c_min), '
           'OF_MOTION_AFFINE, OF_ABI_VERSION);}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 128, 64, 120, 40, 24, 2, 3]


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
NAN, INF = float("nan"), float("inf")

BAD_FIT_OPTS = [
    dict(model="projective"), dict(model=2), dict(model=None), dict(iters=-1), dict(iters=65), dict(iters=1.0),
    dict(iters=True), dict(kappa=0.0), dict(kappa=-1.0), dict(kappa=NAN), dict(kappa=INF), dict(kappa="x"),
    dict(decay=0.0), dict(decay=1.5), dict(decay=-0.5), dict(decay=NAN), dict(c_min=0.0), dict(c_min=-1.0),
    dict(c_min=NAN), dict(c_min=INF)]


@pytest.mark.parametrize("kw", BAD_FIT_OPTS + [
    dict(flow=np.zeros((8, 9))), dict(flow=np.zeros((8, 9, 3))), dict(flow=np.zeros((0, 9, 2))),
    dict(flow=np.zeros((8, 9, 2), dtype=complex)), dict(weight=np.zeros((8, 10))), dict(weight=np.full((8, 9), -1.0)),
    dict(weight=np.full((8, 9), NAN)), dict(weight=np.full((8, 9), INF)), dict(state=np.zeros((8, 10), np.uint8)),
    dict(state=np.zeros((8, 9))), dict(state=np.full((8, 9), 256)), dict(state=np.full((8, 9), -1))])
def test_fit_motion_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(flow=Z)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.fit_motion(**a)


@pytest.mark.parametrize("kw", [
    dict(im=np.zeros(8)), dict(im=np.zeros((8, 9, 5))), dict(im=np.zeros((0, 9))),
    dict(im=np.zeros((8, 9), dtype=complex)), dict(matrix=np.eye(3)), dict(matrix=np.zeros(6)),
    dict(matrix=np.zeros((2, 3), dtype=complex)), dict(matrix=None)])
def test_warp_affine_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(im=IM, matrix=np.eye(3)[:2])
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.warp_affine(**a)


@pytest.mark.parametrize("kw", BAD_FIT_OPTS + [
    dict(shape=(8,)), dict(shape=(8, 9, 2)), dict(shape=(8, 9, 5)), dict(shape=(8, 9, 1)), dict(shape=(0, 9)),
    dict(method="nonexistent_method"), dict(radius=0), dict(radius=31), dict(radius=1.0), dict(radius=True),
    dict(sigma_t=0.0), dict(sigma_t=-1.0), dict(sigma_t=NAN), dict(sigma_t=INF), dict(alpha1=-0.5),
    dict(alpha2=INF)])
def test_stabilizer_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(shape=(8, 9))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.Stabilizer(**a)
    if "shape" not in kw:
        with pytest.raises(ValueError):
            optical_flow.stabilize_frames([IM, IM], **kw)


def test_stabilize_frames_bad_frames_raise_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.stabilize_frames([])
    with pytest.raises(ValueError):
        optical_flow.stabilize_frames([np.zeros((8, 9)), np.zeros((8, 10))])
    with pytest.raises(ValueError):
        optical_flow.stabilize_frames([np.zeros((8, 9, 5))])


# ---- the order of the sums ------------------------------------------------------
def test_sum_order_is_pinned_by_hand_computed_cases():
    # two tiles side by side.  Tile 0: the tree's first step adds column 32 to column 0 (1e16 + 1
    # rounds to 1e16) before column 16 cancels it: 0.0, where left to right gives 1.0.  Tile 1:
    # columns 1 and 33 cancel in the first step, so column 0's 1.0 survives, where left to right
    # loses it.  The group tree adds the two tile values: 1.0; the exact sum is 2.0.
    a = np.zeros((1, 128))
    a[0, 0], a[0, 16], a[0, 32] = 1e16, -1e16, 1.0
    a[0, 64], a[0, 65], a[0, 97] = 1.0, 1e16, -1e16
    assert list(mn.tile_values(a)) == [0.0, 1.0]
    assert mn.ordered_sum(a) == 1.0 and math.fsum(a.ravel()) == 2.0
    # a column adds its rows ascending: (1e16 + 1) - 1e16 = 0, not 1; the ninth row is a second tile
    b = np.array([[1e16], [1.0], [-1e16], [0.0], [0.0], [0.0], [0.0], [0.0], [3.0]])
    assert list(mn.tile_values(b)) == [0.0, 3.0] and mn.ordered_sum(b) == 3.0
    assert mn.ordered_sum(b[[0, 2, 1]]) == 1.0
    # 65 tiles: the second level has two groups, the last padded with zeros
    c = np.zeros((8 * 65, 1))
    c[::8, 0] = np.arange(1.0, 66.0)
    assert mn.tile_values(c).size == 65 and mn.ordered_sum(c) == 65.0 * 66.0 / 2.0
    assert mn.group_tree([5.0]) == 5.0 and mn.tree64(np.arange(64.0)) == 2016.0


@pytest.mark.parametrize("H,W", [(1, 1), (3, 130), (37, 53), (72, 449), (4100, 3)])
def test_sum_order_agrees_with_fsum(H, W):
    a = np.random.default_rng(H * 1000 + W).normal(0.0, 1.0, (H, W)) ** 3
    want = math.fsum(a.ravel())
    scale = math.fsum(np.abs(a).ravel())
    assert abs(mn.ordered_sum(a) - want) <= 1e-9 * scale


# ---- the fit on hand-made cases ----------------------------------------------------
def affine_flow(H, W, th):
    """The exact model flow of th, float64 (H, W, 2)."""
    _, _, _, x, y = mn.frame_coords(H, W)
    return np.stack([th[0] + th[1] * x + th[2] * y, th[3] + th[4] * x + th[5] * y], -1)


TH_AFF = (1.5, 0.25, -0.75, -0.5, 1.0, 0.5)
TH_SIM = (1.5, 0.8, -1.2, -0.7, 1.2, 0.8)             # the scene's: th1 = th5, th4 = -th2
TH_SIM_DYADIC = (1.5, 0.75, -1.25, -0.5, 1.25, 0.75)  # a similarity that float32 holds exactly


@pytest.mark.parametrize("model,th", [("affine", TH_AFF), ("similarity", TH_SIM_DYADIC), ("affine", TH_SIM_DYADIC),
                                      ("translation", (2.0, 0, 0, -3.0, 0, 0))])
def test_exact_model_flow_returns_its_parameters(model, th):
    # 24 x 40 (s = 20): the float32 flow is the model up to its rounding
    for it in (0, 10):
        r = mn.fit(affine_flow(24, 40, th), model, iters=it)
        assert r.degenerate == 0 and r.passes == it + 1
        assert np.abs(r.theta - np.array(th)).max() <= 1e-6
    # 16 x 32 (s = 16): x and y are multiples of 1/32, so with dyadic parameters the flow is exact
    # in float32 and the parameters come back to 1e-12
    f = affine_flow(16, 32, th)
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f)
    for it in (0, 10):
        r = mn.fit(f, model, iters=it)
        assert r.degenerate == 0 and np.abs(r.theta - np.array(th)).max() <= 1e-12, (it, r.theta)
        assert r.support == 16 * 32 and r.rms <= 1e-12 and (r.cutoff == 0.5 if it else r.cutoff > 2.0)
        assert np.all(r.inliers == 1.0)
        M = mn.matrix_of(list(th), 16, 32)
        assert np.abs(r.matrix - M).max() <= 1e-12
        # the matrix moves a pixel where the flow does: (j, i) -> (j + u, i + v)
        p = np.array([5.0, 3.0, 1.0])
        assert np.abs(M @ p - (p[:2] + f[3, 5])).max() <= 1e-12


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1)])
@pytest.mark.parametrize("model", ["similarity", "affine"])
def test_a_single_row_or_column_loses_rank_and_solves_the_translation(H, W, model):
    f = np.zeros((H, W, 2))
    f[..., 0], f[..., 1] = 2.0, -1.5
    r = mn.fit(f, model)
    if (H, W) != (1, 1) and model == "similarity":  # a line of points determines a similarity
        assert r.degenerate == 0
        assert np.abs(r.theta - np.array([2.0, 0, 0, -1.5, 0, 0])).max() <= 1e-12
    else:
        assert r.degenerate == 1
        assert np.array_equal(r.theta, [2.0, 0, 0, -1.5, 0, 0])
    assert r.passes == 11 and r.support == H * W
    t = mn.fit(f, "translation")
    assert t.degenerate == 0 and np.array_equal(t.theta, [2.0, 0, 0, -1.5, 0, 0])
    assert np.array_equal(t.matrix, [[1.0, 0.0, 2.0], [0.0, 1.0, -1.5]])


def test_an_all_masked_flow_stops_with_zero_parameters():
    f = np.full((6, 7, 2), 3.0)
    for kw in (dict(state=np.ones((6, 7), np.uint8)), dict(weight=np.zeros((6, 7))),
               dict(state=np.full((6, 7), 2, np.uint8), weight=np.ones((6, 7)))):
        r = mn.fit(f, "affine", **kw)
        assert r.degenerate == 2 and r.passes == 1 and np.array_equal(r.theta, np.zeros(6))
        assert np.array_equal(r.matrix, [[1.0, 0, 0], [0, 1.0, 0]])
        assert r.support == 0.0 and math.isnan(r.rms) and r.cutoff == 0.5 and np.all(r.inliers == 0.0)
    r = mn.fit(np.full((6, 7, 2), np.nan), "similarity")
    assert r.degenerate == 2 and np.array_equal(r.theta, np.zeros(6))


def test_masked_and_nonfinite_pixels_do_not_enter_the_fit():
    H, W = 20, 30
    rng = np.random.default_rng(11)
    base = (affine_flow(H, W, TH_AFF) + rng.normal(0, 0.2, (H, W, 2))).astype(np.float32)
    state = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), (H, W))
    weight = rng.uniform(0, 2, (H, W)).astype(np.float32)
    weight[rng.uniform(size=(H, W)) < 0.1] = 0.0
    bad = rng.uniform(size=(H, W)) < 0.1   # pixels whose flow is not finite, unmasked by the state
    a, b = base.copy(), base.copy()
    a[bad, 0], b[bad, 1] = np.nan, -np.inf
    a[state != 0] = (1e30, -7.0)
    b[state != 0] = (np.nan, np.inf)
    for model in ("translation", "similarity", "affine"):
        ra, rb = mn.fit(a, model, weight, state), mn.fit(b, model, weight, state)
        for k in ("theta", "matrix", "inliers"):
            assert np.array_equal(getattr(ra, k).view(np.uint32), getattr(rb, k).view(np.uint32)), k
        assert (ra.cutoff, ra.support, ra.rms, ra.passes, ra.degenerate) == \
               (rb.cutoff, rb.support, rb.rms, rb.passes, rb.degenerate)
        assert ra.degenerate == 0 and np.all(ra.inliers[bad | (state != 0) | (weight == 0)] == 0.0)
        assert np.array_equal(ra.masked, bad | (state != 0))
        assert np.abs(ra.theta - np.array(TH_AFF)).max() < (3.0 if model != "affine" else 0.2)


# ---- the prototype scene ----------------------------------------------------------
def scene(H=120, W=160, share=0.30, seed=0):
    """An affine (similarity) background flow TH_SIM with Gaussian noise of
    0.1 px and a block of `share` of the area moving (6, -4)."""
    rng = np.random.default_rng(seed)
    f = affine_flow(H, W, TH_SIM) + rng.normal(0.0, 0.1, (H, W, 2))
    bh = int(round(H * 0.6))
    bw = int(round(share * H * W / bh))
    fg = np.zeros((H, W), bool)
    fg[H // 5:H // 5 + bh, W // 4:W // 4 + bw] = True
    f[fg] = (6.0, -4.0)
    return f.astype(np.float32), fg


def test_the_scene_is_recovered_where_least_squares_is_not():
    """120 x 160, 30 % foreground.  Measured max |dth|: affine 1.0e-3,
    similarity 7.8e-4, least squares (iters = 0) 1.35 for both (a prototype
    with another true motion: 0.0018 / 0.0009 / 1.9).  The gate of 0.01 is about
    three standard errors of a 0.1 px noise fit plus the Tukey bias."""
    f, fg = scene()
    assert abs(fg.mean() - 0.30) < 0.005
    for model in ("affine", "similarity"):
        r = mn.fit(f, model)
        err = np.abs(r.theta - np.array(TH_SIM)).max()
        ls = mn.fit(f, model, iters=0)
        err_ls = np.abs(ls.theta - np.array(TH_SIM)).max()
        inl = r.inliers
        print(f"{model}: max |dth| {err:.2e} (least squares {err_ls:.2f}), cutoff {r.cutoff:.3f}, rms {r.rms:.3f}, "
              f"support {r.support:.0f}, inliers on the background {inl[~fg].mean():.3f}, foreground "
              f"{inl[fg].mean():.4f}")
        assert r.degenerate == 0 and r.passes == 11 and r.cutoff == 0.5
        assert err <= 0.01
        assert err_ls > 1.0
        # the inlier plane segments the two layers
        assert inl[~fg].mean() > 0.7 and inl[fg].max() == 0.0
        assert 0.05 < r.rms < 0.2


# ---- the affine warp ------------------------------------------------------------------
def test_warp_affine_restatement():
    rng = np.random.default_rng(4)
    im = rng.uniform(0, 255, (7, 9, 3)).astype(np.float32)
    out, valid = mn.warp_affine(im, mn.I6)
    assert np.array_equal(out, im) and valid.all() and out.dtype == np.float32 and valid.dtype == np.uint8
    out, valid = mn.warp_affine(im[..., 0], [1, 0, 2, 0, 1, -1])   # out(i, j) = im(i - 1, j + 2)
    assert np.array_equal(out[1:, :7], im[:-1, 2:, 0]) and valid[1:, :7].all()
    assert not valid[0].any() and not valid[:, 7:].any() and np.all(out[0] == 0) and np.all(out[:, 7:] == 0)
    out, valid = mn.warp_affine(im, [1, 0, 0.5, 0, 1, 0])
    want = (0.5 * im[:, :-1].astype(np.float64) + 0.5 * im[:, 1:].astype(np.float64)).astype(np.float32)
    assert np.array_equal(out[:, :-1], want) and valid[:, :-1].all() and not valid[:, -1].any()
    out, valid = mn.warp_affine(im, [1, 0, np.nan, 0, 1, 0])
    assert not valid.any() and np.all(out == 0)


# ---- path smoothing ---------------------------------------------------------------------
def test_inverse_and_composition():
    M = (1.1, -0.2, 3.0, 0.3, 0.9, -2.0)
    P = mn.compose(M, mn.inv(M))
    assert np.abs(np.array(P) - np.array(mn.I6)).max() <= 1e-15
    assert mn.compose(M, mn.I6) == M and mn.compose(mn.I6, M) == M
    A, B = np.vstack([np.reshape(M, (2, 3)), [0, 0, 1]]), np.array([[0.5, 1, 2], [0, 2, -1], [0, 0, 1.0]])
    assert np.abs(np.array(mn.compose(M, B[:2])).reshape(2, 3) - (A @ B)[:2]).max() <= 1e-15
    assert mn.keep(M) == (M, 0)
    for bad in ((1, 2, 0, 2, 4, 0), (1e-7, 0, 0, 0, 1e-7, 0), (1, 0, np.nan, 0, 1, 0), (np.inf, 0, 0, 0, 1, 0)):
        assert mn.keep(bad) == (mn.I6, 4)
    assert mn.keep((1e-6, 0, 0, 0, 1e-6, 5.0))[1] == 0   # det = 1e-12 exactly: kept


def test_identity_motions_give_identity_transforms():
    for radius in (1, 3, 30):
        for t in (0, 2, 5):
            S = mn.smooth([mn.I6] * 5, t, 6, radius, 3.0)
            assert np.array_equal(S, np.reshape(mn.I6, (2, 3)))


@pytest.mark.parametrize("radius,sigma_t", [(1, 3.0), (3, 1.5), (8, 3.0)])
def test_pure_translations_are_smoothed_linearly(radius, sigma_t):
    rng = np.random.default_rng(radius)
    n = 12
    c = np.cumsum(rng.uniform(-3, 3, (n, 2)), 0)   # the camera positions
    motions = [(1.0, 0.0, c[k + 1, 0] - c[k, 0], 0.0, 1.0, c[k + 1, 1] - c[k, 1]) for k in range(n - 1)]
    for frames in (n, 5):   # the whole clip, and a clip of 5 frames so far
        for t in range(frames):
            S = mn.smooth(motions, t, frames, radius, sigma_t)
            ds = [d for d in range(-radius, radius + 1) if 0 <= t + d <= frames - 1]
            g = np.array([math.exp(-(d * d) / (2 * sigma_t * sigma_t)) for d in ds])
            want = (g[:, None] * c[[t + d for d in ds]]).sum(0) / g.sum() - c[t]
            assert np.array_equal(S[:, :2], np.eye(2))
            assert np.abs(S[:, 2] - want).max() <= 1e-12


def test_session_schedule():
    pushes, flush = mn.session_schedule(6, 2)
    assert [p[0] for p in pushes] == [-1, -1, 0, 1, 2, 3] and [f[0] for f in flush] == [4, 5]
    pushes, flush = mn.session_schedule(2, 3)
    assert [p[0] for p in pushes] == [-1, -1] and [f[0] for f in flush] == [0, 1]
