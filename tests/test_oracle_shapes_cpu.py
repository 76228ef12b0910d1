"""The float64 oracle pinned against the reference at degenerate and
tile-seam shapes (tests/golden/stage_shapes.npz, gen_stage_shapes.py): one
row, one column, planes smaller than a stencil radius, the B-spline prefilter's
taps or a filter window, and one pixel past a tile.  tests/test_gpu_stage_shapes.py
judges the HIP kernels by this oracle at these and larger shapes, so it has to
be right here first.

atol = 1e-10 max|ref| per array (measured: <= 4e-13 absolute on 0..255
data); the weighted median and the median, which select input values, exactly.
"""
import numpy as np
import pytest

import oracle as O
import stage_inputs as S


def _close(got, ref, what):
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= 1e-10 * np.abs(ref).max(), (what, err)


@pytest.fixture(scope="module")
def fx(golden):
    d = golden("stage_shapes.npz")

    def at(H, W):
        t = S.tag(H, W) + ":"
        return {k[len(t):]: v for k, v in d.items() if k.startswith(t)}
    return at


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_fixture_inputs_are_the_shared_recipe(fx, H, W):
    """The GPU sweep builds its inputs with stage_inputs.make(); at fixture
    shapes they are the fixture's own, and no warped coordinate is within
    1e-3 px of an in/out-of-bounds threshold."""
    d, m = fx(H, W), S.make(H, W)
    for k in ("images", "const", "uv", "occ", "lab"):
        np.testing.assert_array_equal(d[k], m[k], err_msg=k)
        np.testing.assert_array_equal(d[k], S.f32(d[k]), err_msg=k)  # float32-representable
    assert not S.near_threshold(d["uv"]).any()
    assert np.ptp(d["images"]) >= 40  # textured, not flat (57 on the six pixels of 2x3)


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_rof(fx, H, W):
    d = fx(H, W)
    for name, (theta, iters, alp) in S.ROF_CASES.items():
        if name in d:  # left out of the fixture at 113x49 (file size)
            _close(O.rof_texture(d["images"], theta, iters, alp), d[name], name)
    _close(O.rof_texture(d["const"], 1 / 8, 100, 0.95), d["rof_const"], "rof_const")
    assert ("rof100" in d and "rof37" in d) or (H, W) == (113, 49)


@pytest.mark.parametrize("H,W,case", [(113, 49, "rof100"), (113, 49, "rof37"), (5, 49, "rof100"), (5, 49, "rof37"),
                                      (37, 65, "rof100"), (37, 65, "rof37"), (60, 1100, "rof100"),
                                      (60, 1100, "rof37"), (130, 4100, "rof37")])
def test_rof_plain_float32(H, W, case):
    """The basis of the GPU sweep's ROF seam bound: the untiled numpy float32
    restatement is within half of S.ROF_SEAM_TOL of the oracle at every shape
    of the sweep that has a tile seam."""
    theta, iters, alp = S.ROF_CASES[case]
    rgb1, rgb2 = S.frames(H, W, 1000 + 7 * H + W)
    im = np.stack([rgb1[..., 1], rgb2[..., 1]], axis=2)
    e = np.abs(S.rof_texture_f32(im, theta, iters, alp) - O.rof_texture(im, theta, iters, alp)).max()
    print(f"plain float32 ROF {H}x{W} {case}: {e:.3e}")
    assert e <= S.ROF_SEAM_TOL / 2, e


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_pyramid(fx, H, W):
    d = fx(H, W)
    for sp in S.PYR_SPACINGS:
        p = O.pyramid(d["images"], S.pyramid_kernel(sp), S.PYR_LEVELS, 1.0 / sp)
        for lv in range(1, S.PYR_LEVELS):
            _close(p[lv], d[f"pyr_{sp}_{lv}"], (sp, lv))


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_resample(fx, H, W):
    d = fx(H, W)
    for name, sz in S.resample_sizes(H, W).items():
        if f"rs_{name}" in d:  # 'up' is left out of the fixture at 113x49 (file size)
            _close(O.resample_flow(d["uv"], sz), d[f"rs_{name}"], name)
    assert "rs_dn" in d and ("rs_up" in d or (H, W) == (113, 49))


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
@pytest.mark.parametrize("method", S.INTERPS)
def test_partial_deriv(fx, H, W, method):
    d = fx(H, W)
    out = O.partial_deriv(d["images"], d["uv"], method, S.FILT, 0.5)
    for got, name in zip(out, ("It", "Ix", "Iy")):
        ref = d[f"{method}_{name}"]
        assert got.shape == ref.shape
        # an all-zero plane (every sample out of bounds on a 1-pixel-wide
        # plane) has max|ref| = 0: then the oracle must be zero too
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (name, np.abs(got - ref).max())


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_occlusion(fx, H, W):
    d = fx(H, W)
    _close(O.detect_occlusion(d["uv"], d["images"]), d["occ_out"], "occ")


@pytest.mark.parametrize("H,W", S.FIXTURE_SHAPES)
def test_weighted_median_and_median(fx, H, W):
    d = fx(H, W)
    for name, (guide, hsz, sig) in S.WMF_CASES.items():
        g = d["lab"] if guide == "lab" else d["images"][..., 0]
        np.testing.assert_array_equal(O.weighted_median(d["uv"], g, d["occ"], hsz, sig), d[name], err_msg=name)
    for sz in S.MEDIAN_SIZES:
        np.testing.assert_array_equal(O.median_filter(d["uv"], sz), d[f"med{sz}"], err_msg=f"med{sz}")
