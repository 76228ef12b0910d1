"""CPU tests of the reduced-resolution flow (include/optflow.h, "Reduced-
resolution flow with edge-aware upsampling"): the formula itself, on the numpy
float64 restatement (tests/upsample_numpy.py), the Python validators and the
C ABI mirror.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import upsample_numpy as un


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_stage_functions_and_the_scale_keywords():
    import optical_flow
    for name in ("reduce_frame", "upsample_flow"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    for fn in (optical_flow.estimate_flow, optical_flow.estimate_flow_bidirectional, optical_flow.interpolate_frames,
               optical_flow.PointTracker.__init__, optical_flow.track_points, optical_flow.TemporalDenoiser.__init__,
               optical_flow.denoise_frames, optical_flow.Stabilizer.__init__, optical_flow.stabilize_frames):
        p = inspect.signature(fn).parameters
        assert p["scale"].default == 1 and p["upsample_range"].default == 20.0, fn
    p = inspect.signature(optical_flow.upsample_flow).parameters
    assert list(p) == ["flow_lo", "guide", "scale", "range", "guide_lo", "return_info"]
    assert p["range"].default == 20.0 and p["guide_lo"].default is None and p["return_info"].default is False


def test_c_abi_mirror_declares_the_five_entries():
    from optical_flow import _abi, _native
    want = {"of_reduce_frame": 7, "of_flow_upsample": 10, "of_estimate_flow_scaled": 10,
            "of_estimate_flow_bidir_scaled": 16, "of_session_set_flow_scale": 3}
    for name, nargs in want.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _abi.OF_ABI_VERSION == 3
    assert ctypes.sizeof(_abi.OfUpsampleOpts) == 16 and _abi.OfUpsampleOpts.range.offset == 8
    assert (_abi.OF_SESSION_TRACKS, _abi.OF_SESSION_DENOISE, _abi.OF_SESSION_STAB) == (1, 2, 4)


def test_upsample_opts_layout_matches_header(tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    from optical_flow import _abi
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %d %d %d\\n",'
           'sizeof(of_upsample_opts), offsetof(of_upsample_opts, range), OF_SESSION_TRACKS, OF_SESSION_DENOISE,'
           'OF_SESSION_STAB);}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(_abi.OfUpsampleOpts), _abi.OfUpsampleOpts.range.offset,
                                     _abi.OF_SESSION_TRACKS, _abi.OF_SESSION_DENOISE, _abi.OF_SESSION_STAB]


# ---- argument checks: ValueError before the library is touched --------------
@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


IM = np.zeros((8, 9))
IM3 = np.zeros((8, 9, 3))
ZLO = np.zeros((4, 5, 2))
BAD_SCALES = [0, 5, -2, 2.0, "2", None, True]
BAD_RANGES = [0, -1.0, float("nan"), float("inf"), "20", None, True]


@pytest.mark.parametrize("scale", BAD_SCALES + [1])
def test_reduce_frame_bad_scale_raises_before_any_library_call(no_library, scale):
    import optical_flow
    with pytest.raises(ValueError, match="scale"):
        optical_flow.reduce_frame(IM, scale)


@pytest.mark.parametrize("im", [np.zeros((0, 4)), np.zeros(5), np.zeros((4, 4, 5)), np.zeros((2, 2, 2, 2)),
                                np.zeros((4, 4), dtype=complex)])
def test_reduce_frame_bad_frame_raises_before_any_library_call(no_library, im):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.reduce_frame(im, 2)


@pytest.mark.parametrize("kw", [dict(scale=s) for s in BAD_SCALES + [1]] + [dict(range=r) for r in BAD_RANGES]
                         + [dict(flow_lo=np.zeros((4, 4, 2))), dict(flow_lo=np.zeros((8, 9, 2))),
                            dict(flow_lo=np.zeros((4, 5))), dict(flow_lo=np.zeros((4, 5, 3))),
                            dict(guide=np.zeros((8, 9, 5))), dict(guide=np.zeros(8)),
                            dict(guide_lo=np.zeros((4, 5, 3))), dict(guide_lo=np.zeros((5, 5))),
                            dict(scale=3)])  # (8, 9) at scale 3 is (3, 3), not (4, 5)
def test_upsample_flow_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(flow_lo=ZLO, guide=IM, scale=2, guide_lo=np.zeros((4, 5)))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.upsample_flow(**a)


@pytest.mark.parametrize("kw", [dict(scale=s) for s in BAD_SCALES] + [dict(upsample_range=r) for r in BAD_RANGES])
def test_scale_keywords_raise_before_any_library_call(no_library, kw):
    import optical_flow
    for call in (lambda: optical_flow.estimate_flow(IM3, IM3, **kw),
                 lambda: optical_flow.estimate_flow_bidirectional(IM3, IM3, **kw),
                 lambda: optical_flow.interpolate_frames(IM3, IM3, **kw),
                 lambda: optical_flow.PointTracker((8, 9), **kw),
                 lambda: optical_flow.track_points([IM, IM], **kw),
                 lambda: optical_flow.TemporalDenoiser((8, 9), sigma=5.0, **kw),
                 lambda: optical_flow.denoise_frames([IM, IM], sigma=5.0, **kw),
                 lambda: optical_flow.Stabilizer((8, 9), **kw),
                 lambda: optical_flow.stabilize_frames([IM, IM], **kw)):
        with pytest.raises(ValueError, match="scale|upsample_range"):
            call()


def test_scale_refuses_what_it_cannot_combine_with(no_library):
    import optical_flow
    with pytest.raises(NotImplementedError, match="data_weight"):
        optical_flow.estimate_flow(IM3, IM3, data_weight=np.ones((8, 9)), scale=2)
    with pytest.raises(NotImplementedError):
        optical_flow.estimate_flow(np.zeros((8, 9, 2)), np.zeros((8, 9, 2)), scale=2)
    with pytest.raises(NotImplementedError):
        optical_flow.estimate_flow_bidirectional(np.zeros((8, 9, 2)), np.zeros((8, 9, 2)), scale=2)
    with pytest.raises(ValueError, match="scale"):
        optical_flow.interpolate_frames(IM3, IM3, flows=(np.zeros((8, 9, 2)), np.zeros((8, 9, 2))), scale=2)


# ---- the box reduction ------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_reduce_is_the_block_mean_with_clipped_last_blocks(s):
    rng = np.random.default_rng(s)
    im = rng.uniform(0, 255, (7, 10, 3)).astype(np.float32)
    L = un.reduce_frame(im, s)
    hs, ws = un.low_shape(7, 10, s)
    assert L.shape == (hs, ws, 3) and L.dtype == np.float32
    for a in range(hs):
        for b in range(ws):
            blk = im[a * s:(a + 1) * s, b * s:(b + 1) * s].astype(np.float64)
            np.testing.assert_allclose(L[a, b], blk.mean((0, 1)), rtol=1e-6)
    assert un.reduce_frame(im[..., 0], s).shape == (hs, ws)
    c = np.full((5, 6), 37.25, np.float32)
    assert np.array_equal(un.reduce_frame(c, s), np.full(un.low_shape(5, 6, s), 37.25, np.float32))


# ---- sharpness: a condition on the formula ----------------------------------
@pytest.fixture(scope="module", params=[(96, 128), (67, 131)], ids=lambda p: f"{p[0]}x{p[1]}")
def scenes(request):
    H, W = request.param
    return {sigma: un.two_layer_scene(H, W, sigma) for sigma in (0, 5)}


@pytest.mark.parametrize("sigma", [0, 5])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_edge_aware_weights_keep_the_motion_boundary_sharp(scenes, s, sigma):
    """Mean endpoint error in the band within s pixels of the rectangle's
    outline, range 20: at most a quarter of what the spatial weights alone
    leave, and at most 1 % of the pixels off the edge-aware branch."""
    im, flow, inside = scenes[sigma]
    L = un.reduce_frame(im, s)
    f_lo = un.reduce_frame(flow, s) / np.float32(s)
    out, info = un.upsample(f_lo, L, im, s, 20.0)
    plain, _ = un.upsample(f_lo, L, im, s, 20.0, spatial_only=True)
    band = un.outline_band(inside, s)
    epe = np.sqrt(((out.astype(np.float64) - flow) ** 2).sum(-1))[band].mean()
    epe_plain = np.sqrt(((plain.astype(np.float64) - flow) ** 2).sum(-1))[band].mean()
    share = float((info != 0).mean())
    print(f"{im.shape[:2]} s={s} sigma={sigma}: band AEPE {epe:.4f} vs spatial {epe_plain:.4f}, info != 0 {share:.5f}")
    assert band.sum() > 0 and np.all(np.isfinite(out))
    assert epe <= 0.25 * epe_plain
    assert share <= 0.01


# ---- fallbacks --------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_constant_low_flow_comes_back_as_exactly_s_times_itself(s):
    H, W = 13, 18
    hs, ws = un.low_shape(H, W, s)
    rng = np.random.default_rng(10 + s)
    guide = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)   # any guide, unrelated to the low one
    L = rng.uniform(0, 255, (hs, ws, 3)).astype(np.float32)
    f = np.empty((hs, ws, 2), np.float32)
    f[..., 0], f[..., 1] = 1.25, -0.75
    out, info = un.upsample(f, L, guide, s, 20.0)
    assert np.array_equal(out[..., 0], np.full((H, W), np.float32(s * 1.25)))
    assert np.array_equal(out[..., 1], np.full((H, W), np.float32(s * -0.75)))
    assert set(np.unique(info)) <= {0, 1}


@pytest.mark.parametrize("s", [2, 3])
def test_a_guide_unlike_the_low_guide_everywhere_gives_the_spatial_result(s):
    H, W = 11, 14
    hs, ws = un.low_shape(H, W, s)
    rng = np.random.default_rng(20 + s)
    L = rng.uniform(0, 50, (hs, ws)).astype(np.float32)
    guide = rng.uniform(100, 150, (H, W)).astype(np.float32)    # differs from L by more than range = 20 everywhere
    f = rng.normal(0, 2, (hs, ws, 2)).astype(np.float32)
    out, info = un.upsample(f, L, guide, s, 20.0)
    plain, _ = un.upsample(f, L, guide, s, 20.0, spatial_only=True)
    assert np.all(info == 1)
    assert np.array_equal(out, plain)


def test_an_all_nan_low_flow_gives_info_2_and_nan():
    H, W, s = 9, 10, 2
    hs, ws = un.low_shape(H, W, s)
    guide = np.full((H, W), 100.0, np.float32)
    out, info = un.upsample(np.full((hs, ws, 2), np.nan, np.float32), un.reduce_frame(guide, s), guide, s)
    assert np.all(info == 2) and np.all(np.isnan(out))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_a_nan_island_one_pixel_wide_is_bridged(s):
    H, W = 24, 28
    hs, ws = un.low_shape(H, W, s)
    guide = np.full((H, W, 3), 120.0, np.float32)
    f = np.empty((hs, ws, 2), np.float32)
    f[..., 0], f[..., 1] = 2.0, 1.0
    f[hs // 2, :, 0] = np.nan          # a row, a column and a speck, each 1 low pixel wide
    f[:, ws // 3, 1] = np.inf
    f[1, 1] = np.nan
    out, info = un.upsample(f, un.reduce_frame(guide, s), guide, s)
    assert np.all(np.isfinite(out)) and np.all(info == 0)
    assert np.array_equal(out[..., 0], np.full((H, W), np.float32(2.0 * s)))
    assert np.array_equal(out[..., 1], np.full((H, W), np.float32(1.0 * s)))


def test_a_guide_pixel_that_is_not_finite_takes_the_spatial_branch():
    H, W, s = 8, 10, 2
    hs, ws = un.low_shape(H, W, s)
    guide = np.full((H, W), 80.0, np.float32)
    L = un.reduce_frame(guide, s)
    guide[3, 4] = np.nan
    rng = np.random.default_rng(4)
    f = rng.normal(0, 1, (hs, ws, 2)).astype(np.float32)
    out, info = un.upsample(f, L, guide, s)
    plain, _ = un.upsample(f, L, guide, s, spatial_only=True)
    assert info[3, 4] == 1 and (info != 0).sum() == 1
    assert np.array_equal(out[3, 4], plain[3, 4]) and np.all(np.isfinite(out))
