"""Frame interpolation / image warping: what can be checked without a GPU."""
import numpy as np
import pytest


def test_package_exports_interpolation_api():
    import optical_flow
    from optical_flow import interface
    from optical_flow.utils import warping
    assert callable(optical_flow.interpolate_frames) and callable(optical_flow.warp_image)
    assert optical_flow.interpolate_frames is interface.interpolate_frames
    assert optical_flow.warp_image is warping.warp_image
    assert (optical_flow.INTERP_BLEND, optical_flow.INTERP_FRAME1_ONLY, optical_flow.INTERP_FRAME2_ONLY,
            optical_flow.INTERP_NEITHER, optical_flow.INTERP_FILLED) == (0, 1, 2, 3, 4)
    for name in ("interpolate_frames", "warp_image", "INTERP_BLEND", "INTERP_FRAME1_ONLY", "INTERP_FRAME2_ONLY",
                 "INTERP_NEITHER", "INTERP_FILLED"):
        assert name in optical_flow.__all__


def test_c_abi_mirror_declares_the_three_entries():
    from optical_flow import _native
    assert len(_native._SIGS["of_warp_image"][0]) == 8
    assert len(_native._SIGS["of_interp_frames"][0]) == 15
    assert len(_native._SIGS["of_estimate_interp"][0]) == 17


@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


@pytest.mark.parametrize("s1,s2", [((8, 9, 3), (8, 10, 3)), ((8, 9), (8, 9, 3)), ((8, 9, 3), (9, 9, 3)),
                                   ((8, 9, 2), (8, 9, 1)), ((8, 9, 5), (8, 9, 5)), ((8,), (8,)), ((0, 9), (0, 9))])
def test_mismatched_frames_raise_before_any_library_call(no_library, s1, s2):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(np.zeros(s1), np.zeros(s2))
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(np.zeros(s1), np.zeros(s2), flows=(np.zeros(s1[:2] + (2,)),) * 2)


@pytest.mark.parametrize("fs", [((8, 9, 2), (8, 10, 2)), ((8, 9), (8, 9)), ((8, 9, 3), (8, 9, 3)),
                                ((9, 8, 2), (9, 8, 2))])
def test_mismatched_flows_raise_before_any_library_call(no_library, fs):
    import optical_flow
    im = np.zeros((8, 9, 3))
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(im, im, flows=(np.zeros(fs[0]), np.zeros(fs[1])))
    with pytest.raises(ValueError):
        optical_flow.warp_image(im, np.zeros(fs[0]) if fs[0] != (8, 9, 2) else np.zeros(fs[1]))


@pytest.mark.parametrize("t", [0, 1, 0.0, 1.0, float("nan"), -0.1, [], [0.5, 1.0], [[0.5]], float("inf")])
def test_bad_t_raises_before_any_library_call(no_library, t):
    import optical_flow
    im = np.zeros((8, 9, 3))
    z = np.zeros((8, 9, 2))
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(im, im, t)
    with pytest.raises(ValueError):
        optical_flow.interpolate_frames(im, im, t, flows=(z, z))


def test_warp_image_rejects_bad_images_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.warp_image(np.zeros((8, 9, 5)), np.zeros((8, 9, 2)))
    with pytest.raises(ValueError):
        optical_flow.warp_image(np.zeros((8,)), np.zeros((8, 2)))
    with pytest.raises(ValueError):
        optical_flow.warp_image(np.zeros((0, 9)), np.zeros((0, 9, 2)))
