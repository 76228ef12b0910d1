"""Bidirectional flow / forward-backward check: what can be checked without a GPU."""
import numpy as np
import pytest


def test_package_exports_bidirectional_api():
    import optical_flow
    from optical_flow.utils import occlusion
    assert callable(optical_flow.estimate_flow_bidirectional)
    assert callable(optical_flow.forward_backward_check)
    assert optical_flow.forward_backward_check is occlusion.forward_backward_check
    assert (optical_flow.FB_CONSISTENT, optical_flow.FB_OCCLUDED, optical_flow.FB_OUT_OF_FRAME) == (0, 1, 2)
    assert (occlusion.FB_CONSISTENT, occlusion.FB_OCCLUDED, occlusion.FB_OUT_OF_FRAME) == (0, 1, 2)
    for name in ("estimate_flow_bidirectional", "forward_backward_check", "FB_CONSISTENT", "FB_OCCLUDED",
                 "FB_OUT_OF_FRAME"):
        assert name in optical_flow.__all__
    assert optical_flow.BidirectionalFlow._fields == ("forward", "backward", "occ_forward", "occ_backward")


def test_c_abi_mirror_declares_the_two_entries():
    from optical_flow import _native
    assert "of_fb_consistency" in _native._SIGS and "of_estimate_flow_bidir" in _native._SIGS
    assert len(_native._SIGS["of_fb_consistency"][0]) == 9
    assert len(_native._SIGS["of_estimate_flow_bidir"][0]) == 17


@pytest.mark.parametrize("s1,s2", [((8, 9, 3), (8, 10, 3)), ((8, 9), (8, 9, 3)), ((8, 9, 3), (9, 9, 3)),
                                   ((8, 9, 2), (8, 9, 1))])
def test_mismatched_frames_raise_before_any_library_call(monkeypatch, s1, s2):
    import optical_flow
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)
    with pytest.raises(ValueError):
        optical_flow.estimate_flow_bidirectional(np.zeros(s1), np.zeros(s2))
