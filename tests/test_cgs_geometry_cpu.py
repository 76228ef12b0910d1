"""Strip geometry of the fused CG iteration (k_cgs, 'backslash'), no device.

A k_cgs strip is 64 lanes x 2 px = 128 columns with 8 halo columns towards
each neighbouring strip.  The first strip has no neighbour on its left and the
last none on its right, so they own those 8 columns too: n strips cover
112 n + 16 columns, 1920 columns are 17 strips (120 + 15 * 112 + 120), and a
level of up to 128 columns is one strip.
"""
import pytest

WIDTHS = [1, 120, 128, 129, 240, 241, 1536, 1920, 3840, 57344]


def _strips(W):
    return max(1, -(-(W - 16) // 112))


@pytest.mark.parametrize("W", WIDTHS)
def test_cgs_strip_count(W):
    from optical_flow import _native
    g = _native.solver_geometry(40, W, "backslash")
    assert g["grid_x"] == _strips(W), (W, g)
    assert g["grid_x"] * g["strip_cols"] >= W, (W, g)
    assert g["strip_cols"] == (128 if g["grid_x"] == 1 else 120), (W, g)
    assert 1 <= g["blocks"] == g["grid_x"] * g["grid_y"] <= 512, (W, g)
    assert g["bands"] * g["rows"] >= 40 and g["grid_y"] == g["bands"], (W, g)


def test_cgs_strips_1080p():
    from optical_flow import _native
    g = _native.solver_geometry(1080, 1920, "backslash")
    assert g["grid_x"] == 17, g
    assert g["bands"] * g["rows"] >= 1080, g
    assert g["blocks"] <= 512, g
    # 864 x 1536 (the other token-holding level of a 1080p pair) keeps 14
    assert _native.solver_geometry(864, 1536, "backslash")["grid_x"] == 14


def test_cgs_too_wide_still_refused():
    from optical_flow import _native
    assert _native.solver_geometry(64, 57344, "backslash")["grid_x"] == 512
    with pytest.raises(NotImplementedError):
        _native.solver_geometry(64, 124 * 513, "backslash")
    with pytest.raises(NotImplementedError):
        _native.solver_geometry(64, 57344 + 17, "backslash")
