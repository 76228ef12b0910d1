"""CPU tests of the flow-guided video inpainting (include/optflow.h,
"Flow-guided video inpainting"): the arithmetic itself, on the numpy float64
restatement (tests/inpaint_numpy.py), the Python validators and the C ABI
mirror.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import inpaint_numpy as ip


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_new_functions():
    import optical_flow
    for name in ("grow_mask", "pair_weight", "propagate_fill", "VideoInpainter", "inpaint_frames"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    assert (optical_flow.INPAINT_KEPT, optical_flow.INPAINT_FILLED, optical_flow.INPAINT_UNFILLED) == (0, 1, 2)
    p = inspect.signature(optical_flow.grow_mask).parameters
    assert list(p) == ["mask", "g"]
    p = inspect.signature(optical_flow.pair_weight).parameters
    assert list(p) == ["mask_a", "mask_b", "grow", "margin"] and (p["grow"].default, p["margin"].default) == (2, 4)
    p = inspect.signature(optical_flow.propagate_fill).parameters
    assert list(p) == ["frames", "masks", "fw", "bw", "t", "radius", "grow", "return_status", "return_hops"]
    assert (p["radius"].default, p["grow"].default, p["return_status"].default, p["return_hops"].default) == \
        (8, 2, False, False)
    p = inspect.signature(optical_flow.VideoInpainter.__init__).parameters
    assert list(p)[:9] == ["self", "H", "W", "channels", "method", "params", "radius", "grow", "margin"]
    assert (p["radius"].default, p["grow"].default, p["margin"].default) == (8, 2, 4)
    for m in ("push", "flush", "close"):
        assert callable(getattr(optical_flow.VideoInpainter, m))
    assert list(inspect.signature(optical_flow.VideoInpainter.push).parameters) == ["self", "frame", "mask"]
    p = inspect.signature(optical_flow.inpaint_frames).parameters
    assert list(p)[:7] == ["frames", "masks", "method", "radius", "grow", "margin", "return_status"]
    assert (p["method"].default, p["radius"].default, p["grow"].default, p["margin"].default) == \
        ("classic+nl-fast", 8, 2, 4)
    assert "scale" not in p


def test_c_abi_mirror_declares_the_six_entries():
    from optical_flow import _abi, _native
    want = {"of_mask_grow": 8, "of_inpaint_fill": 14, "of_inpaint_open": 6, "of_inpaint_push": 6,
            "of_inpaint_flush": 4, "of_inpaint_close": 1}
    for name, nargs in want.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _native.EXPORTED_SYMBOLS[-6:] == tuple(want)  # appended
    assert _abi.OF_ABI_VERSION == 3
    assert ctypes.sizeof(_abi.OfInpaintOpts) == 16


FIELDS = ["radius", "grow", "margin", "pad_"]


def test_header_constants_and_struct_match_the_mirror(tmp_path):
    from conftest import ROOT
    from optical_flow import _abi
    offs = ", ".join(f"offsetof(of_inpaint_opts, {f})" for f in FIELDS)
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%d %d %d %d %d %d %d %d %zu'
           + " %zu" * len(FIELDS) + '\\n", OF_ABI_VERSION, OF_INPAINT_KEPT, OF_INPAINT_FILLED, OF_INPAINT_UNFILLED, '
           "OF_INPAINT_MAX_RADIUS, OF_INPAINT_MAX_GROW, OF_INPAINT_MAX_MARGIN, OF_MASK_GROW_MAX, "
           "sizeof(of_inpaint_opts), " + offs + ");}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[:8] == [3, _abi.OF_INPAINT_KEPT, _abi.OF_INPAINT_FILLED, _abi.OF_INPAINT_UNFILLED,
                       _abi.INPAINT_MAX_RADIUS, _abi.INPAINT_MAX_GROW, _abi.INPAINT_MAX_MARGIN, _abi.MASK_GROW_MAX]
    assert out[:8] == [3, 0, 1, 2, 16, 8, 16, 24]
    assert out[8:] == [ctypes.sizeof(_abi.OfInpaintOpts)] + [getattr(_abi.OfInpaintOpts, f).offset for f in FIELDS]
    assert out[8] == 16 and [n for n, _ in _abi.OfInpaintOpts._fields_] == FIELDS


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
MK = np.zeros((8, 9), np.uint8)
FL = np.zeros((8, 9, 2))
NAN_IM = np.full((8, 9), np.nan)
BAD_RADIUS = [dict(radius=v) for v in (0, 17, -1, 2.0, "2", None, True, float("nan"))]
BAD_GROW = [dict(grow=v) for v in (-1, 9, 1.0, "1", None, True, float("inf"))]
BAD_MARGIN = [dict(margin=v) for v in (-1, 17, 2.0, None, True)]


@pytest.mark.parametrize("mask", [np.zeros((8, 9)), np.zeros((8, 9), np.float32), np.zeros((8,), np.uint8),
                                  np.zeros((8, 9, 1), np.uint8), np.zeros((0, 9), np.uint8), "mask", None])
def test_masks_must_be_2d_integers_or_bools(no_library, mask):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.grow_mask(mask, 1)
    with pytest.raises(ValueError):
        optical_flow.pair_weight(mask, MK)
    with pytest.raises(ValueError):
        optical_flow.pair_weight(MK, mask)
    with pytest.raises(ValueError):
        optical_flow.propagate_fill([IM, IM], [MK, mask], [FL], [FL], 0)
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([IM, IM], [mask, MK])


@pytest.mark.parametrize("g", [-1, 25, 1.0, "1", None, True])
def test_grow_mask_bad_g(no_library, g):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.grow_mask(MK, g)


@pytest.mark.parametrize("kw", BAD_GROW + BAD_MARGIN + [dict(mask_b=np.zeros((9, 8), np.uint8))])
def test_pair_weight_bad_arguments(no_library, kw):
    import optical_flow
    a = dict(mask_a=MK, mask_b=MK)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.pair_weight(**a)


@pytest.mark.parametrize("kw", BAD_RADIUS + BAD_GROW + [
    dict(t=-1), dict(t=2), dict(t=0.0), dict(t=None), dict(masks=[MK]), dict(masks=[MK, MK, MK]),
    dict(masks=[MK, np.zeros((9, 8), np.uint8)]), dict(fw=[]), dict(bw=[FL, FL]), dict(fw=[np.zeros((8, 9, 3))]),
    dict(bw=[np.zeros((9, 8, 2))]), dict(frames=[IM, np.zeros((8, 8))]), dict(frames=[]),
    dict(frames=[IM, NAN_IM]), dict(frames=[np.full((8, 9), np.inf), IM]),
    dict(frames=[np.zeros((8, 9, 5))] * 2), dict(frames=[np.zeros(8)] * 2), dict(frames=[IM.astype(str)] * 2)])
def test_propagate_fill_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(frames=[IM, IM], masks=[MK, MK], fw=[FL], bw=[FL], t=0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.propagate_fill(**a)


@pytest.mark.parametrize("kw", BAD_RADIUS + BAD_GROW + BAD_MARGIN)
def test_session_bad_options_raise_before_any_library_call(no_library, kw):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.VideoInpainter(8, 9, 1, **kw)
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([IM, IM], [MK, MK], **kw)


def test_session_shapes_raise_before_any_library_call(no_library):
    import optical_flow
    for H, W, ch in ((0, 9, 1), (8, -1, 1), (8.0, 9, 1), (8, 9, 2), (8, 9, 4), (8, 9, True), (46341, 46341, 1)):
        with pytest.raises(ValueError):
            optical_flow.VideoInpainter(H, W, ch)
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([], [])
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([IM, IM], [MK])
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([IM, NAN_IM], [MK, MK])
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([np.zeros((8, 9, 2))] * 2, [MK, MK])  # a session takes 1 or 3 channels


# ---- properties of the restatement ------------------------------------------
def test_grow_is_the_square_window():
    rng = np.random.default_rng(5)
    M = (rng.uniform(size=(23, 31)) < 0.03).astype(np.uint8) * 7
    assert np.array_equal(ip.grow(M, 0), (M != 0).astype(np.uint8))
    for g in (1, 3, 8, 24):
        want = np.zeros(M.shape, np.uint8)
        for i, j in zip(*np.nonzero(M)):
            want[max(i - g, 0):i + g + 1, max(j - g, 0):j + g + 1] = 1
        assert np.array_equal(ip.grow(M, g), want), g
    assert ip.grow(M, 24).all()  # 23 x 31 lies within 24 pixels of any mark


def test_pair_weight_is_off_under_both_holes_and_their_margin():
    a, b = np.zeros((20, 30), bool), np.zeros((20, 30), np.int32)
    a[5, 6] = True
    b[12, 20] = -3
    w = ip.pair_weight(a, b, 1, 2)
    assert w.dtype == np.float32 and set(np.unique(w)) == {0.0, 1.0}
    want = np.ones((20, 30), np.float32)
    want[2:9, 3:10] = 0
    want[9:16, 17:24] = 0
    assert np.array_equal(w, want)


def test_fill_without_neighbours_or_flow_keeps_the_frame_bitwise():
    rng = np.random.default_rng(9)
    f = rng.uniform(0, 255, (10, 12, 3)).astype(np.float32)
    m = rng.uniform(size=(10, 12)) < 0.4
    out, st, hops, _ = ip.fill([f], [m], [], [], 0, 4, 0)
    assert np.array_equal(out.view(np.uint32), f.view(np.uint32)) and not hops.any()
    assert np.array_equal(st, np.where(m, ip.UNFILLED, ip.KEPT))
    # a NaN flow ends the walk: the frame's own value again
    bad = [np.full((10, 12, 2), np.nan, np.float32)]
    out, st, hops, ends = ip.fill([f, f], [m, m], bad, bad, 0, 4, 0)
    assert np.array_equal(out.view(np.uint32), f.view(np.uint32))
    assert (ends[0][m] == ip.END_NAN).all() and (ends[1][m] == ip.END_HOPS).all()


def test_nearer_hit_counts_more():
    H, W = 6, 20
    frames = [np.full((H, W), v, np.float32) for v in (10.0, 0.0, 0.0, 0.0, 100.0)]
    masks = [np.zeros((H, W), np.uint8) for _ in range(5)]
    for s in (1, 2, 3):
        masks[s][:] = 1  # frame 1 .. 3 are all hole: from 1, 1 hop back to frame 0 and 3 on to frame 4
    z = [np.zeros((H, W, 2), np.float32)] * 4
    out, st, hops, _ = ip.fill(frames, masks, z, z, 1, 4, 0)
    assert (st == ip.FILLED).all() and (hops[0] == 3).all() and (hops[1] == 1).all()
    assert np.array_equal(out, np.full((H, W), np.float32((1.0 * 100.0 + 3.0 * 10.0) / 4.0)))


# ---- the scene, along the known flows ---------------------------------------
def _run(frames, masks, fw, bw, truth, radius, grow):
    res = [ip.fill(frames, masks, fw, bw, t, radius, grow) for t in range(len(frames))]
    return res, ip.hole_scores([r[0] for r in res], [r[1] for r in res], masks, truth)


@pytest.fixture(scope="module")
def the_scene():
    return ip.scene(0)


@pytest.mark.parametrize("radius,grow", [(4, 0), (4, 2), (6, 1), (8, 2)])
def test_scene_along_the_known_flows(the_scene, radius, grow):
    """9 frames of 48 x 64 (inpaint_numpy.scene).  Measured with this texture
    seed, over the pixels of the rectangle in all frames: radius 4, grow 0:
    every pixel filled, MSE against the true background 0.38 (0.34 at grow 2),
    710 with all-zero flows at 97 % filled (1099 at grow 2, 89 %), 8086 for the
    untouched rectangle.  Gates: every hole pixel filled, and the compensated
    MSE below 1/100 of the zero-flow MSE of the same run."""
    frames, masks, fw, bw, truth = the_scene
    res, (share, mse) = _run(frames, masks, fw, bw, truth, radius, grow)
    zero = [np.zeros_like(f) for f in fw]
    _, (share0, mse0) = _run(frames, masks, zero, zero, truth, radius, grow)
    untouched = ip.hole_scores(frames, [np.where(m, ip.FILLED, ip.KEPT) for m in masks], masks, truth)[1]
    print(f"radius {radius} grow {grow}: filled {share:.4f}, MSE {mse:.3f}; zero flows: filled {share0:.4f}, "
          f"MSE {mse0:.1f}; untouched {untouched:.0f}")
    for (out, st, hops, _), f, m in zip(res, frames, masks):
        D = ip.grow(m, grow)
        assert (st[m != 0] == ip.FILLED).all() and (st[D != 0] != ip.KEPT).all() and (st[D == 0] == ip.KEPT).all()
        assert np.array_equal(out[D == 0].view(np.uint32), f[D == 0].view(np.uint32))
        assert np.array_equal((hops[0] > 0) | (hops[1] > 0), st == ip.FILLED) and hops.max() <= radius
    assert share == 1.0
    assert mse < mse0 / 100.0


def test_scene_radius_1_leaves_pixels_unfilled_with_the_frames_value(the_scene):
    frames, masks, fw, bw, truth = the_scene
    res, (share, mse) = _run(frames, masks, fw, bw, truth, 1, 0)
    print(f"radius 1 grow 0: filled {share:.4f}, MSE {mse:.3f}")
    n = 0
    for (out, st, hops, _), f in zip(res, frames):
        un = st == ip.UNFILLED
        n += int(un.sum())
        assert np.array_equal(out[un].view(np.uint32), f[un].view(np.uint32))
        assert not hops[:, un].any()
    assert n > 0 and share < 1.0


def test_session_schedule_order():
    frames = [np.zeros((4, 5), np.float32)] * 5
    masks = [np.zeros((4, 5), np.uint8)] * 5
    outs, order = ip.session(frames, masks, 2, 0, 0, pair_fn=lambda a, b, w: (np.zeros((4, 5, 2)),) * 2,
                             fill_fn=lambda fr, mk, fw, bw, t, r, g: ip.fill(fr, mk, fw, bw, t, r, g)[:2])
    assert order == [(2, 0), (3, 1), (4, 2), ("flush", 3), ("flush", 4)] and len(outs) == 5
    _, order = ip.session(frames[:1], masks[:1], 2, 0, 0, pair_fn=None,
                          fill_fn=lambda fr, mk, fw, bw, t, r, g: ip.fill(fr, mk, fw, bw, t, r, g)[:2])
    assert order == [("flush", 0)]
