"""CPU tests of the gradient-domain blending (include/optflow.h,
"Gradient-domain blending"): the multigrid schedule itself, on the numpy
float64 restatement (tests/poisson_numpy.py) against an exact sparse solve,
the blended fill's quality on the inpainting scene, the Python validators and
the C ABI mirror.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import inpaint_numpy as ip
import poisson_numpy as pn


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_new_functions():
    import optical_flow
    for name in ("poisson_fill", "blend_fill"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    assert "INPAINT_SPATIAL" in optical_flow.__all__ and optical_flow.INPAINT_SPATIAL == 3
    p = inspect.signature(optical_flow.poisson_fill).parameters
    assert list(p)[:5] == ["values", "unknown", "source", "has_source", "excluded"]
    assert (p["cycles"].default, p["sweeps"].default, p["coarse_sweeps"].default) == (pn.CYCLES, pn.SWEEPS, pn.COARSE)
    p = inspect.signature(optical_flow.blend_fill).parameters
    assert list(p)[:7] == ["frames", "masks", "fw", "bw", "t", "radius", "grow"] and "return_status" in p
    assert (p["radius"].default, p["grow"].default, p["cycles"].default, p["return_status"].default) == \
        (8, 2, pn.CYCLES, False)
    for f in (optical_flow.VideoInpainter.__init__, optical_flow.inpaint_frames):
        p = inspect.signature(f).parameters
        assert p["blend"].default is False and p["cycles"].default == pn.CYCLES
        assert list(p).index("blend") > list(p).index("params")


def test_c_abi_mirror_declares_the_three_entries():
    from optical_flow import _abi, _native
    want = {"of_poisson_solve": 10, "of_inpaint_blend": 14, "of_inpaint_set_blend": 2}
    for name, nargs in want.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _native.EXPORTED_SYMBOLS[-9:-6] == tuple(want)  # before the six of the inpainter, which stay last
    assert _abi.OF_ABI_VERSION == 3
    assert ctypes.sizeof(_abi.OfBlendOpts) == 16 and ctypes.sizeof(_abi.OfInpaintOpts) == 16


FIELDS = ["cycles", "sweeps", "coarse_sweeps", "pad_"]


def test_header_constants_and_struct_match_the_mirror(tmp_path):
    from conftest import ROOT
    from optical_flow import _abi
    offs = ", ".join(f"offsetof(of_blend_opts, {f})" for f in FIELDS)
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%d %d %d %d %d %d %d %d %zu'
           + " %zu" * len(FIELDS) + '\\n", OF_ABI_VERSION, OF_INPAINT_SPATIAL, OF_PSN_FIXED, OF_PSN_UNKNOWN, '
           "OF_PSN_EXCLUDED, OF_BLEND_MAX_CYCLES, OF_BLEND_MAX_SWEEPS, OF_BLEND_MAX_COARSE_SWEEPS, "
           "sizeof(of_blend_opts), " + offs + ");}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[:8] == [3, _abi.OF_INPAINT_SPATIAL, _abi.OF_PSN_FIXED, _abi.OF_PSN_UNKNOWN, _abi.OF_PSN_EXCLUDED,
                       _abi.BLEND_MAX_CYCLES, _abi.BLEND_MAX_SWEEPS, _abi.BLEND_MAX_COARSE_SWEEPS]
    assert out[:8] == [3, 3, pn.FIXED, pn.UNKNOWN, pn.EXCLUDED, pn.MAX_CYCLES, pn.MAX_SWEEPS, pn.MAX_COARSE]
    assert out[8:] == [ctypes.sizeof(_abi.OfBlendOpts)] + [getattr(_abi.OfBlendOpts, f).offset for f in FIELDS]
    assert out[8] == 16 and [n for n, _ in _abi.OfBlendOpts._fields_] == FIELDS


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
ONE = np.eye(8, 9, dtype=np.uint8)
FL = np.zeros((8, 9, 2))
BAD_OPTS = [dict(cycles=v) for v in (0, 65, -1, 2.0, "2", None, True, float("nan"))] + \
    [dict(sweeps=v) for v in (0, 3, 1.0, None, True)] + [dict(coarse_sweeps=v) for v in (0, 65, 8.0, None, False)]


@pytest.mark.parametrize("kw", BAD_OPTS + [
    dict(values=np.zeros(8)), dict(values=np.zeros((8, 9, 5))), dict(values=np.zeros((0, 9))),
    dict(values=np.full((8, 9), np.nan)), dict(values=IM.astype(str)), dict(unknown=np.zeros((9, 8), np.uint8)),
    dict(unknown=np.zeros((8, 9))), dict(unknown=None), dict(excluded=np.zeros((8, 9))), dict(excluded=ONE),
    dict(source=IM), dict(has_source=MK), dict(source=np.zeros((8, 9, 3)), has_source=MK),
    dict(source=np.full((8, 9), np.inf), has_source=MK), dict(source=IM, has_source=np.zeros((8, 9)))])
def test_poisson_fill_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(values=IM, unknown=ONE)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.poisson_fill(**a)


@pytest.mark.parametrize("kw", BAD_OPTS + [dict(radius=0), dict(grow=9), dict(t=2), dict(masks=[MK]), dict(fw=[]),
                                           dict(frames=[IM, np.full((8, 9), np.nan)])])
def test_blend_fill_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(frames=[IM, IM], masks=[MK, MK], fw=[FL], bw=[FL], t=0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.blend_fill(**a)


@pytest.mark.parametrize("kw", BAD_OPTS + [dict(blend=1), dict(blend=None), dict(blend="yes")])
def test_session_bad_blend_options_raise_before_any_library_call(no_library, kw):
    import optical_flow
    kw = dict(dict(blend=True), **kw)
    with pytest.raises(ValueError):
        optical_flow.VideoInpainter(8, 9, 1, **kw)
    with pytest.raises(ValueError):
        optical_flow.inpaint_frames([IM, IM], [MK, MK], **kw)


# ---- the schedule -----------------------------------------------------------
def test_levels_depend_on_the_frame_size_alone():
    assert [pn.n_levels(*s) for s in ((1, 1), (30, 30), (31, 30), (48, 64), (61, 83), (200, 300), (540, 960),
                                      (1080, 1920))] == [0, 0, 1, 1, 2, 4, 5, 6]


def _problem(H, W, C, seed, unknown, excluded=None, guided=False):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 255, (C, H, W)).astype(np.float32).astype(np.float64)
    lab = np.where(unknown, pn.UNKNOWN, pn.FIXED).astype(np.uint8)
    if excluded is not None:
        lab[excluded & ~unknown] = pn.EXCLUDED
    s = h = None
    if guided:
        s = rng.uniform(0, 255, (C, H, W)).astype(np.float32).astype(np.float64)
        h = rng.uniform(size=(H, W)) < 0.8
    return lab, v, s, h


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (9, 1), (37, 53), (48, 65), (70, 129)])
def test_the_window_is_invisible(H, W):
    """The solve on the window around the unknowns and on the whole frame give
    the same bits, whatever the levels' alignment to the hole."""
    rng = np.random.default_rng(H * W)
    unknown = np.zeros((H, W), bool)
    i0, j0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    unknown[i0:i0 + max(H // 3, 1), j0:j0 + max(W // 3, 1)] = True
    unknown[rng.uniform(size=(H, W)) < 0.02] = True
    lab, v, s, h = _problem(H, W, 2, 7, unknown, rng.uniform(size=(H, W)) < 0.1, guided=True)
    a = pn.solve(lab, v, s, h, cycles=2, crop=True)
    b = pn.solve(lab, v, s, h, cycles=2, crop=False)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a[:, lab != pn.UNKNOWN], v[:, lab != pn.UNKNOWN])


def test_degenerate_problems():
    lab, v, _, _ = _problem(12, 14, 1, 3, np.zeros((12, 14), bool))
    assert np.array_equal(pn.solve(lab, v), v)  # nothing to solve
    # an unknown whose neighbours are all excluded keeps its value; all unknown (singular) stays finite
    unknown = np.zeros((12, 14), bool)
    unknown[5, 5] = True
    ex = np.zeros((12, 14), bool)
    ex[4, 5] = ex[6, 5] = ex[5, 4] = ex[5, 6] = True
    lab, v, _, _ = _problem(12, 14, 1, 3, unknown, ex)
    assert np.array_equal(pn.solve(lab, v), v)
    lab, v, _, _ = _problem(12, 14, 1, 3, np.ones((12, 14), bool))
    x = pn.solve(lab, v)
    assert np.isfinite(x).all() and v.min() <= x.min() and x.max() <= v.max()
    # one unknown between four fixed pixels: their mean after the first sweep
    unknown = np.zeros((12, 14), bool)
    unknown[5, 5] = True
    lab, v, _, _ = _problem(12, 14, 1, 3, unknown)
    assert pn.solve(lab, v)[0, 5, 5] == (((v[0, 4, 5] + v[0, 6, 5]) + v[0, 5, 4]) + v[0, 5, 6]) / 4.0


# ---- accuracy against the exact solve ---------------------------------------
def _image(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return ip._texture(np.random.default_rng(3), xx, yy)[None]


def _rect(H, W, i0, i1, j0, j1):
    m = np.zeros((H, W), np.uint8)
    m[i0:i1, j0:j1] = 1
    return m


ACCURACY = {
    "scene hole, grown by 1": lambda: ip.grow(ip.scene(0)[1][4], 1),
    "blob with strip 61 x 83": lambda: pn.blob_label(61, 83),
    "blob with strip 200 x 300": lambda: pn.blob_label(200, 300),
    "rectangle 324 x 432 in 540 x 960": lambda: _rect(540, 960, 100, 424, 200, 632),
    "corner 60 x 70 in 150 x 210": lambda: _rect(150, 210, 0, 60, 0, 70),
    "comb of 3-pixel stripes 150 x 210": lambda: np.maximum.reduce(
        [_rect(150, 210, k, k + 3, 5, 200) for k in range(5, 145, 6)] + [_rect(150, 210, 5, 145, 100, 103)]),
    "rectangle 342 x 607 in 1080 x 1920": lambda: _rect(1080, 1920, 300, 642, 500, 1107),
}


@pytest.mark.parametrize("name", list(ACCURACY))
def test_default_options_reach_half_a_level(name):
    """max |x - exact| <= 0.5 on a 0..255 scale with the default options, from
    a start that is off by 10 % gain + 12 with sigma = 3 noise, and already two
    cycles before the default count.  Measured per cycle (cycles 1 .. 8):
      scene hole       18    1.6   0.6    0.051  0.021  0.0017 7.5e-4 6.1e-5
      blob 61 x 83     25    4.7   0.84   0.17   0.037  0.0088 0.0021 5.1e-4
      blob 200 x 300   34    6.6   1.3    0.27   0.063  0.015  0.0035 8.6e-4
      rect 540 x 960   39    7.1   1.4    0.33   0.077  0.019  0.0046 0.0011
      corner           30    6.2   1.5    0.37   0.097  0.027  0.0079 0.0024
      comb             9.3   1.1   0.15   0.023  0.0033 4.8e-4 6.9e-5 9.9e-6
      rect 1080 x 1920 36    8.0   1.4    0.33   0.069  0.017  0.0040 9.9e-4"""
    pytest.importorskip("scipy")
    lab = ACCURACY[name]().astype(np.uint8)
    H, W = lab.shape
    v = pn.off_start(np.random.default_rng(1), _image(H, W), lab)
    ex = pn.exact(lab, v)
    errs = []
    pn.solve(lab, v, trace=lambda k, x: errs.append(float(np.abs(x - ex).max())))
    print(name, "L", pn.n_levels(H, W), " ".join(f"{e:.2g}" for e in errs))
    assert len(errs) == pn.CYCLES
    assert errs[-1] <= 0.5
    assert errs[pn.CYCLES - 3] <= 0.5  # two cycles to spare


def test_guided_solve_matches_the_exact_one():
    """With a source everywhere the solution is the source plus a membrane of
    the boundary's offset; against spsolve on the same right-hand side."""
    pytest.importorskip("scipy")
    lab = pn.blob_label(61, 83)
    tr = _image(61, 83)
    v = pn.off_start(np.random.default_rng(1), tr, lab)
    s = (0.97 * tr - 9.0).astype(np.float32).astype(np.float64)
    h = np.ones((61, 83), bool)
    ex = pn.exact(lab, v, s, h)
    x = pn.solve(lab, v, s, h)
    err = float(np.abs(x - ex).max())
    print("guided: max error", err)
    assert err <= 0.5


# ---- the blended fill on the scene, along the known flows -------------------
def _drift(frames, truth, d):
    fr = [(f.astype(np.float64) * (1.0 + d * (s - 4)) + 60.0 * d * (s - 4)).astype(np.float32)
          for s, f in enumerate(frames)]
    tr = [(f.astype(np.float64) * (1.0 + d * (s - 4)) + 60.0 * d * (s - 4)).astype(np.float32)
          for s, f in enumerate(truth)]
    return fr, tr


def _mse(outs, masks, truth, sel=None):
    """Over the pixels of the masks as drawn (and of sel), all frames pooled: (mean squared error, count)."""
    n, err = 0, 0.0
    for k, (o, m, tr) in enumerate(zip(outs, masks, truth)):
        hole = np.asarray(m) != 0
        if sel is not None:
            hole &= sel[k]
        n += int(hole.sum())
        err += float(((np.asarray(o, np.float64) - tr.astype(np.float64)) ** 2)[hole].sum())
    return err / max(n, 1), n


@pytest.fixture(scope="module")
def the_scene():
    return ip.scene(0)


def quality_gates(frames, masks, truth, plain_fn, blend_fn, label):
    """The three gates of the issue on a clip; plain_fn / blend_fn(frames, radius)
    -> (outs, statuses) with grow 1.  Returns the measured values."""
    got = {}
    for d in (0.03, 0.0):
        fr, tr = _drift(frames, truth, d)
        po, _ = plain_fn(fr, 6)
        bo, bs = blend_fn(fr, 6)
        plain, n = _mse(po, masks, tr)
        blended, _ = _mse(bo, masks, tr)
        got[d] = (plain, blended)
        print(f"{label} drift {d}: {n} hole pixels, plain MSE {plain:.3f}, blended {blended:.3f}")
        assert not any((s == ip.UNFILLED).any() for s in bs)
        assert blended < plain / 2 if d else blended <= 2 * plain
    po, ps = plain_fn(frames, 1)
    bo, bs = blend_fn(frames, 1)
    assert not any((s == ip.UNFILLED).any() for s in bs)
    src = [s == ip.FILLED for s in bs]
    spa = [s == pn.SPATIAL for s in bs]
    p_src, n_src = _mse(po, masks, truth, src)
    b_src, _ = _mse(bo, masks, truth, src)
    b_spa, n_spa = _mse(bo, masks, truth, spa)
    var = np.concatenate([t[(np.asarray(m) != 0) & s].astype(np.float64) for t, m, s in zip(truth, masks, spa)]).var()
    print(f"{label} radius 1: {n_src} sourced pixels, plain MSE {p_src:.3f}, blended {b_src:.3f}; "
          f"{n_spa} spatial pixels, MSE {b_spa:.1f}, the truth's variance there {var:.1f}")
    assert n_spa > 0 and n_src > 0
    assert b_src <= 2 * p_src
    assert b_spa < var
    got["radius1"] = (n_src, p_src, b_src, n_spa, b_spa, var)
    return got


def test_scene_quality_along_the_known_flows(the_scene):
    """inpaint_numpy.scene(0), known flows, grow 1; the 2268 pixels of the
    rectangle in all 9 frames pooled; frame s and its truth times 1 + d (s - 4)
    plus 60 d (s - 4) for the drift.  Measured: d = 0.03: plain MSE 88.41,
    blended 23.68; no drift: 0.358 and 0.357; radius 1: 612 sourced pixels,
    plain 0.470, blended 0.209; 1656 spatial pixels, MSE 969.7 against the
    truth's variance of 1719.9 over them (today's output there is the object
    itself).  Gates: blended < plain / 2 with drift, <= 2 plain without; at
    radius 1 no UNFILLED status, sourced pixels <= 2 plain, spatial pixels
    below the truth's variance."""
    frames, masks, fw, bw, truth = the_scene
    T = len(frames)

    def plain(fr, radius):
        res = [ip.fill(fr, masks, fw, bw, t, radius, 1) for t in range(T)]
        return [r[0] for r in res], [r[1] for r in res]

    def blended(fr, radius):
        res = [pn.blend(fr, masks, fw, bw, t, radius, 1) for t in range(T)]
        for (o, st), f, m in zip(res, fr, masks):
            Om = ip.grow(m, 1) != 0
            assert np.array_equal(o[~Om].view(np.uint32), f[~Om].view(np.uint32)) and (st[~Om] == ip.KEPT).all()
            assert (st[Om] != ip.KEPT).all()
        return [r[0] for r in res], [r[1] for r in res]

    quality_gates(frames, masks, truth, plain, blended, "known flows,")
