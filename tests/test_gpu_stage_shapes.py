"""GPU stage parity at tile-seam and degenerate shapes: the image and flow
stage kernels through the public Python wrappers,
against the float64 oracle on the same float32-representable inputs and, at
the shapes tests/golden/stage_shapes.npz holds, against the reference.

test_gpu_stages.py checks these kernels at one 37x53 crop.  The shapes here
are the ones at which their shape-dependent code takes another path:

  (1,70) (70,1)   one row / column: ext_reflect / ext_mirror with n == 1,
                  k_resize with W - 1 == 0, ROF's first and last row / column
                  guards on the same pixel; (1,70) also crosses an OF_BX block
  (2,3) (3,3)     (2,3) is below the 5-tap radius: the general k_correlate
                  with multi-fold reflection; (3,3) the smallest k_correlate_k;
                  both narrower than OF_BSPL_K and the weighted-median window
  (5,49)          ROF_TW + 1: the second ROF column tile owns one column
  (113,49)        ROF_TH + 1: the second ROF row tile owns one row
  (112,48) (37,65)  exactly one ROF tile; OF_BX + 1 columns
  (9,17)          weighted median only: WMF_T + 1 rows, 2 WMF_T + 1 columns
  (60,1100)       _preprocess and ROF: 18 x 15 blocks against k_minmax's
                  256-block cap, a grid-stride pass
  (130,4100)      every grid2 kernel: 65 x 31 = 2015 blocks for 33 block rows,
                  a second stride pass with nt & 7 == 7; 86 x 2 ROF tiles

Tolerances are test_gpu_stages.py's.  Inputs: tests/stage_inputs.py.  The
flow is a multiple of 2^-16 px (2^-10 px at 4100 columns), so the warped
coordinate j + 1 + u is exact in float32 at every shape: what is left is the
arithmetic of the kernels, not the rounding of a coordinate near 4096, and a
row or column of wrong pixels at a seam stands out against it.

Every test prints a line "stage_shapes | stage | shape | figure".
"""
import functools

import numpy as np
import pytest

import oracle as O
import stage_inputs as S

pytestmark = pytest.mark.gpu

SMALL = [(1, 70), (70, 1), (2, 3), (3, 3), (5, 49), (113, 49), (112, 48), (37, 65)]
WIDE = (60, 1100)
BIG = (130, 4100)
OP_METHODS = [("classic+nl", 0.0), ("hs", 0.0), ("classic-c", 0.0)]


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


def _say(stage, hw, fig):
    print(f"stage_shapes | {stage} | {hw[0]}x{hw[1]} | {fig}")


@functools.lru_cache(maxsize=None)
def _in(H, W):
    d = S.make(H, W)
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def fx(golden):
    d = golden("stage_shapes.npz")

    def at(H, W):
        t = S.tag(H, W) + ":"
        out = {k[len(t):]: v for k, v in d.items() if k.startswith(t)}
        if out:  # same inputs, or the comparison means nothing
            for k in ("images", "uv", "occ", "lab"):
                np.testing.assert_array_equal(out[k], _in(H, W)[k])
        return out
    return at


def _check(got, refs, atol, stage, hw):
    """got vs every (name, ref) in refs, absolute."""
    errs = []
    for name, ref in refs:
        assert got.shape == ref.shape, (stage, name, got.shape, ref.shape)
        errs.append((name, float(np.abs(got - ref).max()) if ref.size else 0.0))
    _say(stage, hw, " ".join(f"{n} {e:.2e}" for n, e in errs))
    for name, e in errs:
        assert e <= atol, (stage, hw, name, e)


# ---- _preprocess ------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL + [WIDE, BIG], ids=_ids(SMALL + [WIDE, BIG]))
def test_preprocess(H, W):
    from optical_flow.interface import _preprocess
    d = _in(H, W)
    gray, lab = _preprocess(d["rgb1"], d["rgb2"])
    ref = O.rgb2lab(d["rgb1"])
    for c in range(3):
        ref[..., c] = O.scale_image(ref[..., c], 0, 255)
    g1, g2 = O.rgb2gray(d["rgb1"]), O.rgb2gray(d["rgb2"])
    e = np.abs(np.moveaxis(lab, 0, 2) - ref).max()
    _say("preprocess", (H, W), f"gray differing px {int((gray[0] != g1).sum() + (gray[1] != g2).sum())} lab {e:.2e}")
    np.testing.assert_array_equal(gray[0], g1)  # integer-valued: exact
    np.testing.assert_array_equal(gray[1], g2)
    assert e <= 255 * 2e-5, e


# ---- ROF --------------------------------------------------------------------
def _rof_cases(hw):
    return ["rof37"] if hw == BIG else ["rof100", "rof37"]


@pytest.mark.parametrize("H,W,case", [(h, w, c) for (h, w) in SMALL + [WIDE, BIG] for c in _rof_cases((h, w))])
def test_rof(fx, H, W, case):
    """2e-3 everywhere, as test_gpu_stages.py.  That bound cannot see a halo
    that is a pixel short: what a launch of ROF_K + 1 iterations gets wrong in
    a tile's first owned row or column has passed through 9 updates that each
    scale it by at most theta * delta = 1/4, 4^-9 = 3.8e-6 of a dual variable
    <= 1, about 1e-4 of the 0..255 texture (measured with that mutant:
    profiles/stage_shapes.md).  So the pixels within 8 of a tile seam are also
    held to S.ROF_SEAM_TOL, twice what plain float32 costs (stage_inputs.py)."""
    from optical_flow.utils.image_processing import structure_texture_decomposition_rof as rof
    theta, iters, alp = S.ROF_CASES[case]
    im = _in(H, W)["images"]
    ref = O.rof_texture(im, theta, iters, alp)
    refs = [("oracle", ref)]
    if case in fx(H, W):
        refs.append(("reference", fx(H, W)[case]))
    got = rof(im, theta, iters, alp)
    _check(got, refs, 2e-3, case, (H, W))
    band = S.rof_seam_band(H, W)
    if band.any():
        e = float(np.abs(got - ref)[band].max())
        _say(case + " seam band", (H, W), f"oracle {e:.2e} over {int(band.sum())} px")
        assert e <= S.ROF_SEAM_TOL, e


@pytest.mark.parametrize("H,W", SMALL, ids=_ids(SMALL))
def test_rof_constant_plane(fx, H, W):
    """hi == lo in scale_image: the reference's answer is the midpoint."""
    from optical_flow.utils.image_processing import structure_texture_decomposition_rof as rof
    c = _in(H, W)["const"]
    refs = [("oracle", O.rof_texture(c, 1 / 8, 100, 0.95))]
    if "rof_const" in fx(H, W):
        refs.append(("reference", fx(H, W)["rof_const"]))
    _check(rof(c, 1 / 8, 100, 0.95), refs, 2e-3, "rof_const", (H, W))


# ---- pyramid ----------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL + [BIG], ids=_ids(SMALL + [BIG]))
def test_pyramid(fx, H, W):
    from optical_flow.utils.pyramid import compute_image_pyramid
    im = _in(H, W)["images"]
    levels = 2 if (H, W) == BIG else S.PYR_LEVELS  # one step at 130x4100
    figs = []
    for sp in S.PYR_SPACINGS:
        f = S.pyramid_kernel(sp)
        p = compute_image_pyramid(im, f, levels, 1.0 / sp)
        o = O.pyramid(im, f, levels, 1.0 / sp)
        for lv in range(1, levels):
            assert p[lv].shape == o[lv].shape, (sp, lv, p[lv].shape, o[lv].shape)
            errs = [np.abs(p[lv] - o[lv]).max()]
            if f"pyr_{sp}_{lv}" in fx(H, W):
                errs.append(np.abs(p[lv] - fx(H, W)[f"pyr_{sp}_{lv}"]).max())
            figs.append((sp, lv, p[lv].shape[:2], max(errs)))
    _say("pyramid", (H, W), " ".join(f"{sp}/{lv} {s[0]}x{s[1]} {e:.2e}" for sp, lv, s, e in figs))
    for sp, lv, s, e in figs:
        assert e <= 2e-4 * 255, (sp, lv, s, e)


# ---- resample_flow ----------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL + [BIG], ids=_ids(SMALL + [BIG]))
def test_resample_flow(fx, H, W):
    from optical_flow.utils.warping import resample_flow
    uv = _in(H, W)["uv"]
    for name, sz in S.resample_sizes(H, W).items():
        if (H, W) == BIG and name == "up":
            continue
        refs = [("oracle", O.resample_flow(uv, sz))]
        if f"rs_{name}" in fx(H, W):
            refs.append(("reference", fx(H, W)[f"rs_{name}"]))
        _check(resample_flow(uv, sz), refs, 2e-5, f"resample_{name} {sz[0]}x{sz[1]}", (H, W))


# ---- partial_deriv ----------------------------------------------------------
@pytest.mark.parametrize("H,W,method", [(h, w, m) for (h, w) in SMALL for m in S.INTERPS] +
                         [BIG + ("bi-cubic",), BIG + ("cubic",)])
def test_partial_deriv(fx, H, W, method):
    """Every pixel whose fp64 warped coordinate is more than 1e-3 px from an
    in/out-of-bounds threshold meets 5e-3 + 1e-5 |ref|; the excluded share is
    0 below 200 px (the flow seeds are chosen so) and <= 0.5 % above."""
    from optical_flow.utils.derivatives import partial_deriv
    d = _in(H, W)
    skip = S.near_threshold(d["uv"])
    assert skip.sum() <= (0 if H * W < 200 else 0.005 * H * W), skip.sum()
    out = partial_deriv(d["images"], d["uv"], method, S.FILT, 0.5)
    ref = O.partial_deriv(d["images"], d["uv"], method, S.FILT, 0.5)
    worst, nz = 0.0, 0
    for got, r, name in zip(out, ref, ("It", "Ix", "Iy")):
        cmp = [r] + ([fx(H, W)[f"{method}_{name}"]] if f"{method}_{name}" in fx(H, W) else [])
        for rr in cmp:
            err = np.abs(got - rr)
            bad = (err > 5e-3 + 1e-5 * np.abs(rr)) & ~skip
            worst = max(worst, float(err[~skip].max()) if (~skip).any() else 0.0)
            assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], float(err[bad].max()))
        nz += int((r != 0).sum())
    _say(f"partial_deriv {method}", (H, W), f"max err {worst:.2e} excluded {int(skip.sum())} nonzero ref {nz}")


# ---- flow operator ----------------------------------------------------------
@pytest.mark.parametrize("meth,alpha", OP_METHODS, ids=[m for m, _ in OP_METHODS])
@pytest.mark.parametrize("H,W", SMALL + [BIG], ids=_ids(SMALL + [BIG]))
def test_operator_planes(H, W, meth, alpha):
    """The elementwise bounds of test_gpu_stages.test_flow_operator's oracle
    half.  The flow is its own (sigma 0.7 px, generic float32, as there)."""
    from optical_flow.methods.config import load_of_method
    d = _in(H, W)
    uv = S.f32(np.random.default_rng(3000 + 7 * H + W).normal(0, 0.7, (H, W, 2)))
    It, Ix, Iy = (S.f32(a) for a in O.partial_deriv(d["images"], uv, "cubic" if meth == "hs" else "bi-cubic",
                                                    S.FILT, 0.5))
    o = load_of_method(meth)
    o.images = d["images"]
    coef, rhs = o._operator_planes(uv, None, It, Ix, Iy, alpha)
    oc, orhs = O.flow_operator(o.to_params(), alpha, uv, None, It, Ix, Iy)
    scale = np.abs(oc).max(axis=(1, 2), keepdims=True)
    bscale = np.abs(orhs).max()
    ec = np.abs(coef - oc) / (1e-4 * np.abs(oc) + 1e-6 * scale + 1e-300)
    eb = np.abs(rhs - orhs) / (1e-4 * np.abs(orhs) + 2e-5 * bscale + 1e-300)
    _say(f"operator {meth}", (H, W), f"coef {ec.max():.3f} rhs {eb.max():.3f} of the bound")
    assert np.all(np.abs(coef - oc) <= 1e-4 * np.abs(oc) + 1e-6 * scale), np.abs(coef - oc).max()
    assert np.all(np.abs(rhs - orhs) <= 1e-4 * np.abs(orhs) + 2e-5 * bscale)


# ---- occlusion ---------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL + [BIG], ids=_ids(SMALL + [BIG]))
def test_occlusion(fx, H, W):
    from optical_flow.utils.occlusion import detect_occlusion
    d = _in(H, W)
    refs = [("oracle", O.detect_occlusion(d["uv"], d["images"]))]
    if "occ_out" in fx(H, W):
        refs.append(("reference", fx(H, W)["occ_out"]))
    _check(detect_occlusion(d["uv"], d["images"]), refs, 1e-5, "occlusion", (H, W))


# ---- weighted median ---------------------------------------------------------
def _mirror(i, n):
    """Whole-sample reflection of an index array (np.pad 'reflect', any fold)."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


WMF_SHAPES = SMALL + [(9, 17)]


@pytest.mark.parametrize("guide,hsz,sig", [("gray", 7, 7.0), ("lab", 7, 7.0), ("gray", 3, 4.0), ("lab", 3, 4.0),
                                           ("gray", 0, 7.0), ("lab", 0, 7.0)])
@pytest.mark.parametrize("H,W", WMF_SHAPES, ids=_ids(WMF_SHAPES))
def test_weighted_median(fx, H, W, guide, hsz, sig):
    """>= 99.9 % of the values exact with >= 1000 of them, at most one
    non-exact value below; every non-exact value is an input flow value of
    that pixel's window (a neighbouring order statistic)."""
    from optical_flow.utils.weighted_median import denoise_color_weighted_medfilt2
    d = _in(H, W)
    g = d["lab"] if guide == "lab" else d["images"][..., 0]
    out = denoise_color_weighted_medfilt2(d["uv"], g, d["occ"], hsz, [5, 5], sig)
    refs = [O.weighted_median(d["uv"], g, d["occ"], hsz, sig)]
    key = f"wmf_{guide}_h{hsz}"
    if key in fx(H, W):
        np.testing.assert_array_equal(refs[0], fx(H, W)[key])  # the oracle is exact here (CPU pin)
        refs.append(fx(H, W)[key])
    ref = refs[0]
    assert out.shape == ref.shape
    same = np.abs(out - ref) <= 1e-6 * (1 + np.abs(ref))
    _say(f"wmf {guide} hsz {hsz}", (H, W), f"exact {int(same.sum())}/{same.size}")
    if same.size >= 1000:
        assert same.mean() >= 0.999, same.mean()
    else:
        assert (~same).sum() <= 1, np.argwhere(~same)
    off = np.arange(-hsz, hsz + 1)
    for i, j, c in np.argwhere(~same):
        win = d["uv"][np.ix_(_mirror(i + off, H), _mirror(j + off, W))][..., c]
        assert (win == out[i, j, c]).any(), (i, j, c, out[i, j, c], ref[i, j, c])


# ---- median -------------------------------------------------------------------
@pytest.mark.parametrize("H,W,size", [(h, w, z) for (h, w) in SMALL for z in S.MEDIAN_SIZES] + [BIG + (5,)])
def test_median(fx, H, W, size):
    """median_filter2 runs k_median1<size>; k_median2<size> (the float2 form
    the solve uses) has no stage wrapper and stays with the end-to-end tests."""
    from optical_flow.utils.weighted_median import median_filter2
    uv = _in(H, W)["uv"]
    refs = [("oracle", O.median_filter(uv, size))]
    if f"med{size}" in fx(H, W):
        refs.append(("reference", fx(H, W)[f"med{size}"]))
    _check(median_filter2(uv, size), refs, 1e-6, f"median {size}", (H, W))
