"""Generate tests/golden/weighted.npz: the reference on a damaged frame, with
the data term weighted per pixel.

Run ONLY where the read-only reference is mounted (as gen_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_weighted.py

The reference package has no data weight.  Its own code is made to compute
the weighted energy by two monkeypatches that touch nothing but the data term,
each with the weight of the pyramid level it runs on:

 - 'hs': partial_deriv's outputs (It, Ix, Iy) are multiplied by sqrt(w).  HS
   has a quadratic data penalty, so every data-term product (Ix*Ix, Ix*Iy,
   It*Ix, ...) picks up exactly w;
 - 'classic+nl-fast': flow_operator is wrapped so that, for the duration of
   the call, rho_data is a proxy whose deriv_over_x (the data term's IRLS
   weight psi) is multiplied by w.  The spatial penalties' deriv_over_x calls
   return one value per pixel as well ('sameswap'), so the call is told apart
   by the object it is made on, not by its array size; scaling those would
   make the system singular where w == 0.

The per-level weight is the reference's own _build_pyramid of the weight
plane, for the main and for the GNC pyramid, looked up by level size (the two
share the full-resolution level only, where both are the weight itself).

Setup: synth_pair(120, 160, 0); rows 40:75, cols 50:110 of frame 2 overwritten
with uniform integer noise, default_rng(1); weight 0 on that rectangle dilated
by 4 px, 0.5 on columns 0:20, 1 elsewhere.  weighted.npz holds the damaged
frame 2 (uint8), the weight, the weighted reference flows (float32) and, as
recorded results, the mean EPE to ground truth inside the rectangle and more
than 12 px away from it for the clean, damaged and damaged + weight runs.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

REF = os.environ.get("OF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import optical_flow as ref  # noqa: E402  (the reference package)
from optical_flow.methods import config as ref_cfg  # noqa: E402
from optical_flow.methods import hs as ref_hs  # noqa: E402
from optical_flow.methods.classic_nl import ClassicNLOpticalFlow  # noqa: E402

assert os.path.realpath(os.path.dirname(ref.__file__)).startswith(os.path.realpath(REF)), ref.__file__

# our own numpy-only synthetic generator (not reference code)
_spec = importlib.util.spec_from_file_location(
    "synthetic", os.path.join(HERE, "..", "..", "optical-flow-python_amd", "optical_flow", "utils", "synthetic.py"))
synthetic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synthetic)

RECT = (40, 75, 50, 110)  # rows r0:r1, cols c0:c1
DILATE = 4
FAR = 12
METHODS = ("hs", "classic+nl-fast")


def setup():
    im1, im2, gt = synthetic.synth_pair(120, 160, 0)
    r0, r1, c0, c1 = RECT
    rng = np.random.default_rng(1)
    bad = im2.copy()
    bad[r0:r1, c0:c1] = np.floor(rng.uniform(0.0, 256.0, size=(r1 - r0, c1 - c0, 3)))
    w = np.ones(im1.shape[:2])
    w[:, 0:20] = 0.5
    w[r0 - DILATE:r1 + DILATE, c0 - DILATE:c1 + DILATE] = 0.0
    return im1, im2, bad, gt, w


def regions(shape):
    r0, r1, c0, c1 = RECT
    inside = np.zeros(shape, dtype=bool)
    inside[r0:r1, c0:c1] = True
    far = np.ones(shape, dtype=bool)
    far[max(0, r0 - FAR):r1 + FAR, max(0, c0 - FAR):c1 + FAR] = False
    return inside, far


def level_weights(method, w):
    """{(h, w): weight of that level} for every level `method` visits."""
    ope = ref_cfg.load_of_method(method)
    levels = ope.pyramid_levels
    if method.startswith("hs") or getattr(ope, "auto_level", False):
        levels = ope._auto_pyramid_levels(w)
    out = {}
    pyrs = [ope._build_pyramid(w, levels, ope.pyramid_spacing)]
    if not method.startswith("hs"):
        pyrs.append(ope._build_pyramid(w, ope.gnc_pyramid_levels, ope.gnc_pyramid_spacing))
    for pyr in pyrs:
        for lv in pyr:
            assert lv.min() >= 0.0
            if lv.shape in out:
                assert np.array_equal(out[lv.shape], lv), lv.shape
            out[lv.shape] = lv
    return out


class _ScaledPenalty:
    """rho_data for the duration of one flow_operator call: deriv_over_x, one
    value per pixel in column-major order, times the level's weight."""

    def __init__(self, rho, wl):
        self._rho, self._w = rho, wl.ravel(order="F")

    def __getattr__(self, name):
        return getattr(self._rho, name)

    def deriv_over_x(self, x):
        p = self._rho.deriv_over_x(x)
        assert p.shape == self._w.shape, (p.shape, self._w.shape)
        return p * self._w


@contextlib.contextmanager
def weighted_reference(method, w):
    lw = level_weights(method, w)
    if method.startswith("hs"):
        orig = ref_hs.partial_deriv

        def pd(images, uv, *a, **k):
            s = np.sqrt(lw[images.shape[:2]])
            return tuple(d * (s if d.ndim == 2 else s[:, :, None]) for d in orig(images, uv, *a, **k))
        ref_hs.partial_deriv = pd
        try:
            yield
        finally:
            ref_hs.partial_deriv = orig
    else:
        orig = ClassicNLOpticalFlow.flow_operator

        def fo(self, uv, duv, It, Ix, Iy):
            assert It.ndim == 2  # one channel: deriv_over_x sees H * W values
            rho = self.rho_data
            self.rho_data = _ScaledPenalty(rho, lw[It.shape[:2]])
            try:
                return orig(self, uv, duv, It, Ix, Iy)
            finally:
                self.rho_data = rho
        ClassicNLOpticalFlow.flow_operator = fo
        try:
            yield
        finally:
            ClassicNLOpticalFlow.flow_operator = orig


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    im1, im2, bad, gt, w = setup()
    inside, far = regions(w.shape)
    epe = lambda uv: np.sqrt(((uv - gt) ** 2).sum(-1))  # noqa: E731
    out = {"im2_damaged": bad.astype(np.uint8), "weight": w.astype(np.float32)}
    assert np.array_equal(out["im2_damaged"].astype(np.float64), bad)
    for m in METHODS:
        runs = {"clean": quiet(ref.estimate_flow, im1, im2, m), "damaged": quiet(ref.estimate_flow, im1, bad, m)}
        with weighted_reference(m, w):
            runs["weighted"] = quiet(ref.estimate_flow, im1, bad, m)
        # the patches are gone: the reference computes what it did before
        assert np.array_equal(quiet(ref.estimate_flow, im1, bad, m), runs["damaged"]), m
        out[m] = runs["weighted"].astype(np.float32)
        for tag, uv in runs.items():
            e = epe(uv)
            out[f"{m}:{tag}:aepe_in"] = np.array(e[inside].mean())
            out[f"{m}:{tag}:aepe_far"] = np.array(e[far].mean())
            print(f"  {m:16s} {tag:9s} AEPE inside {e[inside].mean():.3f}  > {FAR} px away {e[far].mean():.3f}")
    path = os.path.join(HERE, "weighted.npz")
    np.savez_compressed(path, **out)
    print(f"wrote weighted.npz ({os.path.getsize(path) / 1024:.1f} KiB)")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
