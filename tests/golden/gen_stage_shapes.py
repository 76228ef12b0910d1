"""Generate tests/golden/stage_shapes.npz: the reference's stage functions at
degenerate and tile-seam shapes (one row, one column, planes smaller than a
stencil or a filter window, one pixel past a tile).

Run ONLY where the read-only reference is mounted (as gen_golden.py), after
the oracle library is built (the Lab guide input comes from it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_stage_shapes.py

Inputs come from tests/stage_inputs.py (our own recipe, shared with the
tests); this file only calls the reference on them.  Keys are
"s{H}x{W}:{name}", all float64:

  inputs   images, const, uv, occ, lab
  rof100, rof37   structure_texture_decomposition_rof(images, 1/8, 100, 0.95)
                  and (1/8, 37, 0.8); rof_const: the same once on `const`
                  (scale_image's hi == lo branch)
  pyr_{spacing}_{level}   compute_image_pyramid, 3 levels, base.py's kernel rule
  rs_up, rs_dn    resample_flow(uv) up by 1.6 and down by 0.5, sizes floored at 1
  {interp}_It/_Ix/_Iy     partial_deriv(images, uv, interp, filt, 0.5)
  occ_out         detect_occlusion(uv, images)
  wmf_{gray,lab}_h{7,3}   denoise_color_weighted_medfilt2(uv, guide, occ, hsz, [5, 5], sigma)
  med{3,5,7}      scipy.ndimage.median_filter(uv[..., c], size, mode='reflect') per component

The ROF variants and the 1.6x resample (180x78 of full-entropy float64) are
left out at the largest shape (113x49) to keep the file under 1 MiB; the
constant-plane ROF and the 0.5x resample stay.
"""
import os
import sys

import numpy as np

REF = os.environ.get("OF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_inputs as S  # noqa: E402  (our own input recipe)

# S.make() imports our oracle, which imports our package's struct layouts; build
# the inputs first, then let the reference package take the name optical_flow
_INPUTS = {hw: S.make(*hw) for hw in S.FIXTURE_SHAPES}
for _m in [m for m in sys.modules if m == "optical_flow" or m.startswith("optical_flow.")]:
    del sys.modules[_m]
sys.path.insert(0, REF)

import optical_flow as ref  # noqa: E402  (the reference package)
from optical_flow.utils import image_processing as ref_ip  # noqa: E402
from optical_flow.utils import pyramid as ref_pyr  # noqa: E402
from optical_flow.utils import warping as ref_warp  # noqa: E402
from optical_flow.utils import derivatives as ref_der  # noqa: E402
from optical_flow.utils import occlusion as ref_occ  # noqa: E402
from optical_flow.utils import weighted_median as ref_wm  # noqa: E402
from scipy.ndimage import median_filter  # noqa: E402

assert os.path.realpath(os.path.dirname(ref.__file__)).startswith(os.path.realpath(REF)), ref.__file__

NO_ROF = NO_RS_UP = {(113, 49)}


def stages(H, W, d):
    out = {k: d[k] for k in ("images", "const", "uv", "occ", "lab")}
    images, uv = d["images"], d["uv"]
    if (H, W) not in NO_ROF:
        for name, (theta, iters, alp) in S.ROF_CASES.items():
            out[name] = ref_ip.structure_texture_decomposition_rof(images, theta, iters, alp)
    out["rof_const"] = ref_ip.structure_texture_decomposition_rof(d["const"], 1 / 8, 100, 0.95)
    for sp in S.PYR_SPACINGS:
        sig = np.sqrt(sp) / np.sqrt(2)  # the kernel rule of the reference's _build_pyramid
        f = ref_ip.fspecial_gaussian(int(2 * round(1.5 * sig) + 1), sig)
        for lv, a in enumerate(ref_pyr.compute_image_pyramid(images, f, S.PYR_LEVELS, 1.0 / sp)):
            if lv:
                out[f"pyr_{sp}_{lv}"] = a
    for name, sz in S.resample_sizes(H, W).items():
        if name == "up" and (H, W) in NO_RS_UP:
            continue
        out[f"rs_{name}"] = ref_warp.resample_flow(uv, sz)
    assert not S.near_threshold(uv).any(), (H, W, "pick another FLOW_SEED")
    for m in S.INTERPS:
        for got, name in zip(ref_der.partial_deriv(images, uv, m, S.FILT, 0.5), ("It", "Ix", "Iy")):
            out[f"{m}_{name}"] = got
    out["occ_out"] = ref_occ.detect_occlusion(uv, images)
    for name, (guide, hsz, sig) in S.WMF_CASES.items():
        g = d["lab"] if guide == "lab" else images[..., 0]
        out[name] = ref_wm.denoise_color_weighted_medfilt2(uv, g, d["occ"], hsz, [5, 5], sig)
    for sz in S.MEDIAN_SIZES:
        out[f"med{sz}"] = np.stack([median_filter(uv[..., c], size=sz, mode="reflect") for c in range(2)], axis=2)
    return out


def main():
    out = {}
    for (H, W) in S.FIXTURE_SHAPES:
        for k, v in stages(H, W, _INPUTS[(H, W)]).items():
            v = np.asarray(v)
            assert v.dtype == np.float64 and np.all(np.isfinite(v)), (H, W, k, v.dtype)
            out[f"{S.tag(H, W)}:{k}"] = v
    path = os.path.join(HERE, "stage_shapes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote stage_shapes.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays)")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
