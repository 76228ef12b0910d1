"""Inputs of the stage shape sweep (tests/test_gpu_stage_shapes.py,
tests/test_oracle_shapes_cpu.py) and of its fixture generator
(tests/golden/gen_stage_shapes.py): one deterministic recipe per (H, W), so
that the fixture's inputs and the inputs a test builds at a shape the fixture
does not hold come from the same place.

Everything is numpy; every float input is float32-representable (the GPU
wrappers round to float32, the float64 checkers then see the same numbers).
"""
import numpy as np

FILT = np.array([1, -8, 0, 8, -1]) / 12.0

# shapes held by tests/golden/stage_shapes.npz
FIXTURE_SHAPES = [(1, 70), (70, 1), (2, 3), (3, 3), (5, 49), (9, 17), (113, 49)]

# Seed of the flow per shape.  A seed is admitted when no warped coordinate
# x + u, y + v (fp64, 1-based) lies within 1e-3 px of an in/out-of-bounds
# threshold (1, W, 1, H) -- near_threshold() below; checked on the CPU by the
# generator and by test_oracle_shapes_cpu.py.  Shapes not listed use H * W.
# (2,3) and (3,3): the admitted seed below 400 past H * W that leaves the most
# samples in bounds (4 of 6 and 5 of 9 pixels; H * W itself leaves 0 and 1).
FLOW_SEED = {(113, 49): 5539, (2, 3): 297, (3, 3): 19}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def tag(H, W):
    return f"s{H}x{W}"


def frames(H, W, seed):
    """Two integer-valued RGB frames in 0..255: a few plane waves (structure)
    plus +-40 of per-pixel, per-channel noise (texture, and colour that keeps
    every Lab channel's range wide on a plane of six pixels); frame 2 is the
    same field 1.3 px right and 0.7 px up with its own noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(float)
    K = 4
    f = rng.uniform(0.05, 0.4, (3, K))
    th = rng.uniform(0, 2 * np.pi, (3, K))
    ph = rng.uniform(0, 2 * np.pi, (3, K))
    out = []
    for dx, dy in ((0.0, 0.0), (1.3, -0.7)):
        im = np.empty((H, W, 3))
        for c in range(3):
            acc = sum(np.sin(f[c, k] * ((x - dx) * np.cos(th[c, k]) + (y - dy) * np.sin(th[c, k])) + ph[c, k])
                      for k in range(K))
            im[..., c] = 128.0 + 30.0 * acc + rng.integers(-40, 41, (H, W))
        out.append(np.floor(np.clip(im, 0, 255) + 0.5))
    return out


def flow(H, W, seed):
    """sigma = 1.5 px: samples leave the plane on every side.  Multiples of
    2^-16 px up to 128 rows / columns and of 2^-10 px above (up to 8192): the
    flow and the warped coordinate j + 1 + u are then exact in float32, so a
    float32 kernel and a float64 checker interpolate at the same point (the
    rounding of a coordinate near 4096, 2.4e-4 px, times a gradient of tens
    of grey levels per pixel would use up partial_deriv's 5e-3 by itself)."""
    q = 65536.0 if max(H, W) <= 128 else 1024.0
    return np.round(np.random.default_rng(seed).normal(0.0, 1.5, (H, W, 2)) * q) / q


def near_threshold(uv, eps=1e-3):
    """Pixels whose warped coordinate is within eps of 1, W (x) or 1, H (y):
    the only places where partial_deriv is discontinuous in the flow."""
    H, W = uv.shape[:2]
    xg, yg = np.meshgrid(np.arange(1, W + 1.0), np.arange(1, H + 1.0))
    x2, y2 = xg + uv[..., 0], yg + uv[..., 1]
    return ((np.abs(x2 - 1) <= eps) | (np.abs(x2 - W) <= eps) | (np.abs(y2 - 1) <= eps) | (np.abs(y2 - H) <= eps))


def make(H, W):
    """dict of inputs at (H, W): rgb1, rgb2, images (two gray frames),
    const (a constant plane), uv, occ (weighted-median occlusion weights) and
    lab (frame 1's Lab, each channel scaled to 0..255, from the oracle, whose
    rgb2lab is pinned to the reference at 1e-11).  occ and lab are rounded to
    multiples of 2^-10 and 2^-6: exact in float32, and small in the fixture."""
    import oracle as O
    seed = FLOW_SEED.get((H, W), H * W)
    rgb1, rgb2 = frames(H, W, 1000 + 7 * H + W)
    images = np.stack([rgb1[..., 1], rgb2[..., 1]], axis=2)
    rng = np.random.default_rng(2000 + 7 * H + W)
    occ = rng.uniform(0.0, 1.0, (H, W))
    occ[: max(1, H // 5), : max(1, W // 4)] = 0.0  # weights at the 1e-10 floor
    lab = O.rgb2lab(rgb1)
    for c in range(3):
        lab[..., c] = O.scale_image(lab[..., c], 0, 255)
    return {"rgb1": rgb1, "rgb2": rgb2, "images": images, "const": np.full((H, W), 93.0), "uv": flow(H, W, seed),
            "occ": np.round(occ * 1024) / 1024, "lab": np.round(lab * 64) / 64}


def rof_texture_f32(im, theta, iters, alp):
    """structure_texture_decomposition_rof restated in plain numpy float32,
    whole planes at a time (no tiles, no halo): what float32 alone costs
    against the float64 oracle.  The yardstick of the ROF seam bound."""
    f = np.float32

    def scale(a, lo, hi):
        mn, mx = a.min(), a.max()
        if mn == mx:
            return np.full_like(a, f((lo + hi) / 2))
        return (a - mn) / (mx - mn) * f(hi - lo) + f(lo)

    im = np.asarray(im, dtype=f)
    x = scale(im[..., None] if im.ndim == 2 else im, -1, 1)
    th, dl, al = f(theta), f(1.0 / (4.0 * theta)), f(alp)
    out = np.empty_like(x)
    for c in range(x.shape[2]):
        I = x[..., c]
        px, py = np.zeros_like(I), np.zeros_like(I)

        def div():
            d = px + py
            d[:, 1:] -= px[:, :-1]
            d[1:, :] -= py[:-1, :]
            return d
        for _ in range(iters):
            u = I + th * div()
            gx, gy = np.zeros_like(I), np.zeros_like(I)
            gx[:, :-1] = u[:, 1:] - u[:, :-1]
            gy[:-1, :] = u[1:, :] - u[:-1, :]
            a, b = px + dl * gx, py + dl * gy
            n = np.maximum(np.sqrt(a * a + b * b), f(1))
            px, py = a / n, b / n
        out[..., c] = I - al * (I + th * div())
    out = scale(out, 0, 255).astype(np.float64)
    return out[..., 0] if im.ndim == 2 else out


def rof_seam_band(H, W, tw=48, th=112, k=8):
    """(H, W) mask of the pixels within k of a seam between two k_rof_iters
    tiles (ROF_TW x ROF_TH = 48 x 112 outputs, ROF_K = 8 halo)."""
    def near(n, t):  # indices in [seam - k, seam + k) for the seams t, 2t, ... < n
        x, seams = np.arange(n), np.arange(t, n, t)
        return ((x[:, None] >= seams[None, :] - k) & (x[:, None] < seams[None, :] + k)).any(axis=1)
    return near(H, th)[:, None] | near(W, tw)[None, :]


# ROF, pixels within 8 of a tile seam: 2 x the largest error of rof_texture_f32
# against the oracle over the shapes of the sweep that have a seam, measured
# on the CPU (100 / 37 iterations): 4.93e-5 / 6.02e-5 at 113x49, 4.45e-5 /
# 3.78e-5 at 5x49, 4.52e-5 / 3.78e-5 at 37x65, 5.69e-5 / 4.37e-5 at 60x1100,
# 4.13e-5 at 130x4100 (37).  Another summation order of the same float32
# arithmetic moves each figure by ~10 %.  test_oracle_shapes_cpu.py::
# test_rof_plain_float32 holds the restatement to half the bound.
ROF_SEAM_TOL = 2 * 6.02e-5


def pyramid_kernel(spacing):
    """The smoothing kernel rule of methods/base.py's _build_pyramid."""
    from optical_flow.utils.image_processing import fspecial_gaussian
    sig = np.sqrt(spacing) / np.sqrt(2.0)
    return fspecial_gaussian(int(2 * round(1.5 * sig) + 1), sig)


def resample_sizes(H, W):
    """Up by 1.6 and down by 0.5, floored at 1."""
    return {"up": (max(1, int(H * 1.6)), max(1, int(W * 1.6))), "dn": (max(1, int(H * 0.5)), max(1, int(W * 0.5)))}


# stage parameters shared by the generator and the tests
ROF_CASES = {"rof100": (1 / 8, 100, 0.95), "rof37": (1 / 8, 37, 0.8)}
PYR_SPACINGS = (2.0, 1.25)
PYR_LEVELS = 3
INTERPS = ("bi-cubic", "cubic", "bi-linear")
WMF_CASES = {"wmf_gray_h7": ("gray", 7, 7.0), "wmf_gray_h3": ("gray", 3, 4.0),
             "wmf_lab_h7": ("lab", 7, 7.0), "wmf_lab_h3": ("lab", 3, 4.0)}
MEDIAN_SIZES = (3, 5, 7)
