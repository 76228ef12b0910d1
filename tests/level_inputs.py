"""Inputs of the level shape sweep (tests/test_gpu_level_shapes.py,
tests/test_level_shapes_cpu.py): stage_inputs.make(H, W) -- the same frames
and flows -- plus what one level's warping loop needs beyond a single stage:
three-channel frames, the Lab guide, a data-weight plane, an increment field
x for the update kernel, and the arms of the level itself.

Everything is numpy and deterministic per (H, W); every float input is
float32-representable.
"""
import numpy as np

import stage_inputs as S

SMALL = [(1, 70), (70, 1), (2, 3), (3, 3), (5, 49), (113, 49), (112, 48), (37, 65)]
BIG = (130, 4100)
WMF_SHAPES = SMALL + [(9, 17)]
PITCH = 64  # rows of a device plane start at multiples of 64 elements (of_pitch)


def pitch(W):
    return (W + PITCH - 1) // PITCH * PITCH


def weight_plane(H, W):
    """Like test_gpu_weight._random_weight: [0, 2] with 15 % exact zeros, and
    a one, a zero and a two at fixed places so that every plane of >= 3
    pixels has all three (a value above 1 included) whatever the draw."""
    rng = np.random.default_rng(4000 + 7 * H + W)
    w = rng.uniform(0.0, 2.0, (H, W)).astype(np.float32)
    w[rng.uniform(size=(H, W)) < 0.15] = 0.0
    f = w.reshape(-1)
    if f.size >= 3:
        f[0], f[f.size // 2], f[-1] = 1.0, 0.0, 2.0
    return w.astype(np.float64)


def smooth_flow(H, W):
    """A flow whose divergence is small (the occlusion map of uv + x is then
    not ~0 everywhere, as it is for stage_inputs' sigma 1.5 px noise) and
    whose components are well away from 0: a constant (0.75, -0.5) px, a plane
    wave of 0.25 px and 0.02 px of noise.  Multiples of 2^-16 px up to 128
    rows / columns and of 2^-10 px above, like stage_inputs.flow and for its
    reason: j + u + clip(x) is then exact in float32, so the kernel and the
    float64 checker sample frame 2 at the same point."""
    rng = np.random.default_rng(5000 + 7 * H + W)
    y, x = np.mgrid[0:H, 0:W].astype(float)
    u = 0.75 + 0.25 * np.sin(0.21 * x + 0.13 * y) + rng.normal(0, 0.02, (H, W))
    v = -0.5 + 0.25 * np.cos(0.17 * x - 0.19 * y) + rng.normal(0, 0.02, (H, W))
    q = _quantum(H, W)
    return np.round(np.stack([u, v], axis=2) * q) / q


def _quantum(H, W):
    return 65536.0 if max(H, W) <= 128 else 1024.0


# where the forced |x| > 1 increments go: (row, column) as fractions of the
# last index.  Column 0, column W - 1, row 0 and the first pixel of a row --
# the places whose left / upper neighbour k_update_occ recomputes across a row
# start or a pitch.
_FORCED = [((0.0, 0.0), (1.75, -1.5)), ((0.0, 1.0), (-1.25, 2.0)), ((1.0, 0.0), (1.5, 1.25)),
           ((0.5, 0.0), (-2.0, 1.5)), ((0.0, 0.5), (1.5, -1.25)), ((0.5, 1.0), (1.25, -1.75))]


def forced_positions(H, W):
    return sorted({(int(round(a * (H - 1))), int(round(b * (W - 1)))) for (a, b), _ in _FORCED})


def increment(H, W):
    """x: sigma 0.1 px of noise in multiples of 2^-12 px (2^-10 px above 128
    rows / columns; |x| < 1), both components beyond +-1 at
    forced_positions(H, W), and one pixel that is not forced (if the plane has
    one) set to (0.25, -0.5)."""
    rng = np.random.default_rng(6000 + 7 * H + W)
    q = min(4096.0, _quantum(H, W))
    x = np.round(rng.normal(0.0, 0.1, (H, W, 2)) * q) / q
    for (a, b), val in _FORCED:
        x[int(round(a * (H - 1))), int(round(b * (W - 1)))] = val
    forced = set(forced_positions(H, W))
    free = [(i, j) for i in range(H - 1, -1, -1) for j in range(W - 1, -1, -1) if (i, j) not in forced]
    if free:
        x[free[0]] = (0.25, -0.5)
    return x


def make(H, W):
    """stage_inputs.make(H, W) plus images3 (the RGB planes of both frames,
    (H, W, 6)), guide (the Lab planes), weight, uvs (smooth_flow) and x."""
    d = dict(S.make(H, W))
    if H == 1 or W == 1:
        # One row / column: a sample stays in the plane only if its flow
        # across the plane is exactly 0, which stage_inputs' flow never is, so
        # every derivative would be 0 and no data term would be assembled.
        # Every second pixel gets that component zeroed (the warped
        # coordinate is then exactly on the plane, in float32 as in float64).
        uv = d["uv"].copy()
        uv[::2 if W == 1 else 1, ::2 if H == 1 else 1, 1 if H == 1 else 0] = 0.0
        d["uv"] = uv
    d["images3"] = np.concatenate([d["rgb1"], d["rgb2"]], axis=2)
    d["guide"] = d["lab"]
    d["weight"] = weight_plane(H, W)
    d["uvs"] = smooth_flow(H, W)
    d["x"] = increment(H, W)
    return d


# ---- the arms of the level -------------------------------------------------
# (name, registry method, attribute overrides, guide, nc, weighted).  Two outer
# iterations each: the second starts from the first's output, in whichever
# buffer the loop left it.
_N = {"max_iters": 2, "max_warping_iters": 2}
ARMS = [
    ("hs mf1 clip", "hs", dict(mf_iter=1, limit_update=True), None, 1, False),
    ("hs mf2 noclip", "hs", dict(mf_iter=2, limit_update=False), None, 1, False),
    ("hs mf2 clip weighted", "hs", dict(mf_iter=2, limit_update=True), None, 1, True),
    ("hs exit", "hs", dict(mf_iter=1, limit_update=True, interpolation_method="bi-linear"), None, 1, False),
    ("ba a1 lin1 mf5", "ba", dict(alpha=1.0, max_linear=1, median_filter_size=[5, 5]), None, 1, False),
    ("ba a0 lin2 mf3", "ba", dict(alpha=0.0, max_linear=2, median_filter_size=[3, 3]), None, 1, False),
    ("classic-c a0 lin1 mf3", "classic-c", dict(alpha=0.0, max_linear=1, median_filter_size=[3, 3]), None, 1, False),
    ("classic-c a1 lin2 mf5", "classic-c", dict(alpha=1.0, max_linear=2, median_filter_size=[5, 5]), None, 1, False),
    ("ba a0 lin2 mf3 weighted", "ba", dict(alpha=0.0, max_linear=2, median_filter_size=[3, 3]), None, 1, True),
    ("classic-c a0 lin1 mf5 rgb", "classic-c", dict(alpha=0.0, max_linear=1, median_filter_size=[5, 5]), None, 3,
     False),
    ("classic+nl a0 lin1", "classic+nl", dict(alpha=0.0, max_linear=1), "lab", 1, False),
    ("classic+nl-fast a1 lin2", "classic+nl-fast", dict(alpha=1.0, max_linear=2), "lab", 1, False),
    ("classic+nl a0 lin1 nomf", "classic+nl", dict(alpha=0.0, max_linear=1, median_filter_size=None), "lab", 1,
     False),
    ("classic+nl a0 lin2 weighted", "classic+nl", dict(alpha=0.0, max_linear=2), "lab", 1, True),
]
ARM_NAMES = [a[0] for a in ARMS]


def arm(name, H, W, d=None):
    """(ope, images, guide, uv0, weight) of an arm at (H, W).  'hs exit': two
    equal frames, a zero flow and bilinear interpolation (which returns the
    frame itself at a zero flow, in float32 as in float64), so the first
    solve's right-hand side and x are exactly 0 and the loop leaves at
    hs.py:127."""
    from optical_flow.methods.config import load_of_method
    _, meth, over, guide, nc, weighted = ARMS[ARM_NAMES.index(name)]
    d = make(H, W) if d is None else d
    o = load_of_method(meth)
    o.parse_input_parameter({**_N, **over})
    o.display = False
    images = d["images"] if nc == 1 else d["images3"]
    uv0 = d["uv"]
    if name == "hs exit":
        images = np.concatenate([images[..., :nc], images[..., :nc]], axis=2)
        uv0 = np.zeros_like(uv0)
    g = d["guide"] if guide == "lab" else None
    o.images = images
    o.color_images = g
    return o, images, g, uv0, (d["weight"] if weighted else None)
