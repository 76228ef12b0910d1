"""Deterministic synthetic image pairs with analytic ground-truth flow.

numpy-only so the GPU box can regenerate the benchmark inputs without scipy.
Recipe follows SURVEY.md §8(d) (``synth_pair``): per RGB channel, K=32 plane
waves; frame 2 samples the same field at (x - u, y - v); ground truth
u = 2 sin(2*pi*y/H) + 0.5, v = 1.5 cos(2*pi*x/W) - 0.25.
"""
import numpy as np


def _field(x, y, f, th, ph):
    K = f.shape[1]
    out = np.empty(x.shape + (3,))
    for c in range(3):
        acc = np.zeros(x.shape)
        for k in range(K):
            acc += np.sin(f[c, k] * (x * np.cos(th[c, k]) + y * np.sin(th[c, k])) + ph[c, k])
        out[..., c] = 128.0 + 40.0 * acc / np.sqrt(K)
    return out


def synth_gt(H, W):
    """Analytic ground-truth flow (H, W, 2) for :func:`synth_pair`."""
    y, x = np.mgrid[0:H, 0:W].astype(float)
    u = 2.0 * np.sin(2.0 * np.pi * y / H) + 0.5
    v = 1.5 * np.cos(2.0 * np.pi * x / W) - 0.25
    return np.stack([u, v], axis=2)


def two_layer_pair(H, W, seed=0, K=32, bg=(0.5, 0.0), fg=(3.0, -2.0)):
    """Return (im1, im2, gt, mask): a pair with a motion boundary.  A textured
    background (plane waves around gray level 95) moves by `bg`, a brighter
    textured rectangle (around 175; rows H//4 .. 3H//4-1, columns W//3 ..
    2W//3-1 of frame 1) moves by `fg` = (u, v), whole pixels, in front of it.
    Frames are float64 RGB with integer values in [0, 255]; gt is the (H, W, 2)
    flow of frame 1's pixels, mask the (H, W) bool rectangle in frame 1."""
    rng = np.random.default_rng(seed)
    par = [(rng.uniform(0.03, 0.35, size=(3, K)), rng.uniform(0.0, 2.0 * np.pi, size=(3, K)),
            rng.uniform(0.0, 2.0 * np.pi, size=(3, K))) for _ in range(2)]
    y, x = np.mgrid[0:H, 0:W].astype(float)

    def rect(xx, yy):
        return (yy >= H // 4) & (yy <= 3 * H // 4 - 1) & (xx >= W // 3) & (xx <= 2 * W // 3 - 1)

    def back(xx, yy):
        return 95.0 + 0.5 * (_field(xx, yy, *par[0]) - 128.0)

    def front(xx, yy):
        return 175.0 + 0.5 * (_field(xx, yy, *par[1]) - 128.0)

    mask = rect(x, y)
    i1 = np.where(mask[..., None], front(x, y), back(x, y))
    x2, y2 = x - fg[0], y - fg[1]
    i2 = np.where(rect(x2, y2)[..., None], front(x2, y2), back(x - bg[0], y - bg[1]))
    gt = np.where(mask[..., None], np.array(fg, dtype=float), np.array(bg, dtype=float))
    im1 = np.floor(np.clip(i1, 0, 255) + 0.5)
    im2 = np.floor(np.clip(i2, 0, 255) + 0.5)
    return im1, im2, gt, mask


def synth_pair(H, W, seed=0, K=32):
    """Return (im1, im2, gt) — two float64 RGB frames with integer values in
    [0, 255] and the (H, W, 2) ground-truth flow from frame 1 to frame 2."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.03, 0.35, size=(3, K))
    th = rng.uniform(0.0, 2.0 * np.pi, size=(3, K))
    ph = rng.uniform(0.0, 2.0 * np.pi, size=(3, K))
    y, x = np.mgrid[0:H, 0:W].astype(float)
    gt = synth_gt(H, W)
    i1 = _field(x, y, f, th, ph)
    i2 = _field(x - gt[..., 0], y - gt[..., 1], f, th, ph)
    im1 = np.floor(np.clip(i1, 0, 255) + 0.5)
    im2 = np.floor(np.clip(i2, 0, 255) + 0.5)
    return im1, im2, gt
