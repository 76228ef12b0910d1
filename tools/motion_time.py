"""Device time of the global motion fit and the affine warp at 1080p, alone and
beside the two flow estimates of a stabiliser push.

    python tools/motion_time.py [--out profiles/motion_time.json] [--size 1080 1920]

1. fit_motion on a seeded flow (an affine motion plus noise and a foreground
   block), per model, 10 robust passes, with a state plane: one call as
   warm-up, then one under of_set_profiling(1); of_kernel_times summed over
   the fit's kernels (motion_init, motion_part, motion_group, motion_final)
   and the call's wall time.
2. warp_affine of an RGB frame: `warp_affine` (k_warp_affine, one launch).
3. A Stabilizer session (similarity, radius 1) over synth_pair(H, W, 0) as an
   alternating RGB clip: one session as warm-up, then one whose second push
   runs under profiling: the fit's and the warp's kernels beside every other
   kernel of the push (the two flow estimates with their shared preprocessing
   and fb_check), and the push's wall time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402

METHOD = "classic+nl-fast"
FIT_KERNELS = ("motion_init", "motion_part", "motion_group", "motion_final")


def kernel_times(ctx):
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    return {names[i].decode(): {"ms": ms[i], "launches": counts[i]} for i in range(n.value)}


def profiled(ctx, fn):
    """(fn's result, its wall ms, the kernel times of that one call)."""
    fn()  # warm-up
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    t0 = time.perf_counter()
    r = fn()
    wall = (time.perf_counter() - t0) * 1e3
    k = kernel_times(ctx)
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return r, wall, k


def scene_flow(H, W):
    rng = np.random.default_rng(0)
    s = 0.5 * max(H, W)
    ii, jj = np.mgrid[0:H, 0:W]
    x, y = (jj - 0.5 * (W - 1)) / s, (ii - 0.5 * (H - 1)) / s
    f = np.stack([1.5 + 0.8 * x - 1.2 * y, -0.7 + 1.2 * x + 0.8 * y], -1) + rng.normal(0, 0.1, (H, W, 2))
    f[H // 5:H // 5 * 4, W // 4:W // 4 * 3] = (6.0, -4.0)
    state = (rng.uniform(size=(H, W)) < 0.05).astype(np.uint8)
    return f.astype(np.float32), state


def session(frames, ctx, profile):
    with optical_flow.Stabilizer(frames[0].shape, METHOD, model="similarity", radius=1) as st:
        st.push(frames[0])
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
        t0 = time.perf_counter()
        idx, _ = st.push(frames[1])
        wall = (time.perf_counter() - t0) * 1e3
        k = kernel_times(ctx) if profile else {}
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
        assert idx == 0
        return wall, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    args = ap.parse_args()
    H, W = args.size
    ctx = _native.context()
    flow, state = scene_flow(H, W)
    fits = []
    for model in ("translation", "similarity", "affine"):
        r, wall, k = profiled(ctx, lambda: optical_flow.fit_motion(flow, model, state=state, return_inliers=True))
        own = {n: k[n] for n in FIT_KERNELS if n in k}
        part = own["motion_part"]
        fits.append({"model": model, "iters": 10, "passes_launched": part["launches"], "kernels": own,
                     "fit_kernels_ms": sum(v["ms"] for v in own.values()),
                     "motion_part_ms_per_pass": part["ms"] / part["launches"],
                     # u, v (8 bytes) and the state byte per pixel and pass; the last pass writes 4 more
                     "motion_part_gbytes_per_s": 9.0 * H * W / (part["ms"] / part["launches"] * 1e-3) / 1e9,
                     "call_wall_ms": wall, "degenerate": r.degenerate, "theta": [float(t) for t in r.theta]})
    im = np.random.default_rng(1).uniform(0, 255, (H, W, 3)).astype(np.float32)
    A = np.array([[1.01, -0.02, 3.5], [0.02, 1.01, -2.25]])
    _, wall, k = profiled(ctx, lambda: optical_flow.warp_affine(im, A, return_valid=True))
    warp = {"channels": 3, "kernel_ms": k["warp_affine"]["ms"], "launches": k["warp_affine"]["launches"],
            "call_wall_ms": wall}
    im1, im2, _ = synth_pair(H, W, 0)
    frames = [im1, im2]
    session(frames, ctx, False)  # warm-up
    wall, k = session(frames, ctx, True)
    own_ms = sum(k[n]["ms"] for n in FIT_KERNELS + ("warp_affine",) if n in k)
    other_ms = sum(v["ms"] for n, v in k.items() if n not in FIT_KERNELS + ("warp_affine",))
    push = {"model": "similarity", "radius": 1, "fit_and_warp_kernels_ms": own_ms, "other_kernels_ms": other_ms,
            "share_of_kernel_time": own_ms / (own_ms + other_ms), "push_wall_ms": wall}
    rec = {"size": [H, W], "method": METHOD, "fit": fits, "warp_affine": warp, "stabilizer_push": push}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
