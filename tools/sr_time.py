"""Device time of the super-resolution kernels for one 1080p -> 4K RGB frame
with 4 neighbours, alone and in a session push beside the two flow estimates
of that push.

    python tools/sr_time.py [--out profiles/sr_time.json] [--size 1080 1920] [--sigma 10]

synth_pair(H, W, 0) with seeded Gaussian noise as an alternating clip,
classic+nl-fast, factor 2, patch 2, reach 0.75, back 0 and 0.5.  The stage
call: super_resolve of frame 2 with the other four along zero flows, once as
warm-up, then under of_set_profiling(1); of_kernel_times for `fuse_weights`
(k_fuse_weights), `super_resolve` (k_super_resolve) and, with back > 0,
`reduce_frame` and `sr_back`.  The session: one SuperResolver of radius 2 as
warm-up, then one whose last push -- the first that emits a frame with all its
neighbours -- runs under profiling; those kernels and `flow_compose` (two
launches) beside the sum over every other kernel (the two flow estimates with
their shared preprocessing and fb_check), and the push's wall time."""
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
OWN = ("fuse_weights", "super_resolve", "reduce_frame", "sr_back", "flow_compose")


def kernel_times(ctx):
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    return {names[i].decode(): (ms[i], counts[i]) for i in range(n.value)}


def profiled(ctx, profile, fn):
    """fn() under of_set_profiling(1) when `profile`: (result, wall ms, kernel times)."""
    if profile:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    t0 = time.perf_counter()
    r = fn()
    wall = (time.perf_counter() - t0) * 1e3
    k = kernel_times(ctx) if profile else {}
    if profile:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return r, wall, k


def split(k):
    own = {name: {"ms": k[name][0], "launches": k[name][1]} for name in OWN if name in k}
    return own, sum(v["ms"] for v in own.values()), sum(v[0] for name, v in k.items() if name not in own)


def stage(frames, sigma, back, ctx, profile):
    zero = np.zeros(frames[0].shape[:2] + (2,), np.float32)
    neigh = [frames[k] for k in (1, 3, 0, 4)]
    (_, sup), wall, k = profiled(ctx, profile, lambda: optical_flow.super_resolve(
        frames[2], neigh, [zero] * 4, 2, sigma, back=back, return_support=True))
    return wall, k, float(sup.mean())


def session(frames, sigma, ctx, profile):
    """Push 5 frames into a session of radius 2; the last push emits frame 2
    with all 4 neighbours."""
    with optical_flow.SuperResolver(frames[0].shape, METHOD, factor=2, sigma=sigma, radius=2) as sr:
        for f in frames[:4]:
            sr.push(f)
        (idx, _), wall, k = profiled(ctx, profile, lambda: sr.push(frames[4]))
        assert idx == 2
        return wall, k, float(sr.last_support.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--sigma", type=float, default=10.0)
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    rng = np.random.default_rng(0)
    frames = [(im1, im2)[k & 1] + rng.normal(0, args.sigma, im1.shape) for k in range(5)]
    ctx = _native.context()
    stages = []
    for back in (0.0, 0.5):
        stage(frames, args.sigma, back, ctx, False)  # warm-up
        wall, k, sup = stage(frames, args.sigma, back, ctx, True)
        own, own_ms, _ = split(k)
        stages.append({"back": back, "kernels": own, "sr_kernels_ms": own_ms, "call_wall_ms": wall,
                       "mean_support": sup})
    session(frames, args.sigma, ctx, False)  # warm-up
    wall, k, sup = session(frames, args.sigma, ctx, True)
    own, own_ms, other_ms = split(k)
    rec = {"size": [H, W], "out_size": [2 * H, 2 * W], "channels": 3, "factor": 2, "neighbours": 4, "patch": 2,
           "reach": 0.75, "method": METHOD, "sigma": args.sigma, "stage": stages,
           "session_push": {"radius": 2, "kernels": own, "sr_kernels_ms": own_ms, "other_kernels_ms": other_ms,
                            "sr_share_of_kernel_time": own_ms / (own_ms + other_ms), "push_wall_ms": wall,
                            "mean_support": sup}}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
