"""Device time of the temporal denoiser's kernels per 1080p RGB frame beside
the two flow estimates of the same push.

    python tools/fuse_time.py [--out profiles/fuse_time.json] [--size 1080 1920] [--sigma 10]

synth_pair(H, W, 0) with seeded Gaussian noise as an alternating clip,
classic+nl-fast, patch 2.  Per radius (1: a frame and its 2 neighbours, 2: its
4 neighbours, two of them along chained flows): one TemporalDenoiser session
as warm-up, then one whose last push -- the first that emits a frame with all
its neighbours -- runs under of_set_profiling(1); of_kernel_times of that push
for `fuse` (k_fuse, one launch), `flow_compose` (k_flow_compose, two launches
at radius 2) and summed over every other kernel (the two flow estimates with
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


def kernel_times(ctx):
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    return {names[i].decode(): (ms[i], counts[i]) for i in range(n.value)}


def session(frames, sigma, radius, ctx, profile):
    """Push 2 radius + 1 frames; the last push emits frame `radius` with all
    2 radius neighbours."""
    with optical_flow.TemporalDenoiser(frames[0].shape, METHOD, sigma=sigma, radius=radius, patch=2) as dn:
        for f in frames[:2 * radius]:
            dn.push(f)
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
        t0 = time.perf_counter()
        idx, _ = dn.push(frames[2 * radius])
        wall = (time.perf_counter() - t0) * 1e3
        k = kernel_times(ctx) if profile else {}
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
        assert idx == radius
        return wall, k, float(dn.last_weight.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--sigma", type=float, default=10.0)
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    rng = np.random.default_rng(0)
    frames = [(im1, im2)[k & 1] + rng.normal(0, args.sigma, im1.shape) for k in range(5)]
    ctx = _native.context()
    runs = []
    for radius in (1, 2):
        session(frames, args.sigma, radius, ctx, False)  # warm-up
        wall, k, mean_w = session(frames, args.sigma, radius, ctx, True)
        own = {name: {"ms": k[name][0], "launches": k[name][1]} for name in ("fuse", "flow_compose") if name in k}
        own_ms = sum(v["ms"] for v in own.values())
        other_ms = sum(v[0] for name, v in k.items() if name not in own)
        runs.append({
            "radius": radius, "neighbours": 2 * radius, "patch": 2, "kernels": own,
            "fuse_ms_per_frame": own["fuse"]["ms"] / own["fuse"]["launches"],
            "flow_compose_ms_per_launch": (own["flow_compose"]["ms"] / own["flow_compose"]["launches"]
                                           if "flow_compose" in own else None),
            "denoise_kernels_ms_per_push": own_ms, "other_kernels_ms": other_ms,
            "denoise_share_of_kernel_time": own_ms / (own_ms + other_ms), "push_wall_ms": wall,
            "mean_effective_frames": mean_w,
        })
    rec = {"size": [H, W], "channels": 3, "method": METHOD, "sigma": args.sigma, "runs": runs}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
