"""Device time of the point tracker's kernels per push beside the two flow
estimates of the same push, at 1080p.

    python tools/track_time.py [--out profiles/track_time.json] [--size 1080 1920] [--steps 8 1]

synth_pair(H, W, 0) as a two-frame clip, classic+nl-fast.  Per seeding step:
one PointTracker session as warm-up, then one under of_set_profiling(1);
of_kernel_times of the second push summed over the tracker's kernels
(track_advance, track_mark, track_flags, track_scan, track_scatter) and over
every other kernel of the push (the two flow estimates with their shared
preprocessing, fb_check and the gray plane), the table size and the push's
wall time.  min_eig = 0 so every free cell seeds (step 1: one track per pixel);
track_flags is timed once more with the default min_eig = 25 (seed_points on
the second frame's gray plane), where it also evaluates the structure tensor."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.interface import _rgb2gray  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402

METHOD = "classic+nl-fast"


def kernel_times(ctx):
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    return {names[i].decode(): (ms[i], counts[i]) for i in range(n.value)}


def session(frames, step, ctx, profile):
    with optical_flow.PointTracker(frames[0].shape, METHOD, step=step, min_eig=0.0) as tr:
        first = tr.push(frames[0])
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
        t0 = time.perf_counter()
        snap = tr.push(frames[1])
        wall = (time.perf_counter() - t0) * 1e3
        k = kernel_times(ctx) if profile else {}
        if profile:
            ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return first, snap, wall, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--steps", type=int, nargs="+", default=(8, 1))
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    ctx = _native.context()
    runs = []
    for step in args.steps:
        session((im1, im2), step, ctx, False)  # warm-up
        first, snap, wall, k = session((im1, im2), step, ctx, True)
        track = {name: {"ms": v[0], "launches": v[1]} for name, v in k.items() if name.startswith("track_")}
        track_ms = sum(v["ms"] for v in track.values())
        other_ms = sum(v[0] for name, v in k.items() if not name.startswith("track_"))
        # track_flags with the eigenvalue test on (min_eig = 0 skips the structure tensor)
        gray = _rgb2gray(im2)
        optical_flow.seed_points(gray, step=step)
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
        seeded = optical_flow.seed_points(gray, step=step)
        flags_ms = kernel_times(ctx)["track_flags"][0]
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
        runs.append({
            "track_flags_ms_min_eig_25": flags_ms, "seeds_min_eig_25": len(seeded),
            "step": step, "tracks_advanced": len(first.xy), "tracks_after": len(snap.xy),
            "alive_after": int((snap.status == 0).sum()), "n_new": snap.n_new,
            "track_kernels": track, "track_ms_per_push": track_ms, "other_kernels_ms": other_ms,
            "track_share_of_kernel_time": track_ms / (track_ms + other_ms), "push_wall_ms": wall,
        })
    rec = {"size": [H, W], "method": METHOD, "runs": runs}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
