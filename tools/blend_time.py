"""Device time of the gradient-domain blending for one 1080p RGB frame at
radius 8 with a 10 % mask, alone and in a session push beside the two weighted
flow estimates of that push; and the wall time of a push without blending.

    python tools/blend_time.py [--out profiles/blend_time.json] [--size 1080 1920] [--radius 8] [--off N]

The clip, masks and method of tools/inpaint_time.py.  The stage call:
blend_fill of the middle frame along zero flows, once as warm-up, then under
of_set_profiling(1); of_kernel_times for the solver's kernels (psn_*), the
blended fill's own (blend_*) and the fill's (mask_grow, inpaint_fill).  The
session: one VideoInpainter(blend=True) as warm-up, then one whose last push --
the first that emits a frame with all its neighbours -- runs under profiling.
With --off N: no blending at all (only what the library had before blending),
N sessions after a warm-up one, the wall time of each one's last push and the
SHA-256 of the frame it emitted, to compare two builds."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from inpaint_time import METHOD, kernel_times, profiled  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402

FILL = ("mask_grow", "inpaint_fill")


def split(k):
    """(the solver's kernels, the blended fill's other kernels, the fill's, everything else) of of_kernel_times."""
    def part(pick):
        own = {n: {"ms": v[0], "launches": v[1]} for n, v in k.items() if pick(n)}
        return {"kernels": own, "ms": sum(v["ms"] for v in own.values()),
                "launches": int(sum(v["launches"] for v in own.values()))}
    solver, blend, fill = (part(lambda n: n.startswith("psn_")), part(lambda n: n.startswith("blend_")),
                           part(lambda n: n in FILL))
    other = sum(v[0] for n, v in k.items() if not n.startswith(("psn_", "blend_")) and n not in FILL)
    return solver, blend, fill, other


def shares(st):
    return {name: float((st == v).mean()) for name, v in (("kept", 0), ("filled", 1), ("unfilled", 2), ("spatial", 3))}


def record(wall, k, st):
    solver, blend, fill, other = split(k)
    return {"solver": solver, "blend": blend, "fill": fill, "other_kernels_ms": other,
            "blending_ms": solver["ms"] + blend["ms"], "blending_launches": solver["launches"] + blend["launches"],
            "wall_ms": wall, "status": shares(st)}


def stage(frames, masks, radius, ctx, profile):
    zero = [np.zeros(frames[0].shape[:2] + (2,), np.float32)] * (len(frames) - 1)
    (_, st), wall, k = profiled(ctx, profile, lambda: optical_flow.blend_fill(
        frames, masks, zero, zero, radius, radius, 2, return_status=True))
    return record(wall, k, st)


def session(frames, masks, radius, ctx, profile, **kw):
    """Push 2 radius + 1 frames; the last push emits the middle frame with all
    its neighbours."""
    H, W = frames[0].shape[:2]
    with optical_flow.VideoInpainter(H, W, 3, METHOD, radius=radius, grow=2, margin=4, **kw) as vi:
        for f, m in zip(frames[:-1], masks[:-1]):
            vi.push(f, m)
        (idx, out), wall, k = profiled(ctx, profile, lambda: vi.push(frames[-1], masks[-1]))
        assert idx == radius
        return record(wall, k, vi.last_status), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--off", type=int, default=0)
    args = ap.parse_args()
    H, W = args.size
    R = args.radius
    im1, im2, _ = synth_pair(H, W, 0)
    frames = [(im1, im2)[k & 1] for k in range(2 * R + 1)]
    mh, mw = int(round(H * 0.1 ** 0.5)), int(round(W * 0.1 ** 0.5))
    masks = []
    for k in range(2 * R + 1):
        m = np.zeros((H, W), np.uint8)
        y0, x0 = (H - mh) // 2, (W - mw) // 2 + 8 * (k - R)
        m[y0:y0 + mh, max(x0, 0):x0 + mw] = 1
        masks.append(m)
    ctx = _native.context()
    rec = {"size": [H, W], "channels": 3, "radius": R, "grow": 2, "margin": 4, "method": METHOD,
           "mask_share": float(np.mean([m.mean() for m in masks]))}
    if args.off:
        session(frames, masks, R, ctx, False)  # warm-up
        runs = [session(frames, masks, R, ctx, False) for _ in range(args.off)]
        rec["push_without_blending"] = {
            "push_wall_ms": [r["wall_ms"] for r, _ in runs],
            "sha256": sorted({hashlib.sha256(np.ascontiguousarray(o).tobytes()).hexdigest() for _, o in runs})}
    else:
        stage(frames, masks, R, ctx, False)  # warm-up
        rec["stage"] = stage(frames, masks, R, ctx, True)
        session(frames, masks, R, ctx, False, blend=True)  # warm-up
        t0 = time.perf_counter()
        rec["session_push"], _ = session(frames, masks, R, ctx, True, blend=True)
        rec["session_wall_s"] = time.perf_counter() - t0
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
