"""Device time of the inpainting kernels for one 1080p RGB frame at radius 8
with a 10 % mask, alone and in a session push beside the two weighted flow
estimates of that push.

    python tools/inpaint_time.py [--out profiles/inpaint_time.json] [--size 1080 1920] [--radius 8]

synth_pair(H, W, 0) as an alternating clip of 2 radius + 1 frames,
classic+nl-fast, grow 2, margin 4; the mask is a rectangle of a tenth of the
frame moving by 8 px per frame.  The stage call: propagate_fill of the middle
frame along zero flows, once as warm-up, then under of_set_profiling(1);
of_kernel_times for `mask_grow` (k_mask_grow, one launch per frame within
reach) and `inpaint_fill` (k_inpaint_fill).  The session: one VideoInpainter as
warm-up, then one whose last push -- the first that emits a frame with all its
neighbours -- runs under profiling; those kernels (mask_grow: the frame's own
mask and the pair weight) beside the sum over every other kernel (the two
weighted flow estimates), and the push's wall time."""
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
OWN = ("mask_grow", "inpaint_fill")


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


def status_shares(st):
    return {name: float((st == v).mean()) for name, v in (("kept", 0), ("filled", 1), ("unfilled", 2))}


def stage(frames, masks, radius, ctx, profile):
    zero = [np.zeros(frames[0].shape[:2] + (2,), np.float32)] * (len(frames) - 1)
    (_, st), wall, k = profiled(ctx, profile, lambda: optical_flow.propagate_fill(
        frames, masks, zero, zero, radius, radius, 2, return_status=True))
    return wall, k, status_shares(st)


def session(frames, masks, radius, ctx, profile):
    """Push 2 radius + 1 frames; the last push emits the middle frame with all
    its neighbours."""
    H, W = frames[0].shape[:2]
    with optical_flow.VideoInpainter(H, W, 3, METHOD, radius=radius, grow=2, margin=4) as vi:
        for f, m in zip(frames[:-1], masks[:-1]):
            vi.push(f, m)
        (idx, _), wall, k = profiled(ctx, profile, lambda: vi.push(frames[-1], masks[-1]))
        assert idx == radius
        return wall, k, status_shares(vi.last_status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--radius", type=int, default=8)
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
    stage(frames, masks, R, ctx, False)  # warm-up
    wall, k, shares = stage(frames, masks, R, ctx, True)
    own, own_ms, _ = split(k)
    st = {"kernels": own, "inpaint_kernels_ms": own_ms, "call_wall_ms": wall, "status": shares}
    session(frames, masks, R, ctx, False)  # warm-up
    wall, k, shares = session(frames, masks, R, ctx, True)
    own, own_ms, other_ms = split(k)
    top = sorted(((v[0], name, v[1]) for name, v in k.items() if name not in own), reverse=True)[:5]
    rec = {"size": [H, W], "channels": 3, "radius": R, "grow": 2, "margin": 4, "method": METHOD,
           "mask_share": float(np.mean([m.mean() for m in masks])), "stage": st,
           "session_push": {"kernels": own, "inpaint_kernels_ms": own_ms, "other_kernels_ms": other_ms,
                            "other_kernels_top": [{"name": n, "ms": ms, "launches": c} for ms, n, c in top],
                            "inpaint_share_of_kernel_time": own_ms / (own_ms + other_ms), "push_wall_ms": wall,
                            "status": shares}}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
