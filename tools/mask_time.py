"""Device time of the mask propagation kernels for one 1080p RGB advance, alone
and in a session push beside the two flow estimates of that push.

    python tools/mask_time.py [--out profiles/mask_time.json] [--size 1080 1920]

synth_pair(H, W, 0) as the two frames, classic+nl-fast, the defaults (vote
radius 8, range 20, smooth 1); the mask is a rectangle of a tenth of the frame.
The stage call, advance_mask of frame 2, once as warm-up, then under
of_set_profiling(1), with two inputs: `band`, the rectangle moved by 8 px over
a still background, untrusted (state 1) in the 8 px it uncovers, so that only
the tiles along that band vote; and `scattered`, a flow uniform in +-6 with 30 %
of the states untrusted at random, so that every tile takes the vote's LDS
path.  of_kernel_times for `mask_carry`, `mask_vote` and `mask_mode`.  The
session: one MaskPropagator as warm-up, then one whose second push runs under
profiling; those kernels beside the sum over every other kernel (the two flow
estimates and the forward-backward check), and the push's wall time."""
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
OWN = ("mask_carry", "mask_vote", "mask_mode")


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
    return {name: float((st == v).mean()) for name, v in (("carried", 0), ("voted", 1), ("unknown", 2))}


def stage(mask, frame, flow, state, ctx, profile):
    (_, st), wall, k = profiled(ctx, profile, lambda: optical_flow.advance_mask(mask, frame, flow, state,
                                                                                return_status=True))
    own, own_ms, _ = split(k)
    return {"kernels": own, "mask_kernels_ms": own_ms, "call_wall_ms": wall, "status": status_shares(st)}


def session(frames, mask, ctx, profile):
    H, W = frames[0].shape[:2]
    with optical_flow.MaskPropagator(H, W, 3, METHOD) as mp:
        mp.push(frames[0], mask)
        _, wall, k = profiled(ctx, profile, lambda: mp.push(frames[1]))
        return wall, k, status_shares(mp.last_status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    mh, mw = int(round(H * 0.1 ** 0.5)), int(round(W * 0.1 ** 0.5))
    y0, x0 = (H - mh) // 2, (W - mw) // 2
    mask = np.zeros((H, W), np.uint8)
    mask[y0:y0 + mh, x0:x0 + mw] = 1
    # band: the rectangle has moved 8 px to the right; the 8 px it uncovered are not trusted
    band_flow = np.zeros((H, W, 2), np.float32)
    band_flow[y0:y0 + mh, x0 + 8:x0 + mw + 8, 0] = -8.0
    band_state = np.zeros((H, W), np.uint8)
    band_state[y0:y0 + mh, x0:x0 + 8] = 1
    rng = np.random.default_rng(0)
    sc_flow = rng.uniform(-6, 6, (H, W, 2)).astype(np.float32)
    sc_state = (rng.uniform(size=(H, W)) < 0.3).astype(np.uint8)
    ctx = _native.context()
    stages = {}
    for name, flow, state in (("band", band_flow, band_state), ("scattered", sc_flow, sc_state)):
        stage(mask, im2, flow, state, ctx, False)  # warm-up
        stages[name] = stage(mask, im2, flow, state, ctx, True)
    session((im1, im2), mask, ctx, False)  # warm-up
    wall, k, shares = session((im1, im2), mask, ctx, True)
    own, own_ms, other_ms = split(k)
    top = sorted(((v[0], name, v[1]) for name, v in k.items() if name not in own), reverse=True)[:5]
    rec = {"size": [H, W], "channels": 3, "vote_radius": 8, "vote_range": 20.0, "smooth": 1, "method": METHOD,
           "mask_share": float(mask.mean()), "stage": stages,
           "session_push": {"kernels": own, "mask_kernels_ms": own_ms, "other_kernels_ms": other_ms,
                            "other_kernels_top": [{"name": n, "ms": ms, "launches": c} for ms, n, c in top],
                            "mask_share_of_kernel_time": own_ms / (own_ms + other_ms), "push_wall_ms": wall,
                            "status": shares}}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
