"""Device time of the frame interpolation beside the two flow estimates of
the same call, at 1080p.

    python tools/interp_time.py [--out profiles/interp_time.json] [--size 1080 1920]

synth_pair(H, W, 0), classic+nl-fast, interpolate_frames(im1, im2,
[0.25, 0.5, 0.75]) (one of_estimate_interp call).  One warm-up call, then one
call under of_set_profiling(1); of_kernel_times summed over the interpolation
kernels (interp_splat, interp_resolve, interp_fill, interp_render) per frame,
over fb_check, and over every other kernel of the call (the two flow
estimates with their shared preprocessing), and the call's wall time."""
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
TS = [0.25, 0.5, 0.75]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    optical_flow.interpolate_frames(im1, im2, TS, METHOD)  # warm-up
    ctx = _native.context()
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    t0 = time.perf_counter()
    frames = optical_flow.interpolate_frames(im1, im2, TS, METHOD)
    wall = (time.perf_counter() - t0) * 1e3
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    k = {names[i].decode(): (ms[i], counts[i]) for i in range(n.value)}
    interp = {name: {"ms": v[0], "launches": v[1]} for name, v in k.items() if name.startswith("interp_")}
    interp_ms = sum(v["ms"] for v in interp.values())
    fb_ms = k.get("fb_check", (0.0, 0))[0]
    flow_ms = sum(v[0] for name, v in k.items() if not name.startswith("interp_") and name != "fb_check")
    # the same frames along the same flows, with the info byte
    r = optical_flow.estimate_flow_bidirectional(im1, im2, METHOD)
    f2, _, infos = optical_flow.interpolate_frames(im1, im2, TS, flows=r, return_info=True)
    rec = {
        "size": [H, W], "method": METHOD, "t": TS,
        "interp_kernels": interp,
        "interp_ms_per_frame": interp_ms / len(TS),
        "fb_check_ms": fb_ms,
        "flow_kernels_ms": flow_ms,
        "interp_share_of_kernel_time": interp_ms / (interp_ms + fb_ms + flow_ms),
        "call_wall_ms": wall,
        "info_share_t0.5": [float((infos[1] & 3 == j).mean()) for j in range(4)],
        "filled_share_t0.5": float((infos[1] & 4 != 0).mean()),
        "one_call_equals_two_bitwise": bool(all(np.array_equal(a, b) for a, b in zip(frames, f2))),
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
