"""Wall time of the bidirectional estimate at scale 1, 2 and 4 at 1080p RGB,
the device time of the two new kernels, and the accuracy each scale costs.

    python tools/scale_time.py [--out profiles/scale_time.json] [--size 1080 1920] [--reps 7]

synth_pair(H, W, 0), classic+nl-fast, upsample_range 20.  One warm-up of every
scale, then `reps` rounds that time one estimate_flow_bidirectional call per
scale, the scales alternating inside a round, on the host clock (the call ends
in a stream synchronisation): warm medians and spreads (max - min) per scale.
Scale 1 is the full-resolution call, unchanged by the scale option.  Then one
call per scale under of_set_profiling(1) for the device time of reduce_frame
and flow_upsample (of_kernel_times) and the sum over all kernels.  AEPE of the
forward flow against the synthetic pair's ground truth, and on RubberWhale
(tests/golden) against flow10.flo, per scale.  Exit status 0 always: the
record says whether scale 2 beat scale 1 beyond the spreads."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402

METHOD = "classic+nl-fast"
SCALES = (1, 2, 4)


def kernel_times(ctx):
    n = C.c_int(0)
    names = (C.c_char_p * 512)()
    ms = (C.c_double * 512)()
    counts = (C.c_int64 * 512)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 512, names, ms, counts, None, C.byref(n)))
    return {names[i].decode(): (ms[i], counts[i]) for i in range(n.value)}


def aepe(uv, gt):
    known = np.all(np.abs(gt) < 1e9, axis=-1)   # Middlebury marks unknown flow with 1e9
    return float(np.sqrt(((uv - gt) ** 2).sum(-1))[known].mean())


def rubberwhale():
    from PIL import Image
    g = os.path.join(ROOT, "tests", "golden")
    im1 = np.array(Image.open(os.path.join(g, "frame10.png"))).astype(np.float64)
    im2 = np.array(Image.open(os.path.join(g, "frame11.png"))).astype(np.float64)
    return im1, im2, optical_flow.read_flo(os.path.join(g, "flow10.flo"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    H, W = args.size
    im1, im2, gt = synth_pair(H, W, 0)
    ctx = _native.context()

    def call(s):
        return optical_flow.estimate_flow_bidirectional(im1, im2, METHOD, scale=s)

    acc = {s: aepe(call(s).forward, gt) for s in SCALES}  # also the warm-up of every scale
    walls = {s: [] for s in SCALES}
    for _ in range(args.reps):
        for s in SCALES:
            t = time.perf_counter()
            call(s)
            walls[s].append((time.perf_counter() - t) * 1e3)
    prof = {}
    for s in SCALES:
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
        call(s)
        k = kernel_times(ctx)
        ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
        prof[s] = {"all_kernels_ms": sum(v[0] for v in k.values())}
        for name in ("reduce_frame", "flow_upsample"):
            ms, launches = k.get(name, (0.0, 0))
            prof[s][name] = {"ms": ms, "launches": launches}
    rw = {}
    try:
        a, b, g = rubberwhale()
        rw = {s: aepe(optical_flow.estimate_flow(a, b, METHOD, scale=s), g) for s in SCALES}
    except ImportError:   # no PIL: the figure is left out, not guessed
        pass
    spread = lambda v: max(v) - min(v)  # noqa: E731
    med = {s: statistics.median(walls[s]) for s in SCALES}
    rec = {"size": [H, W], "channels": 3, "method": METHOD, "upsample_range": 20.0, "reps": args.reps,
           "bidirectional_wall_ms": {str(s): {"median": med[s], "spread": spread(walls[s]), "all": walls[s]}
                                     for s in SCALES},
           "profiled_call": {str(s): prof[s] for s in SCALES},
           "aepe_synth_forward": {str(s): acc[s] for s in SCALES},
           "aepe_rubberwhale": {str(s): v for s, v in rw.items()},
           "scale2_faster_beyond_spread": bool(med[2] + spread(walls[2]) + spread(walls[1]) < med[1])}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
