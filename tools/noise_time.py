"""Device time of the noise estimators' kernels at 1080p RGB, and what the
temporal denoiser's automatic sigma adds to a push.

    python tools/noise_time.py [--out profiles/noise_time.json] [--size 1080 1920] [--sigma 10] [--pushes 6]

synth_pair(H, W, 0) with seeded Gaussian noise as an alternating clip,
classic+nl-fast, radius 1, patch 2.  Stage entries: after a warm-up call, one
estimate_noise(frame, next frame, flow, mask) and one estimate_noise(frame)
under of_set_profiling(1); of_kernel_times of the call for the noise_* kernels
(launch counts included).  Sessions: one TemporalDenoiser per mode (sigma =
the number, sigma = 'auto') as warm-up, then per mode, alternating, sessions
whose pushes from the second on (each estimates a pair and emits a frame) are
timed on the host clock (every push ends in a stream synchronisation); the
last push of one more session per mode runs under of_set_profiling(1) for the
noise_* kernels' share of the push."""
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


def profiled(ctx, fn):
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 1))
    r = fn()
    k = kernel_times(ctx)
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    return r, k


def noise_kernels(k):
    own = {name: {"ms": v[0], "launches": v[1]} for name, v in k.items() if name.startswith("noise_")}
    return own, sum(v["ms"] for v in own.values()), sum(v["launches"] for v in own.values())


def session(frames, sigma, ctx, profile_last=False):
    """Wall ms of every push after the first, the last_sigma values, and the
    kernel times of the last push if profiled."""
    walls, sig, k = [], [], {}
    with optical_flow.TemporalDenoiser(frames[0].shape, METHOD, sigma=sigma, radius=1, patch=2) as dn:
        dn.push(frames[0])
        for j, f in enumerate(frames[1:]):
            last = profile_last and j == len(frames) - 2
            t0 = time.perf_counter()
            if last:
                _, k = profiled(ctx, lambda: dn.push(f))
            else:
                dn.push(f)
            walls.append((time.perf_counter() - t0) * 1e3)
            sig.append(dn.last_sigma)
    return walls, sig, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--pushes", type=int, default=6)
    ap.add_argument("--sessions", type=int, default=3)
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    rng = np.random.default_rng(0)
    frames = [(im1, im2)[k & 1] + rng.normal(0, args.sigma, im1.shape) for k in range(args.pushes + 1)]
    ctx = _native.context()

    r = optical_flow.estimate_flow_bidirectional(frames[0], frames[1], METHOD)
    stage = {}
    for name, call in (("pair", lambda: optical_flow.estimate_noise(frames[0], frames[1], r.forward, r.occ_forward)),
                       ("single", lambda: optical_flow.estimate_noise(frames[0]))):
        call()  # warm-up
        est, k = profiled(ctx, call)
        own, ms, launches = noise_kernels(k)
        stage[name] = {"sigma": est.sigma, "per_channel": list(est.per_channel), "used": est.used, "kernels": own,
                       "noise_kernels_ms": ms, "noise_launches": launches}

    modes = {"fixed": args.sigma, "auto": "auto"}
    for s in modes.values():
        session(frames[:3], s, ctx)  # warm-up
    walls = {m: [] for m in modes}
    sig = {}
    for _ in range(args.sessions):
        for m, s in modes.items():
            w, sg, _ = session(frames, s, ctx)
            walls[m] += w
            sig[m] = sg
    prof = {}
    for m, s in modes.items():
        _, _, k = session(frames[:3], s, ctx, profile_last=True)
        own, ms, launches = noise_kernels(k)
        other = sum(v[0] for name, v in k.items() if name not in own)
        prof[m] = {"noise_kernels": own, "noise_kernels_ms": ms, "noise_launches": launches, "other_kernels_ms": other}
    med = {m: float(np.median(w)) for m, w in walls.items()}
    rec = {"size": [H, W], "channels": 3, "method": METHOD, "sigma": args.sigma, "radius": 1, "stage": stage,
           "push_wall_ms_median": med, "push_wall_ms_min": {m: float(np.min(w)) for m, w in walls.items()},
           "push_wall_ms_spread": {m: [float(np.percentile(w, 10)), float(np.percentile(w, 90))]
                                   for m, w in walls.items()},
           "pushes_timed": {m: len(w) for m, w in walls.items()},
           "auto_minus_fixed_ms_median": med["auto"] - med["fixed"], "session_sigma": sig, "profiled_push": prof}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
