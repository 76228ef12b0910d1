"""GPU time of the weighted fused warp + assembly kernel (k_warp_operator<true, ...>)
beside the unweighted one (k_warp_operator<false, ...>), per launch, from of_kernel_times.

    python tools/weight_time.py [--size 1080 1920] [--method classic+nl-fast]

synth_pair(H, W, 0); one warm-up of each form, then one profiled
estimate_flow without and one with a data weight (uniform in [0, 1]; its
values do not change what the kernel executes).  Prints, per pyramid-level
size, the launches and the mean time per launch of both forms."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402


def profiled(fn):
    """{(kernel, level px): (ms per launch, launches)} of the launches fn() makes."""
    ctx = _native.context()
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 2))
    fn()
    n = C.c_int(0)
    names = (C.c_char_p * 1024)()
    ms = (C.c_double * 1024)()
    cnt = (C.c_int64 * 1024)()
    ctx.check(ctx.lib.of_kernel_times(ctx.handle, 1024, names, ms, cnt, None, C.byref(n)))
    ctx.check(ctx.lib.of_set_profiling(ctx.handle, 0))
    out = {}
    for i in range(min(n.value, 1024)):
        name, px = names[i].decode().rsplit("@", 1)
        out[name, int(px)] = (ms[i] / cnt[i], int(cnt[i]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--method", default="classic+nl-fast")
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)
    w = np.random.default_rng(0).uniform(0.0, 1.0, (H, W)).astype(np.float32)
    plain = lambda: optical_flow.estimate_flow(im1, im2, args.method)  # noqa: E731
    weighted = lambda: optical_flow.estimate_flow(im1, im2, args.method, data_weight=w)  # noqa: E731
    plain()
    weighted()
    res = {"plain": profiled(plain), "weighted": profiled(weighted)}
    rows = []
    for (name, px), (t, k) in sorted(res["plain"].items(), key=lambda kv: -kv[0][1]):
        if not name.startswith("warp_operator"):
            continue
        tw, kw = res["weighted"].get((name, px), (float("nan"), 0))
        rows.append({"kernel": name, "px": px, "plain_ms": t, "plain_launches": k, "weighted_ms": tw,
                     "weighted_launches": kw})
    print(json.dumps({"size": [H, W], "method": args.method, "per_launch": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
