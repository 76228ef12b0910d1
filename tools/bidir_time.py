"""Wall time of flow in both directions at 1080p: two estimate_flow calls
((im1, im2) then (im2, im1)) against one estimate_flow_bidirectional call.

    python tools/bidir_time.py [--out profiles/bidir_time.json] [--reps 5]

synth_pair(1080, 1920, 0), classic+nl-fast.  One warm-up of each form, then
`reps` repetitions of the two-call form and `reps` of the one-call form.
Writes the medians, the spreads (max - min), every repetition, the
preprocess_ms of one estimate_flow call and of the bidirectional call (its
shared preprocessing, of_stats), and whether the flows agreed bitwise.
Exit status 1 when the bidirectional median exceeds the two-call median by
more than the two-call form's own spread."""
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
from optical_flow import _abi, _native  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402

METHOD = "classic+nl-fast"


def preprocess_ms(im1, im2):
    """(one of_estimate_flow call's preprocess_ms, the bidirectional call's)."""
    H, W = im1.shape[:2]
    a, b = _native.f32(im1), _native.f32(im2)
    ctx = _native.context()
    ope = optical_flow.load_of_method(METHOD)
    out = np.empty((2, 2, H, W), np.float32)
    res = []
    for bidir in (False, True):
        P = ope.to_params()
        P.guide_mode = int(ope._METHOD == 'classic_nl' and ope.color_images is not None)
        sf, sb = _abi.OfStats(), _abi.OfStats()
        if bidir:
            ctx.check(ctx.lib.of_estimate_flow_bidir(ctx.handle, C.byref(P), _native.ptr(a), _native.ptr(b), H, W, 3,
                                                     None, None, _native.ptr(out[0]), _native.ptr(out[1]), 0.01, 0.5,
                                                     None, None, C.byref(sf), C.byref(sb)))
        else:
            ctx.check(ctx.lib.of_estimate_flow(ctx.handle, C.byref(P), _native.ptr(a), _native.ptr(b), H, W, 3, None,
                                               _native.ptr(out[0]), C.byref(sf)))
        res.append(sf.preprocess_ms)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bidir_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    args = ap.parse_args()
    H, W = args.size
    im1, im2, _ = synth_pair(H, W, 0)

    def two_calls():
        return optical_flow.estimate_flow(im1, im2, METHOD), optical_flow.estimate_flow(im2, im1, METHOD)

    def one_call():
        return optical_flow.estimate_flow_bidirectional(im1, im2, METHOD)

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    fw, bw = two_calls()
    r = one_call()
    bitwise = bool(np.array_equal(fw, r.forward) and np.array_equal(bw, r.backward))
    two = [timed(two_calls)[0] for _ in range(args.reps)]
    one = [timed(one_call)[0] for _ in range(args.reps)]
    pre_one, pre_bidir = preprocess_ms(im1, im2)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    rec = {
        "size": [H, W], "method": METHOD, "reps": args.reps,
        "two_calls_ms": {"median": statistics.median(two), "spread": spread(two), "all": two},
        "bidirectional_ms": {"median": statistics.median(one), "spread": spread(one), "all": one},
        "saving_ms": statistics.median(two) - statistics.median(one),
        "preprocess_ms": {"estimate_flow": pre_one, "estimate_flow_bidirectional": pre_bidir},
        "occ_forward_share": [float((r.occ_forward == k).mean()) for k in (0, 1, 2)],
        "flows_bitwise_equal": bitwise,
    }
    ok = rec["bidirectional_ms"]["median"] <= rec["two_calls_ms"]["median"] + rec["two_calls_ms"]["spread"]
    rec["not_slower_than_two_calls"] = bool(ok)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
