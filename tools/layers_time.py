"""Device time of one default layered motion segmentation at 1080p on an
estimated forward flow, beside the fit and the two flow estimates.

    python tools/layers_time.py [--out profiles/layers_time.json] [--size 1080 1920]

estimate_flow_bidirectional on synth_pair(H, W, 0) (classic+nl-fast) under
of_set_profiling(1) gives the flow estimates' kernel time; then, each after
one warm-up call, fit_motion and segment_motion (affine, default options) on
the forward flow with its forward-backward mask as `state`: of_kernel_times
per kernel, their sum, the scoring kernel's share and the call's wall time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import optical_flow  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.utils.synthetic import synth_pair  # noqa: E402
from motion_time import METHOD, profiled  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    args = ap.parse_args()
    H, W = args.size
    ctx = _native.context()
    im1, im2, _ = synth_pair(H, W, 0)
    bi, wall_flow, k_flow = profiled(ctx, lambda: optical_flow.estimate_flow_bidirectional(im1, im2, METHOD))
    fw, occ = bi.forward, bi.occ_forward
    _, wall_fit, k_fit = profiled(ctx, lambda: optical_flow.fit_motion(fw, "affine", state=occ))
    seg, wall_seg, k_seg = profiled(ctx, lambda: optical_flow.segment_motion(fw, "affine", state=occ))
    total = sum(v["ms"] for v in k_seg.values())
    rec = {"size": [H, W], "method": METHOD, "model": "affine",
           "flow_estimates_kernels_ms": sum(v["ms"] for v in k_flow.values()), "flow_estimates_wall_ms": wall_flow,
           "fit_kernels_ms": sum(v["ms"] for v in k_fit.values()), "fit_wall_ms": wall_fit,
           "segment_kernels_ms": total, "segment_launches": sum(v["launches"] for v in k_seg.values()),
           "segment_wall_ms": wall_seg, "score_share": k_seg["layers_score"]["ms"] / total, "kernels": k_seg,
           "n": seg.n, "pixels": [la.pixels for la in seg.layers], "none": int(np.sum(seg.labels == 255)),
           "masked": int(np.sum(occ != 0)), "theta": [[float(t) for t in la.theta] for la in seg.layers]}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
