"""Does a second, occlusion-weighted pass improve a flow?  (Needs the GPU; a
measurement, not a test: no gate.)

    python tools/occ_refine.py [--method classic+nl-fast] [--out FILE.json]

On RubberWhale (tests/golden/frame10.png, frame11.png, flow10.flo):
estimate_flow_bidirectional gives the forward flow and its forward-backward
mask; the forward flow is then estimated again with data_weight =
(occ_forward == FB_CONSISTENT), i.e. the data term switched off where the
check flagged the pixel as occluded or leaving the frame.  Prints the AEPE
against the ground truth (pixels with known ground truth only) overall, on
the flagged pixels and on the rest, before and after."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

import optical_flow  # noqa: E402
from optical_flow.io.flo_io import read_flo  # noqa: E402
from optical_flow.utils.occlusion import FB_CONSISTENT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="classic+nl-fast")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    im1 = np.array(Image.open(os.path.join(GOLDEN, "frame10.png"))).astype(np.float64)
    im2 = np.array(Image.open(os.path.join(GOLDEN, "frame11.png"))).astype(np.float64)
    gt = read_flo(os.path.join(GOLDEN, "flow10.flo"))
    known = np.all(np.abs(gt) < 1e9, axis=2)
    r = optical_flow.estimate_flow_bidirectional(im1, im2, args.method)
    ok = r.occ_forward == FB_CONSISTENT
    second = optical_flow.estimate_flow(im1, im2, args.method, data_weight=ok)
    flagged = ~ok & known
    rest = ok & known

    def aepe(uv, m):
        return float(np.sqrt(((uv - gt) ** 2).sum(-1))[m].mean()) if m.any() else float("nan")

    rec = {"method": args.method, "size": list(im1.shape[:2]),
           "flagged_share": float((~ok).mean()), "flagged_with_known_gt": int(flagged.sum()),
           "aepe_before": {"all": aepe(r.forward, known), "flagged": aepe(r.forward, flagged),
                           "consistent": aepe(r.forward, rest)},
           "aepe_after": {"all": aepe(second, known), "flagged": aepe(second, flagged),
                          "consistent": aepe(second, rest)}}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
