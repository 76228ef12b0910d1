"""Time of one temporal-consistency push on a 1080p RGB clip: the wall time of
the push that estimates a pair and runs the step, beside the temporal
denoiser's push on the same frames (the two flow estimates and a fusion), and
the kernel time of that push by kernel name and launch count from a
`rocprofv3 --kernel-trace --stats` run of its own.

    python tools/consist_time.py [--out profiles/consist_time.json] [--size 1080 1920] [--runs 2]

Every GPU step is a child process of its own under its own `timeout`; a step
that fails or runs out of time ends the tool there.  The steps:
  wall  --worker consist / --worker denoise, `--runs` times each: a warm-up
        session of two pushes, then a fresh session whose second push is timed
  trace rocprofv3 --kernel-trace --stats -- ... --worker trace: one session,
        two pushes, nothing else, so the kernels of the process are those of
        one pair estimate and one step (push 0 launches nothing)
The solve's kernels are scr_*, psn_prolong, psn_coarsen and fuse_weights; every
other kernel belongs to the two flow estimates of the pair."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "optical-flow-python_amd"))

METHOD = "classic+nl-fast"
SIGMA = 4.0
SOLVE = ("k_scr_", "k_psn_prolong", "k_psn_coarsen", "k_fuse_weights")
STEP_TIMEOUT = 240  # seconds, each child


def clip(H, W):
    """Three frames of a textured 1080p RGB pair and their processed versions:
    the frames times a per-frame gain plus an offset."""
    import numpy as np
    from optical_flow.utils.synthetic import synth_pair
    im1, im2, _ = synth_pair(H, W, 0)
    frames = [np.asarray((im1, im2)[k & 1], np.float32) for k in range(3)]
    if frames[0].ndim == 2:
        frames = [np.repeat(f[..., None], 3, axis=2) for f in frames]
    proc = [f * np.float32(1.0 + 0.05 * (-1) ** k) + np.float32(4 * k) for k, f in enumerate(frames)]
    return frames, proc


def worker(kind, H, W):
    import optical_flow
    frames, proc = clip(H, W)

    def consist(timed):
        with optical_flow.TemporalConsistency(frames[0].shape, 3, METHOD, sigma=SIGMA) as tc:
            tc.push(frames[0], proc[0])
            t0 = time.perf_counter()
            tc.push(frames[1], proc[1])
            return time.perf_counter() - t0

    def denoise(timed):
        with optical_flow.TemporalDenoiser(frames[0].shape, METHOD, sigma=SIGMA, radius=1) as dn:
            dn.push(frames[0])
            t0 = time.perf_counter()
            dn.push(frames[1])
            return time.perf_counter() - t0

    if kind == "trace":
        consist(True)
        return {}
    run = consist if kind == "consist" else denoise
    run(False)  # warm-up: the arena and the lanes at their final size
    return {"kind": kind, "push_wall_ms": 1e3 * run(True)}


def child(args, extra, prefix=()):
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT)] + list(prefix) + \
        [sys.executable, os.path.abspath(__file__), "--size", str(args.size[0]), str(args.size[1])] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"step {' '.join(extra)} ended with status {r.returncode}: nothing more is started\n{r.stderr[-2000:]}")
    return r.stdout


def kernel_stats(folder):
    """name -> (total ms, launches) of the kernel statistics rocprofv3 left under `folder`."""
    files = glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel statistics under {folder}")
    out = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            ms, n = float(row["TotalDurationNs"]) * 1e-6, int(row["Calls"])
            a = out.get(row["Name"], (0.0, 0))
            out[row["Name"]] = (a[0] + ms, a[1] + n)
    return out


def short(name):
    """k_scr_smooth<3>(...) or void k_scr_smooth<3>(...) -> k_scr_smooth<3>"""
    name = name.split("(")[0].strip()
    return name[5:] if name.startswith("void ") else name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consist_time.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--worker", choices=("consist", "denoise", "trace"), default=None)
    args = ap.parse_args()
    H, W = args.size
    if args.worker:
        print(json.dumps(worker(args.worker, H, W)))
        return 0
    rec = {"size": [H, W], "channels": 3, "method": METHOD, "sigma": SIGMA}
    for kind in ("consist", "denoise"):
        rec[kind + "_push_wall_ms"] = [json.loads(child(args, ["--worker", kind]).strip().splitlines()[-1])["push_wall_ms"]
                                       for _ in range(max(args.runs, 2))]
    with tempfile.TemporaryDirectory() as d:
        child(args, ["--worker", "trace"],
              ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "consist", "--"])
        k = kernel_stats(d)
    solve = {short(n): {"ms": v[0], "launches": v[1]} for n, v in k.items() if short(n).startswith(SOLVE)}
    rest = [v for n, v in k.items() if not short(n).startswith(SOLVE)]
    rec["solve"] = {"kernels": solve, "ms": sum(v["ms"] for v in solve.values()),
                    "launches": int(sum(v["launches"] for v in solve.values()))}
    rec["flow_estimates"] = {"ms": sum(v[0] for v in rest), "launches": int(sum(v[1] for v in rest))}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
