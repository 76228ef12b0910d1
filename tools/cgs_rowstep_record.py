"""Record the fixtures of tests/test_gpu_cgs_rowstep.py, or with --set
record_reads / wave1_reads those of tests/test_gpu_cgs_record_reads.py /
tests/test_gpu_cgs_wave1_reads.py, from the library in the tree (to be run
on the commit whose iterates are the reference):

    python tools/cgs_rowstep_record.py [--set rowstep] [--out tests/golden]

Writes cgs_<set>_sha1.json ({case id: {sha1, iters}}) and
cgs_<set>_iterates.npz (float32 iterates of the two smallest shapes).
Each solve runs twice and must reproduce itself bit for bit.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "optical-flow-python_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="rowstep", choices=["rowstep", "record_reads", "wave1_reads"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    RC = importlib.import_module(f"cgs_{args.set}_cases")
    args.out = args.out or RC.GOLDEN
    sha, arrays, systems = {}, {}, {}
    for c in RC.cases():
        key = (c["H"], c["W"], c["kind"])
        if key not in systems:
            systems[key] = RC.system(*key)
        A, b = systems[key]
        x, iters, ran = RC.solve(c, A, b)
        x2, iters2, _ = RC.solve(c, A, b)
        assert "pcg_iter" in ran, (c["id"], ran)
        assert iters == iters2 and RC.digest(x) == RC.digest(x2), c["id"]
        sha[c["id"]] = dict(sha1=RC.digest(x), iters=iters)
        if (c["H"], c["W"]) in RC.ARRAY_SHAPES and c["kind"] == "plain":
            arrays[c["id"]] = x
        print(f"{c['id']}: iters {iters} finite {bool(np.all(np.isfinite(x)))} max|x| {np.abs(x).max():.4g} "
              f"{sha[c['id']]['sha1']}", flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"cgs_{args.set}_sha1.json"), "w") as f:
        json.dump(sha, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(args.out, f"cgs_{args.set}_iterates.npz"), **arrays)


if __name__ == "__main__":
    main()
