"""Cases and fixtures of test_gpu_cgs_wave1_reads.py: K-th iterates of the
'backslash' solver (k_cgs) that must stay bit for bit what the commit before
the wave-1 read change computed (wave 1, the four Horner stages, carries the
ring records of rows n-3 .. n-6 and the s_y rows n-2 .. n-6 in registers
instead of reading them again at every row step).

The fixtures under tests/golden/ were recorded on an MI355X from that commit
with tools/cgs_rowstep_record.py --set wave1_reads: cgs_wave1_reads_sha1.json
holds the sha1 of the float32 bytes of every iterate (and the iteration count
the solve reported), cgs_wave1_reads_iterates.npz the iterates themselves for
the two smallest shapes.

The shapes of cgs_record_reads_cases.py are even-width (the only odd width of
the older gates is 17 x 241).  The ODD instances of the kernel are code
objects of their own, with their own register allocation and spilled SGPRs,
so these cases put them through every position of the 8-step trip: the same
heights, each with the smallest odd width >= 71 that puts it above the 4096
px below which a level never reaches k_cgs (width_of).  A band of r rows walks
r + 20 row steps, a flipped one r + 21 (walk_steps, from of_solver_geometry;
tests/test_cgs_wave1_reads_cpu.py asserts it):

  H = 1 .. 8                one unflipped band of H rows: 21 .. 28 steps
  H = 9, 10, 12, 14, 16     two bands, the flipped second one of 4 .. 8 rows:
                            25 .. 29 steps
  H = 57, 58, 59            eight bands of 8 rows, the flipped last one of 1,
                            2, 3 rows: 22, 23, 24 steps
  59 x 231                  the same bands over a strip seam (two strips)

Each shape with the quadratic operator (alpha = 1.0) and the robust one
(alpha = 0.0) at K = 1 (the FIRST instance), 2 and 8 with rtol 0, and one
solve with the default tolerances on 59 x 231 (residual replacement and the
x_lo = 0 path): 103 cases.
"""
import json
import os

import numpy as np

import cgs_rowstep_cases as RC
from cgs_record_reads_cases import walk_steps  # noqa: F401  (geometry only, no device)

GOLDEN = RC.GOLDEN
SHA1_FILE = os.path.join(GOLDEN, "cgs_wave1_reads_sha1.json")
NPZ_FILE = os.path.join(GOLDEN, "cgs_wave1_reads_iterates.npz")

SMALL_PX = 4096  # CG_SMALL_PX: at most this many pixels never reach k_cgs
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 57, 58, 59]
SEAM_SHAPE = (59, 231)
ALPHAS = (1.0, 0.0)
KS = (1, 2, 8)


def width_of(H):
    """the smallest odd width >= 71 that puts H rows above SMALL_PX"""
    w = SMALL_PX // H + 1
    return max(71, w | 1)


SHAPES = [(H, width_of(H)) for H in HEIGHTS] + [SEAM_SHAPE]
ARRAY_SHAPES = sorted(SHAPES, key=lambda s: s[0] * s[1])[:2]  # iterates kept as arrays


def cases():
    """dict(id, H, W, alpha, K, kind); K None: default tolerances"""
    out = []
    for H, W in SHAPES:
        for a in ALPHAS:
            for K in KS:
                out.append(dict(id=f"{H}x{W}-alpha{a:g}-K{K}", H=H, W=W, alpha=a, K=K, kind="plain"))
    H, W = SEAM_SHAPE
    out.append(dict(id=f"{H}x{W}-converged", H=H, W=W, alpha=1.0, K=None, kind="plain"))
    return out


system, solve, digest = RC.system, RC.solve, RC.digest


def load_fixtures():
    with open(SHA1_FILE) as f:
        sha = json.load(f)
    with np.load(NPZ_FILE) as z:
        arrays = {k: z[k] for k in z.files}
    return sha, arrays
