"""Cases and fixtures of test_gpu_cgs_record_reads.py: K-th iterates of the
'backslash' solver (k_cgs) that must stay bit for bit what the commit before
the record-read change computed (waves 2 and 3 carry the ring records and the
s_g1 / s_yq rows they read in registers instead of reading them again).

The fixtures under tests/golden/ were recorded on an MI355X from that commit
with tools/cgs_record_reads_record.py: cgs_record_reads_sha1.json holds the
sha1 of the float32 bytes of every iterate (and the iteration count the solve
reported), cgs_record_reads_iterates.npz the iterates themselves for the two
smallest shapes.

What the carried values can get wrong: the first steps of a walk (carried
values before any row exists), the boundary between two 8-step trips, and the
last, partial trip, for unflipped (even) and flipped (odd) bands.  A band of
r rows walks r + 20 row steps, a flipped one r + 21, so the shapes are chosen
to make the walks of each kind cover every residue mod 8 (walk_steps below,
from of_solver_geometry; tests/test_cgs_record_reads_cpu.py asserts it):

  H = 1 .. 8                one unflipped band of H rows: 21 .. 28 steps
  H = 9, 10, 12, 14, 16     two bands, the flipped second one of 4 .. 8 rows:
                            25 .. 29 steps
  H = 57, 58, 59            eight bands of 8 rows, the flipped last one of 1,
                            2, 3 rows: 22, 23, 24 steps
  59 x 230                  the same bands over a strip seam

The issue that asked for these cases gave them all the width 70 (one strip
that owns all 128 lanes) and added 12 x 230.  Levels of at most 4096 px are
solved by the one-workgroup kernels and never reach k_cgs, which leaves only
59 x 70 and 59 x 230 of those, so every other height takes the smallest even
width that puts it above 4096 px (width_of): the band geometry depends on the
height alone there (cg_geometry caps the bands by 512 / strips, which none of
these widths reaches), the walks are the ones listed, and the wider shapes
have several strips, i.e. the seam that 12 x 230 was for.

Each shape with the quadratic operator (alpha = 1.0) and the robust one
(alpha = 0.0) at K = 1 (the FIRST instance), 2 and 8 with rtol 0, and one
solve with the default tolerances on 59 x 230.
"""
import json
import os

import numpy as np

import cgs_rowstep_cases as RC

GOLDEN = RC.GOLDEN
SHA1_FILE = os.path.join(GOLDEN, "cgs_record_reads_sha1.json")
NPZ_FILE = os.path.join(GOLDEN, "cgs_record_reads_iterates.npz")

SMALL_PX = 4096  # CG_SMALL_PX: at most this many pixels never reach k_cgs
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 57, 58, 59]
SEAM_SHAPE = (59, 230)
ALPHAS = (1.0, 0.0)
KS = (1, 2, 8)


def width_of(H):
    """70, or the smallest even width that puts H rows above SMALL_PX"""
    w = SMALL_PX // H + 1
    return max(70, w + (w & 1))


SHAPES = [(H, width_of(H)) for H in HEIGHTS] + [SEAM_SHAPE]
ARRAY_SHAPES = sorted(SHAPES, key=lambda s: s[0] * s[1])[:2]  # iterates kept as arrays


def walk_steps(H, W):
    """[(row steps, flipped)] of the bands of an H x W level, from the geometry
    the library reports (no device): band i holds rows [i R, min((i + 1) R, H))
    and an odd band is walked flipped, one step further"""
    from optical_flow import _native
    g = _native.solver_geometry(H, W, "backslash")
    R, nb = g["rows"], g["bands"]
    return [(min((i + 1) * R, H) - i * R + 20 + (i & 1), bool(i & 1)) for i in range(nb)]


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
