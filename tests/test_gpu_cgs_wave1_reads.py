"""k_cgs after the wave-1 read change (wave 1 keeps the ring records of rows
n-3 .. n-6 and the s_y rows it read in registers for the steps that need them
again): every K-th iterate bit for bit the one recorded from the commit before
it, on odd-width shapes (the ODD instances) whose walks end at every position
of the 8-step trip.  Cases, shapes and fixtures: tests/cgs_wave1_reads_cases.py.

Every test prints a line "cgs_wave1_reads | id | iters | sha1 | differing values".
"""
import functools

import numpy as np
import pytest

import cgs_wave1_reads_cases as WR

pytestmark = pytest.mark.gpu

CASES = WR.cases()


@functools.lru_cache(maxsize=None)
def _fixtures():
    return WR.load_fixtures()


@functools.lru_cache(maxsize=None)
def _system(H, W, kind):
    A, b = WR.system(H, W, kind)
    b.setflags(write=False)
    return A, b


def test_fixtures_cover_the_cases():
    sha, arrays = _fixtures()
    assert len(CASES) == 103
    assert sorted(sha) == sorted(c["id"] for c in CASES)
    want = sorted(c["id"] for c in CASES if (c["H"], c["W"]) in WR.ARRAY_SHAPES and c["kind"] == "plain")
    assert sorted(arrays) == want
    for k, v in arrays.items():
        assert v.dtype == np.float32 and WR.digest(v) == sha[k]["sha1"], k


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_iterate_bitwise(i):
    c = CASES[i]
    sha, arrays = _fixtures()
    A, b = _system(c["H"], c["W"], c["kind"])
    x, iters, ran = WR.solve(c, A, b)
    want = sha[c["id"]]
    got = WR.digest(x)
    ndiff = ""
    if c["id"] in arrays:
        ref = arrays[c["id"]]
        ndiff = int((x.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"cgs_wave1_reads | {c['id']} | iters {iters} (recorded {want['iters']}) | {got} | {ndiff}")
    assert "pcg_iter" in ran and not {"pcg_small", "dia_dir"} & ran, ran
    assert iters == want["iters"], (iters, want)
    if c["K"] is not None:
        assert iters == c["K"], iters
    if c["id"] in arrays:
        np.testing.assert_array_equal(x.view(np.uint32), arrays[c["id"]].view(np.uint32))
    assert got == want["sha1"], (got, want)
