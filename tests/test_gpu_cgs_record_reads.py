"""k_cgs after the record-read change (waves 2 and 3 keep the ring records and
the s_g1 / s_yq rows they read in registers for the steps that need them
again): every K-th iterate bit for bit the one recorded from the commit
before it, on shapes whose walks end at every position of the 8-step trip.
Cases, shapes and fixtures: tests/cgs_record_reads_cases.py.

Every test prints a line "cgs_record_reads | id | iters | sha1 | differing values".
"""
import functools

import numpy as np
import pytest

import cgs_record_reads_cases as RR

pytestmark = pytest.mark.gpu

CASES = RR.cases()


@functools.lru_cache(maxsize=None)
def _fixtures():
    return RR.load_fixtures()


@functools.lru_cache(maxsize=None)
def _system(H, W, kind):
    A, b = RR.system(H, W, kind)
    b.setflags(write=False)
    return A, b


def test_fixtures_cover_the_cases():
    sha, arrays = _fixtures()
    assert sorted(sha) == sorted(c["id"] for c in CASES)
    want = sorted(c["id"] for c in CASES if (c["H"], c["W"]) in RR.ARRAY_SHAPES and c["kind"] == "plain")
    assert sorted(arrays) == want
    for k, v in arrays.items():
        assert v.dtype == np.float32 and RR.digest(v) == sha[k]["sha1"], k


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_iterate_bitwise(i):
    c = CASES[i]
    sha, arrays = _fixtures()
    A, b = _system(c["H"], c["W"], c["kind"])
    x, iters, ran = RR.solve(c, A, b)
    want = sha[c["id"]]
    got = RR.digest(x)
    ndiff = ""
    if c["id"] in arrays:
        ref = arrays[c["id"]]
        ndiff = int((x.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"cgs_record_reads | {c['id']} | iters {iters} (recorded {want['iters']}) | {got} | {ndiff}")
    assert "pcg_iter" in ran and not {"pcg_small", "dia_dir"} & ran, ran
    assert iters == want["iters"], (iters, want)
    if c["K"] is not None:
        assert iters == c["K"], iters
    if c["id"] in arrays:
        np.testing.assert_array_equal(x.view(np.uint32), arrays[c["id"]].view(np.uint32))
    assert got == want["sha1"], (got, want)
