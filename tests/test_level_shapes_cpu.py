"""CPU half of the level shape sweep (tests/test_gpu_level_shapes.py).

1. level_numpy.level_loop with the oracle's float64 stages reproduces the
   oracle's own level (oracle.compute_flow_base: hs_base / irls_base of
   optflow_oracle.c, pinned to the reference by test_oracle_golden.py) to
   1e-12 relative, for every unweighted arm and shape of the GPU sweep: the
   duv bookkeeping, mf_iter, the clip and the exit test are transcribed right.
2. The inputs meet the conditions the GPU comparisons lean on (a failing
   shape or seed is replaced, not excused).
3. Planted bugs in the numpy model of of_flow_update move the occlusion map
   by >= 10 x the 1e-5 bound the GPU test holds it to.

Every test prints a line "level_shapes | what | shape | figure".
"""
import functools

import numpy as np
import pytest

import level_inputs as L
import level_numpy as LN
import oracle as O
import stage_inputs as S

UNWEIGHTED = [a[0] for a in L.ARMS if not a[5]]


def _say(what, hw, fig):
    print(f"level_shapes | {what} | {hw[0]}x{hw[1]} | {fig}")


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


@functools.lru_cache(maxsize=None)
def _in(H, W):
    d = L.make(H, W)
    for a in d.values():
        a.setflags(write=False)
    return d


# ---- 1. the loop against the oracle's level, and the conditions on its x ------
@pytest.mark.parametrize("name", UNWEIGHTED)
@pytest.mark.parametrize("H,W", L.SMALL, ids=_ids(L.SMALL))
def test_loop_equals_the_oracle_level(H, W, name):
    ope, images, guide, uv0, _ = L.arm(name, H, W, _in(H, W))
    trace = []
    got = LN.level_loop(LN.OracleBackend(), ope, images, guide, uv0, None, trace)
    ref = O.compute_flow_base(ope, uv0)
    err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)) if np.abs(ref).max() > 0 else \
        float(np.abs(got).max())
    xs = np.concatenate([np.abs(t[2]).ravel() for t in trace])
    norms = [t[3] for t in trace]
    _say(f"loop vs oracle, {name}", (H, W),
         f"rel err {err:.1e} solves {len(trace)} |x| min {xs.min():.2e} max {xs.max():.2e} "
         f"||x|| {' '.join(f'{n:.3g}' for n in norms)}")
    assert err <= 1e-12, err
    if name == "hs exit":
        # the exit is taken at the first warp, from an exact zero
        assert len(trace) == 1 and norms[0] == 0.0 and np.array_equal(got, uv0)
        return
    n_out = int(ope.max_warping_iters if ope._METHOD == 'hs' else ope.max_iters * ope.max_linear)
    assert len(trace) == n_out, (len(trace), n_out)  # no early exit elsewhere
    if ope._METHOD == 'hs':
        # ||x|| a factor 10 away from the 1e-3 exit at every warp: the float32
        # level takes the same branch as this float64 loop
        assert all(n >= 1e-2 or n <= 1e-4 for n in norms), norms
    if ope.limit_update:
        # the clip acts on some component of the case's x and leaves another alone
        assert (xs > 1).any() and (xs < 1).any(), (xs.min(), xs.max())


# ---- 2. conditions on the inputs ---------------------------------------------
@pytest.mark.parametrize("H,W", L.SMALL + [L.BIG], ids=_ids(L.SMALL + [L.BIG]))
def test_input_conditions(H, W):
    d = _in(H, W)
    x, w = d["x"], d["weight"]
    for k in ("x", "uvs", "weight", "uv", "images3", "guide"):
        assert np.array_equal(d[k], d[k].astype(np.float32).astype(np.float64)), k
    big = (np.abs(x) > 1).all(axis=2)
    # clipped pixels in column 0, in column W - 1, in row 0 and at the first
    # pixel of a row (of the last row: its k - 1 is another row's end)
    assert big[:, 0].any() and big[:, W - 1].any() and big[0, :].any() and big[H - 1, 0]
    assert (np.abs(x) < 1).all(axis=2).any() or H * W <= len(L.forced_positions(H, W))
    if H * W >= 20:
        assert (w == 0).any() and (w == 1).any() and (w > 1).any()
    # some sample of the warp stays in the plane (one row / column included):
    # the assembly has a data term to work on
    inside = int((O.partial_deriv(d["images"], d["uv"], "bi-linear", S.FILT, 0.5)[0] != 0).sum())
    assert inside >= min(3, H * W // 2), inside
    _say("inputs", (H, W), f"clipped px {int(big.sum())} of {H * W}, weight zeros {int((w == 0).sum())} "
         f"ones {int((w == 1).sum())} above one {int((w > 1).sum())}, samples in the plane {inside}")


# ---- 3. planted bugs in the model of of_flow_update ---------------------------
def _acts(mutant, H, W):
    """left_unclipped needs a left neighbour, upper_at_W an upper one and a
    pitch that is not W; no_col0_guard acts on every plane."""
    return {"left_unclipped": W > 1, "upper_at_W": H > 1 and L.pitch(W) != W, "no_col0_guard": True}[mutant]


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("H,W", L.SMALL + [L.BIG], ids=_ids(L.SMALL + [L.BIG]))
def test_model_of_flow_update_and_its_mutants(H, W, nc):
    d = _in(H, W)
    images = d["images"] if nc == 1 else d["images3"]
    uv1, occ = LN.flow_update_model(d["uvs"], d["x"], True, images, L.pitch(W))
    ref = O.detect_occlusion(uv1, images)
    e0 = float(np.abs(occ - ref).max())
    figs = [f"model vs oracle {e0:.1e} occ max {ref.max():.2f}"]
    assert e0 <= 1e-12, e0
    for m in ("left_unclipped", "upper_at_W", "no_col0_guard"):
        if not _acts(m, H, W):
            continue
        _, bad = LN.flow_update_model(d["uvs"], d["x"], True, images, L.pitch(W), m)
        e = float(np.abs(bad - ref).max())
        figs.append(f"{m} {e:.1e}")
        assert e >= 10 * 1e-5, (m, e)
    _say(f"update model nc {nc}", (H, W), " ".join(figs))
