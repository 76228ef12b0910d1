"""CPU tests of the blind temporal consistency (include/optflow.h, "Blind
temporal consistency"): the screened multigrid schedule itself, on the numpy
float64 restatement (tests/screen_numpy.py) against an exact sparse solve, the
consistency step's quality on the inpainting scene along the known flows, the
Python validators and the C ABI mirror.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import poisson_numpy as pn
import screen_numpy as sn

# the shapes of the GPU tests, and one with four levels
SHAPES = [(1, 1), (1, 7), (9, 1), (2, 2), (37, 53), (48, 65), (40, 129), (200, 300)]
# sigma is what the original frames differ by where they show the same surface: on the scene the root mean square of
# frame t minus frame t-1 warped along the true flow, over the truly visible pixels, is 0.69 (test_sigma_is_the_scene_s)
SIGMA = 0.7


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_new_functions():
    import optical_flow
    for name in ("screened_poisson", "consistency_step", "TemporalConsistency", "consistent_frames"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    p = inspect.signature(optical_flow.screened_poisson).parameters
    assert list(p)[:3] == ["target", "anchor", "weight"]
    assert (p["cycles"].default, p["sweeps"].default, p["coarse_sweeps"].default) == (sn.CYCLES, sn.SWEEPS, sn.COARSE)
    p = inspect.signature(optical_flow.consistency_step).parameters
    assert list(p)[:7] == ["frame", "prev_frame", "processed", "prev_out", "flow", "state", "lam"]
    assert (p["state"].default, p["lam"].default, p["sigma"].default, p["strength"].default, p["patch"].default,
            p["cycles"].default) == (None, sn.LAMBDA, None, 4.0, 1, sn.CYCLES)
    p = inspect.signature(optical_flow.TemporalConsistency.__init__).parameters
    assert list(p)[1:4] == ["shape", "processed_channels", "method"]
    assert (p["processed_channels"].default, p["method"].default, p["sigma"].default) == (None, "classic+nl-fast", None)
    assert issubclass(optical_flow.TemporalConsistency, __import__("optical_flow._session", fromlist=["Session"]).Session)
    assert optical_flow.TemporalConsistency._KIND is None  # not a kind of_session_set_flow_scale takes
    p = inspect.signature(optical_flow.consistent_frames).parameters
    assert list(p)[:2] == ["frames", "processed"] and p["sigma"].default is None and p["lam"].default == 1.0


def test_c_abi_mirror_declares_the_five_entries():
    from optical_flow import _abi, _native
    want = {"of_screened_solve": 9, "of_consist_step": 14, "of_consist_open": 7, "of_consist_push": 5,
            "of_consist_close": 1}
    for name, nargs in want.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _abi.OF_ABI_VERSION == 3
    assert ctypes.sizeof(_abi.OfConsistOpts) == 64
    assert not any(n.startswith("OF_SESSION_") and getattr(_abi, n) >= 8 for n in dir(_abi))  # no new kind bit


FIELDS = ["fuse", "solve", "lambda"]


def test_header_constants_and_struct_match_the_mirror(tmp_path):
    from conftest import ROOT
    from optical_flow import _abi
    offs = ", ".join(f"offsetof(of_consist_opts, {f})" for f in FIELDS)
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%d %d %d %zu %zu %zu'
           + " %zu" * len(FIELDS) + '\\n", OF_ABI_VERSION, OF_CONSIST_CYCLES, OF_CONSIST_MAX_CHANNELS, '
           "sizeof(of_fuse_opts), sizeof(of_blend_opts), sizeof(of_consist_opts), " + offs + ");}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[:3] == [3, _abi.CONSIST_CYCLES, _abi.CONSIST_MAX_CHANNELS] and out[:3] == [3, sn.CYCLES, 4]
    assert out[3:6] == [ctypes.sizeof(_abi.OfFuseOpts), ctypes.sizeof(_abi.OfBlendOpts),
                        ctypes.sizeof(_abi.OfConsistOpts)]
    names = [n for n, _ in _abi.OfConsistOpts._fields_]
    assert names == ["fuse", "solve", "lambda_"]
    assert out[6:] == [getattr(_abi.OfConsistOpts, n).offset for n in names]


def test_every_new_kernel_and_entry_is_in_the_unity_build():
    from conftest import ROOT
    csrc = os.path.join(ROOT, "optical-flow-python_amd", "csrc")
    drv = open(os.path.join(csrc, "driver.hip")).read()
    assert drv.index('#include "kernels_poisson.hip"') < drv.index('#include "kernels_screen.hip"')
    assert drv.index('#include "host_poisson.hip"') < drv.index('#include "host_screen.hip"')
    k = open(os.path.join(csrc, "kernels_screen.hip")).read()
    for name in ("k_scr_setup", "k_scr_coarsen_q", "k_scr_smooth", "k_scr_restrict", "k_scr_coarsest", "k_scr_store"):
        assert name + "(" in k


# ---- argument checks: ValueError before the library is touched --------------
@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


IM = np.zeros((8, 9))
IM3 = np.zeros((8, 9, 3))
FL = np.zeros((8, 9, 2))
BAD_SOLVE = [dict(cycles=v) for v in (0, 65, -1, 2.0, "2", None, True, float("nan"))] + \
    [dict(sweeps=v) for v in (0, 3, 1.0, None, True)] + [dict(coarse_sweeps=v) for v in (0, 65, 8.0, None, False)]
BAD_STEP = BAD_SOLVE + [dict(sigma=v) for v in (None, 0, -1.0, float("inf"), "auto", True)] + \
    [dict(lam=v) for v in (-1e-9, float("nan"), float("inf"), None, "1", True)] + \
    [dict(strength=0), dict(strength=float("nan")), dict(patch=-1), dict(patch=4), dict(patch=1.0)]


@pytest.mark.parametrize("kw", BAD_SOLVE + [
    dict(target=np.zeros(8)), dict(target=np.zeros((8, 9, 5))), dict(target=np.zeros((0, 9))),
    dict(target=np.full((8, 9), np.nan)), dict(target=IM.astype(str)), dict(anchor=np.zeros((9, 8))),
    dict(anchor=IM3), dict(anchor=np.full((8, 9), np.inf)), dict(anchor=None), dict(weight=np.zeros((9, 8))),
    dict(weight=IM3), dict(weight=np.full((8, 9), -1e-300)), dict(weight=np.full((8, 9), np.nan)),
    dict(weight=np.full((8, 9), np.inf)), dict(weight=None), dict(weight=IM.astype(str))])
def test_screened_poisson_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(target=IM, anchor=IM, weight=IM)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.screened_poisson(**a)


@pytest.mark.parametrize("kw", BAD_STEP + [
    dict(frame=np.zeros(8)), dict(frame=np.zeros((8, 9, 5))), dict(frame=np.full((8, 9), np.nan)),
    dict(prev_frame=IM3), dict(prev_frame=np.zeros((9, 8))), dict(processed=np.zeros((9, 8))),
    dict(processed=np.zeros((8, 9, 5))), dict(processed=np.full((8, 9), np.inf)), dict(prev_out=IM3),
    dict(processed=IM3), dict(flow=np.zeros((8, 9))), dict(flow=np.zeros((9, 8, 2))),
    dict(state=np.zeros((9, 8), np.uint8)), dict(state=np.zeros((8, 9)))])
def test_consistency_step_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(frame=IM, prev_frame=IM, processed=IM, prev_out=IM, flow=FL, sigma=2.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.consistency_step(**a)


@pytest.mark.parametrize("kw", BAD_STEP + [dict(alpha1=-1.0), dict(alpha2=float("nan")), dict(processed_channels=0),
                                           dict(processed_channels=5), dict(processed_channels=3.0),
                                           dict(shape=(8, 9, 2)), dict(shape=(8,)), dict(shape=(0, 9)),
                                           dict(method="no such method")])
def test_session_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(shape=(8, 9), sigma=2.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.TemporalConsistency(**a)


@pytest.mark.parametrize("kw", BAD_STEP + [dict(frames=[]), dict(frames=[IM, np.zeros((9, 8))]),
                                           dict(frames=[IM, np.full((8, 9), np.nan)]), dict(processed=[IM]),
                                           dict(processed=[]), dict(processed=[IM, np.zeros((9, 8))]),
                                           dict(processed=[np.zeros((8, 9, 5))] * 2),
                                           dict(processed=[np.zeros((9, 8))] * 2),
                                           dict(processed=[IM, np.full((8, 9), np.nan)]),
                                           dict(frames=[np.zeros((8, 9, 2))] * 2)])
def test_consistent_frames_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(frames=[IM, IM], processed=[IM, IM], sigma=2.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.consistent_frames(**a)


# ---- the schedule -----------------------------------------------------------
def test_levels_depend_on_the_frame_size_alone():
    got = {s: sn.levels(*s) for s in ((1, 1), (30, 30), (31, 30), (48, 64), (200, 300), (1080, 1920))}
    assert [got[s][0] for s in got] == [pn.n_levels(*s) for s in got] == [0, 0, 1, 1, 4, 6]
    assert got[(1, 1)][1] == [(-1, -1, 3, 3)] and got[(30, 30)][1] == [(-1, -1, 32, 32)]
    assert got[(31, 30)][1] == [(-2, -2, 36, 34), (-1, -1, 18, 17)]
    # every window holds its grid and an apron, is twice the next one and anchored at the origin
    for (H, W), (L, wins) in got.items():
        for l, (r0, c0, h, w) in enumerate(wins):
            assert r0 == c0 == -(1 << (L - l)) and h + r0 >= -(-H >> l) + 1 and w + c0 >= -(-W >> l) + 1
            if l < L:
                assert (h, w) == (2 * wins[l + 1][2], 2 * wins[l + 1][3])
        assert wins[-1][2] * wins[-1][3] <= pn.CMAX


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("H,W", SHAPES[:-1])
def test_zero_weight_returns_the_target_to_the_bit(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    P = rng.uniform(0, 255, (3, H, W)).astype(np.float32).astype(np.float64)
    A = rng.uniform(-1e3, 1e3, (3, H, W))
    x = sn.solve(P, A, np.zeros((H, W)))
    assert np.array_equal(_bits(x), _bits(P))


def test_degenerate_frames():
    P, A = np.full((1, 1, 1), 7.0), np.full((1, 1, 1), 3.0)
    assert sn.solve(P, A, np.zeros((1, 1)))[0, 0, 0] == 7.0           # deg = 0 and q = 0: the start stays
    assert sn.solve(P, A, np.full((1, 1), 0.3))[0, 0, 0] == (0.3 * 3.0) / 0.3
    # one pixel anchored hard pins the constant: everything moves by the anchor's offset
    rng = np.random.default_rng(0)
    P = rng.uniform(0, 255, (1, 9, 11)).astype(np.float32).astype(np.float64)
    q = np.zeros((9, 11))
    q[4, 5] = 1e6
    x = sn.solve(P, P + 10.0, q, cycles=40)
    assert np.abs(x - (P + 10.0)).max() < 1e-3


# ---- accuracy against the exact solve ---------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_default_options_reach_half_a_level(H, W):
    """max |x - exact| <= 0.5 on a 0..255 scale with the default options
    (5 cycles), q in patches of 0, 1e-3, 1 and 1e3, the anchor off by 10 % gain
    + 12 with sigma = 3 noise.  Measured per cycle (cycles 1 .. 8), correction
    factor 1.5:
      37 x 53    12    5     2.2   0.91  0.38  0.16  0.064  0.026
      48 x 65    5.3   2.3   0.79  0.29  0.11  0.039 0.014  0.0051
      40 x 129   7     1.2   0.28  0.077 0.02  0.0052 0.0013 0.00035
      200 x 300  14    6     2.5   1     0.43  0.18  0.072  0.029
    and at most 0.0054 after one cycle on the four single-level frames.  Four
    cycles leave 0.91 and 1.0: 5 is the smallest count within 0.5.  With a
    factor of 1.25 the fifth cycle leaves 1.8, with 1.0 it leaves 6.7."""
    pytest.importorskip("scipy")
    P, A, q = sn.convergence_case(H, W)
    assert set(np.unique(q)) <= {0.0, 1e-3, 1.0, 1e3} and (H * W < 16 or len(np.unique(q)) == 4)
    ex = sn.exact(P, A, q)
    errs = []
    sn.solve(P, A, q, trace=lambda k, x: errs.append(float(np.abs(x - ex).max())))
    print((H, W), "L", pn.n_levels(H, W), " ".join(f"{e:.2g}" for e in errs))
    assert len(errs) == sn.CYCLES
    assert errs[-1] <= 0.5


# ---- the consistency step on the scene, along the known flows ---------------
@pytest.fixture(scope="module")
def known():
    """The scene, its flickering processed clip and the prototype's results
    along the true flows with the true visibility as the state."""
    frames, bw, vis = sn.scene_truth()
    proc = sn.flicker_clip(frames)
    states = [(~v).astype(np.uint8) for v in vis]
    outs = sn.clip(frames, proc, bw, states, sigma=SIGMA)
    same = sn.clip(frames, frames, bw, states, sigma=SIGMA)
    return frames, bw, vis, states, proc, outs, same


def quality_gates(known, outs, same, label):
    """The issue's gates on a result `outs` of the flickering clip and `same`
    of the clip itself; returns the measured values."""
    frames, bw, vis, _, proc, ref, ref_same = known
    a = sn.instability(proc, bw, vis)
    b = sn.instability(ref, bw, vis)
    fid_ref = sn.fidelity(ref, proc)
    mse_ref = float(np.mean([(np.float64(o) - f) ** 2 for o, f in zip(ref_same, frames)]))
    inst, fid = sn.instability(outs, bw, vis), sn.fidelity(outs, proc)
    mse = float(np.mean([(np.float64(o) - f) ** 2 for o, f in zip(same, frames)]))
    print(f"{label}: instability {inst:.4f} (processed {a:.4f}, known flows {b:.4f}, gate {np.sqrt(a * b):.4f}); "
          f"fidelity {fid:.4f} (known flows {fid_ref:.4f}); unchanged clip: MSE {mse:.4f} (known flows {mse_ref:.4f})")
    assert inst < np.sqrt(a * b)
    assert fid <= 2 * fid_ref
    assert mse < 2 * mse_ref
    return a, b, fid_ref, mse_ref


def test_sigma_is_the_scene_s(known):
    import fuse_numpy as fn
    frames, bw, vis = known[:3]
    d2 = []
    for k in range(1, len(frames)):
        _, _, r, q, ok = fn._landing(bw[k - 1])
        d = frames[k].astype(np.float64) - fn.bil(frames[k - 1].astype(np.float64), r, q)
        d2.append(d[vis[k - 1] & ok] ** 2)
    rms = float(np.sqrt(np.concatenate(d2).mean()))
    print("the scene's frames differ along the true flows by", rms)
    assert abs(rms - SIGMA) < 0.05


def test_scene_quality_along_the_known_flows(known):
    """inpaint_numpy.scene(0), 9 frames of 48 x 64; the processed clip is frame
    t times 1 +- 0.08 plus +- 6 (seed 5); sigma 0.7, lambda 1, 5 cycles.
    Measured along the true flows with the true visibility as the state:
    instability 81.94 of the processed clip, 0.870 of the result (the gate for
    estimated flows is their geometric mean, 8.44); fidelity 0.537; a
    processed clip equal to the frames comes back with an MSE of 2.50 (the
    bilinear resampling of the texture by the sub-pixel flow, step after
    step).  Each step's solve is within 0.0036 of the exact one after 5
    cycles.  (With sigma 2: 0.813, 0.567 and 2.94.)"""
    frames, bw, vis, states, proc, outs, same = known
    a, b, fid, mse = quality_gates(known, outs, same, "known flows")
    assert 75 < a < 90 and b < a / 50 and fid < 1.0 and mse < 4.0
    # push 0 is the processed frame; lambda 0 returns the processed clip to the bit
    assert np.array_equal(outs[0].view(np.uint32), proc[0].view(np.uint32))
    off = sn.clip(frames[:3], proc[:3], bw[:2], states[:2], sigma=SIGMA, lam=0.0)
    assert all(np.array_equal(o.view(np.uint32), p.view(np.uint32)) for o, p in zip(off, proc))
    # a large lambda returns the warped previous output where it is visible
    import fuse_numpy as fn
    big, w = sn.step(frames[1], frames[0], proc[1], proc[0], bw[0], states[0], lam=1e9, sigma=SIGMA)
    _, _, r, q, _ = fn._landing(bw[0])
    warped = fn.bil(proc[0].astype(np.float64), r, q)
    lean = w == 1.0
    assert lean.mean() > 0.5 and np.abs(big - warped)[lean].max() < 1e-3
    # every step's solve is converged
    pytest.importorskip("scipy")
    worst = 0.0

    def solver(P, A, q, **kw):
        nonlocal worst
        x = sn.solve(P, A, q, **kw)
        worst = max(worst, float(np.abs(x - sn.exact(P, A, q)).max()))
        return x

    prev = proc[0]
    for k in range(1, len(frames)):
        prev = sn.step(frames[k], frames[k - 1], proc[k], prev, bw[k - 1], states[k - 1], sigma=SIGMA, solver=solver)[0]
    print("scene: the worst step's distance to the exact solve", worst)
    assert worst <= 0.5
