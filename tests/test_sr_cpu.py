"""CPU tests of the multi-frame super-resolution (include/optflow.h,
"Multi-frame super-resolution along the flow"): the formula itself, on the
numpy float64 restatement (tests/sr_numpy.py), the Python validators and the
C ABI mirror.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import sr_numpy as sn
import upsample_numpy as un


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_new_functions():
    import optical_flow
    for name in ("fuse_weights", "super_resolve", "SuperResolver", "super_resolve_frames"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    p = inspect.signature(optical_flow.super_resolve).parameters
    assert list(p) == ["center", "neighbours", "flows", "factor", "sigma", "states", "strength", "patch", "reach",
                       "back", "return_support"]
    assert (p["strength"].default, p["patch"].default, p["reach"].default, p["back"].default) == (4.0, 2, 0.75, 0.0)
    p = inspect.signature(optical_flow.fuse_weights).parameters
    assert list(p) == ["center", "neighbours", "flows", "sigma", "states", "strength", "patch"]
    p = inspect.signature(optical_flow.SuperResolver.__init__).parameters
    assert p["factor"].default == 2 and p["radius"].default == 2 and p["sigma"].default is None
    assert "scale" not in p  # the upscale factor is `factor`; `scale` means flow reduction
    p = inspect.signature(optical_flow.super_resolve_frames).parameters
    assert p["factor"].default == 2 and "scale" not in p


def test_c_abi_mirror_declares_the_six_entries():
    from optical_flow import _abi, _native
    want = {"of_fuse_weights": 11, "of_super_resolve": 12, "of_sr_open": 6, "of_sr_push": 5, "of_sr_flush": 4,
            "of_sr_close": 1}
    for name, nargs in want.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _abi.OF_ABI_VERSION == 3


FIELDS = ["factor", "radius", "patch", "pad_", "sigma", "strength", "reach", "back", "alpha1", "alpha2"]


def test_sr_opts_layout_matches_header(tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    from optical_flow import _abi
    offs = ", ".join(f"offsetof(of_sr_opts, {f})" for f in FIELDS)
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(FIELDS)
           + '\\n", sizeof(of_sr_opts), ' + offs + ");}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(_abi.OfSrOpts)] + [getattr(_abi.OfSrOpts, f).offset for f in FIELDS]
    assert ctypes.sizeof(_abi.OfSrOpts) == 64 and [n for n, _ in _abi.OfSrOpts._fields_] == FIELDS


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
FL = np.zeros((8, 9, 2))
BAD = ([dict(factor=f) for f in (0, 1, 5, 2.0, "2", None, True)]
       + [dict(sigma=v) for v in (None, 0, -1.0, float("nan"), float("inf"), "auto", True)]
       + [dict(strength=v) for v in (0, float("nan"), "4")]
       + [dict(patch=v) for v in (-1, 4, 1.0)]
       + [dict(reach=v) for v in (0.7, 1.6, 0, float("nan"), "1", None)]
       + [dict(back=v) for v in (-0.1, 1.1, float("inf"), None, "0")])


@pytest.mark.parametrize("kw", BAD + [dict(neighbours=[IM] * 9, flows=[FL] * 9), dict(neighbours=[np.zeros((8, 8))]),
                                      dict(flows=[]), dict(flows=[np.zeros((8, 9, 3))]), dict(states=[]),
                                      dict(states=[np.zeros((9, 8), np.uint8)]), dict(center=np.zeros((8, 9, 5))),
                                      dict(center=np.zeros(8))])
def test_super_resolve_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(center=IM, neighbours=[IM], flows=[FL], factor=2, sigma=5.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.super_resolve(**a)


@pytest.mark.parametrize("kw", BAD + [dict(radius=r) for r in (0, 3, 1.0)] + [dict(alpha1=-1.0),
                                                                              dict(alpha2=float("nan"))])
def test_session_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(factor=2, sigma=5.0)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.SuperResolver((8, 9), **a)
    with pytest.raises(ValueError):
        optical_flow.super_resolve_frames([IM, IM], **a)


def test_fuse_weights_and_shapes_raise_before_any_library_call(no_library):
    import optical_flow
    with pytest.raises(ValueError, match="sigma"):
        optical_flow.fuse_weights(IM, [IM], [FL])
    with pytest.raises(ValueError, match="neighbours"):
        optical_flow.fuse_weights(IM, [], [], 5.0)
    with pytest.raises(ValueError, match="shape"):
        optical_flow.SuperResolver((8, 9, 2), sigma=5.0)
    with pytest.raises(ValueError):
        optical_flow.super_resolve_frames([], sigma=5.0)
    with pytest.raises(ValueError, match="2\\^31"):
        optical_flow.SuperResolver((20000, 30000), factor=2, sigma=5.0)


# ---- properties of the restatement ------------------------------------------
def random_case(H, W, Cc, n, seed):
    rng = np.random.default_rng(seed)
    shp = (H, W) if Cc == 1 else (H, W, Cc)
    center = rng.uniform(0, 255, shp).astype(np.float32)
    neigh = [rng.uniform(0, 255, shp).astype(np.float32) for _ in range(n)]
    flows = [rng.uniform(-3, 3, (H, W, 2)).astype(np.float32) for _ in range(n)]
    return center, neigh, flows


@pytest.mark.parametrize("s", [2, 3, 4])
def test_constant_frames_come_back_exactly(s):
    H, W = 11, 14
    rng = np.random.default_rng(s)
    c = np.full((H, W, 3), 128.0, np.float32)
    flows = [rng.uniform(-4, 4, (H, W, 2)).astype(np.float32) for _ in range(4)]
    for reach, back in ((0.75, 0.0), (1.5, 0.5), (1.0, 1.0)):
        out, S = sn.super_resolve(c, [c] * 4, flows, s, 5.0, reach=reach, back=back)
        assert out.shape == (s * H, s * W, 3) and out.dtype == np.float32 and S.shape == (s * H, s * W)
        assert np.all(out == np.float32(128.0))
        assert np.all(S > 0)


@pytest.mark.parametrize("s", [2, 3])
def test_neighbours_whose_states_are_all_1_give_the_single_frame_result_bitwise(s):
    center, neigh, flows = random_case(13, 17, 3, 3, 40 + s)
    alone, S0 = sn.super_resolve(center, [], [], s, 20.0)
    states = [np.ones((13, 17), np.uint8)] * 3
    out, S = sn.super_resolve(center, neigh, flows, s, 20.0, states)
    assert np.array_equal(out.view(np.uint32), alone.view(np.uint32))
    assert np.array_equal(S.view(np.uint32), S0.view(np.uint32))
    more, S1 = sn.super_resolve(center, neigh, flows, s, 200.0)  # and without the states they do count
    assert (S1 > S0).any() and not np.array_equal(more, alone)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_back_1_reduces_back_to_the_centre_frame(s):
    center, neigh, flows = random_case(12, 15, 3, 2, 50 + s)
    out, _ = sn.super_resolve(center, neigh, flows, s, 200.0, back=1.0)
    err = float(np.abs(un.reduce_frame(out, s).astype(np.float64) - center).max())
    print(f"s={s}: max |reduce_frame(out) - centre| = {err:.3e} (4 ulp of 255 = {4 * 2.0 ** -16:.3e})")
    assert err <= 4 * 2.0 ** -16


# ---- the prototype scene, known flows, factor 2 -------------------------------
def test_prototype_scene_beats_the_bilinear_upsample():
    """48 x 64 frames of tex(1) box-reduced by 2, four neighbours at known
    sub-pixel offsets, noise-free, sigma 3 (1.5 * max(noise, 2)).  Measured
    interior MSE against the high-resolution truth: fused 6.96, bilinear
    upsample of the centre frame 17.39 (ratio 0.40)."""
    truth, center, neigh, flows = sn.scene(2)
    out, S = sn.super_resolve(center, neigh, flows, 2, 3.0)
    e_sr, e_bil = sn.interior_mse(out, truth, 2), sn.interior_mse(sn.bilinear_upsample(center, 2), truth, 2)
    print(f"prototype scene, factor 2, noise-free: fused {e_sr:.2f}, bilinear {e_bil:.2f}, ratio {e_sr / e_bil:.3f}, "
          f"mean support {S.mean():.3f}")
    assert e_sr <= 0.6 * e_bil


def test_the_neighbour_weight_rejects_a_block_of_wrong_flows():
    """The same scene with the flows of a 20 x 20 block wrong by 3 px in every
    neighbour, sigma 5.  Measured MSE over the block's high-resolution pixels:
    64.41 with the neighbour weight, 797.87 with every weight forced to 1."""
    truth, center, neigh, flows = sn.scene(2)
    blk = (slice(14, 34), slice(22, 42))
    bad = []
    for k, f in enumerate(flows):
        f = f.copy()
        f[blk] += ((3.0, 0.0), (0.0, 3.0), (-3.0, 0.0), (0.0, -3.0))[k]
        bad.append(f)
    hb = (slice(28, 68), slice(44, 84))
    mse = lambda o: float(((o.astype(np.float64) - truth) ** 2)[hb].mean())  # noqa: E731
    with_w = mse(sn.super_resolve(center, neigh, bad, 2, 5.0)[0])
    ones = [np.ones((48, 64), np.float32)] * 4
    without = mse(sn.super_resolve(center, neigh, bad, 2, 5.0, weights=ones)[0])
    print(f"wrong-flow block: MSE {with_w:.2f} with the neighbour weight, {without:.2f} with every weight 1")
    assert with_w < 0.25 * without
