"""Layered motion segmentation: what can be checked without a GPU -- the C
ABI mirror, the Python surface's argument checks, and the numpy restatement
(tests/layers_numpy.py): its quality on seeded scenes, the junk class and the
tie rules."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import layers_numpy as ln
import motion_numpy as mn
from conftest import ROOT
from test_motion_cpu import affine_flow, no_library  # noqa: F401  (a fixture)

MODELS = ("translation", "similarity", "affine")
SIGMA = 0.15   # px, the scenes' flow noise

# three true motions per model, more than the cutoff apart everywhere in the frame
TRUTH = {
    "translation": [(1.5, 0, 0, -0.7, 0, 0), (-3.0, 0, 0, 2.0, 0, 0), (4.0, 0, 0, 3.5, 0, 0)],
    "similarity": [(1.5, 0.8, -1.2, -0.7, 1.2, 0.8), (-3.0, -0.5, 0.6, 2.0, -0.6, -0.5),
                   (4.0, 0.3, 0.9, 3.5, -0.9, 0.3)],
    "affine": [(1.5, 0.25, -0.75, -0.5, 1.0, 0.5), (-3.0, -0.6, 0.4, 2.0, 0.3, -0.8),
               (4.0, 0.5, 0.2, 3.5, -0.4, 0.6)],
}


def regions(kind, H=120, W=160):
    """The ground-truth layer of every pixel: "ellipse" a centred ellipse of
    60 % of the frame (layer 1) over layer 0; "three" a left band of 45 % and
    the rest split at 0.55 H; "one" a single layer."""
    ii, jj = np.mgrid[0:H, 0:W]
    if kind == "ellipse":   # area pi*a*b = 0.6*H*W with a/b = W/H
        k = np.sqrt(0.6 / np.pi)
        return ((((jj - 0.5 * (W - 1)) / (k * W)) ** 2 + ((ii - 0.5 * (H - 1)) / (k * H)) ** 2) < 1.0).astype(int)
    if kind == "three":
        return np.where(jj < 0.45 * W, 0, np.where(ii < 0.55 * H, 1, 2))
    return np.zeros((H, W), int)


def layered_scene(kind, model, H=120, W=160, seed=0):
    """(flow float32, truth labels, the true thetas): every region moves by
    its model flow plus Gaussian noise of SIGMA px."""
    gt = regions(kind, H, W)
    ths = TRUTH[model][:gt.max() + 1]
    f = np.zeros((H, W, 2))
    for l, th in enumerate(ths):
        f[gt == l] = affine_flow(H, W, th)[gt == l]
    f += np.random.default_rng(seed).normal(0.0, SIGMA, f.shape)
    return f.astype(np.float32), gt, ths


SCENES = [("ellipse", "similarity"), ("ellipse", "affine")] + [(k, m) for k in ("three", "one") for m in MODELS]


def check_gates(r, gt, ths, what):
    """The quality gates: n is the number of true layers; under the best
    permutation of the layers at least 0.99 of the labels agree with the truth
    and every theta is within 0.05 of its truth.  Returns (agreement, max |dth|)."""
    assert r.n == len(ths) == len(r.layers), (what, r.n)
    best = (-1.0, None)
    for perm in itertools.permutations(range(r.n)):   # layer l of the result is truth perm[l]
        agree = float(np.mean(np.array(perm + (-1,))[np.minimum(r.labels, r.n)] == gt))
        best = max(best, (agree, perm))
    agree, perm = best
    err = max(float(np.abs(np.asarray(r.layers[l].theta) - np.array(ths[perm[l]])).max()) for l in range(r.n))
    print(f"{what}: n {r.n}, agreement {agree:.4f}, max |dth| {err:.4f}, pixels {[la.pixels for la in r.layers]}")
    assert agree >= 0.99, (what, agree)
    assert err <= 0.05, (what, err)
    return agree, err


# ---- the ABI ---------------------------------------------------------------------
def test_package_exports_segment_motion():
    import optical_flow
    from optical_flow import motion
    for name in ("segment_motion", "MotionLayers", "MotionLayer", "LAYER_NONE"):
        assert getattr(optical_flow, name) is getattr(motion, name)
        assert name in optical_flow.__all__
    assert optical_flow.LAYER_NONE == 255 == ln.NONE
    assert optical_flow.MotionLayer._fields == ("theta", "matrix", "support", "rms", "pixels", "degenerate")
    assert optical_flow.MotionLayers._fields == ("labels", "layers", "n", "labels_raw")


def test_c_abi_mirror_declares_the_entry_and_its_two_structs(tmp_path):
    from optical_flow import _abi, _native
    text = open(os.path.join(ROOT, "include", "optflow.h")).read()
    decl = re.search(r"\bint of_segment_motion\(([^;]*)\);", text)
    assert decl and len(decl.group(1).split(",")) == 11
    sig = _native._SIGS["of_segment_motion"][0]
    assert len(sig) == 11
    assert sig[6:8] == [ctypes.POINTER(_abi.OfLayersOpts), ctypes.POINTER(_abi.OfMotionLayer)]
    offs = lambda S: [(f, getattr(S, f).offset) for f, _ in S._fields_]  # noqa: E731
    assert ctypes.sizeof(_abi.OfLayersOpts) == 40
    assert offs(_abi.OfLayersOpts) == [("model", 0), ("max_layers", 4), ("grid", 8), ("passes", 12), ("rounds", 16),
                                       ("smooth", 20), ("cutoff", 24), ("min_support", 32)]
    assert ctypes.sizeof(_abi.OfMotionLayer) == 128
    assert offs(_abi.OfMotionLayer) == [("theta", 0), ("matrix", 48), ("support", 96), ("rms", 104), ("pixels", 112),
                                        ("degenerate", 120), ("pad_", 124)]
    assert _abi.OF_ABI_VERSION == 3 and _abi.OF_LAYER_NONE == 255
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu '
           '%zu %d %d\\n", sizeof(of_layers_opts), sizeof(of_motion_layer), offsetof(of_layers_opts, cutoff), '
           'offsetof(of_layers_opts, min_support), offsetof(of_motion_layer, support), '
           'offsetof(of_motion_layer, pixels), offsetof(of_motion_layer, degenerate), OF_LAYER_NONE, '
           'OF_ABI_VERSION);}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [40, 128, 24, 32, 96, 112, 120, 255, 3]


NAN, INF = float("nan"), float("inf")
BAD_LAYER_OPTS = [
    dict(model="projective"), dict(model=2), dict(max_layers=0), dict(max_layers=9), dict(max_layers=2.0),
    dict(grid=0), dict(grid=17), dict(grid=True), dict(passes=-1), dict(passes=17), dict(rounds=-1), dict(rounds=17),
    dict(smooth=-1), dict(smooth=4), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=NAN), dict(cutoff=INF),
    dict(min_support=0.0), dict(min_support=-0.1), dict(min_support=1.5), dict(min_support=NAN)]


@pytest.mark.parametrize("kw", BAD_LAYER_OPTS + [
    dict(flow=np.zeros((8, 9))), dict(flow=np.zeros((0, 9, 2))), dict(weight=np.zeros((8, 10))),
    dict(weight=np.full((8, 9), -1.0)), dict(weight=np.full((8, 9), NAN)), dict(state=np.zeros((8, 10), np.uint8)),
    dict(state=np.full((8, 9), 256))])
def test_segment_motion_bad_arguments_raise_before_any_library_call(no_library, kw):  # noqa: F811
    import optical_flow
    a = dict(flow=np.zeros((8, 9, 2)))
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.segment_motion(**a)


# ---- quality ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,model", SCENES)
def test_the_restatement_meets_the_quality_gates(kind, model):
    """120 x 160, noise 0.15 px, default options.  Measured: agreement >= 0.9999
    and max |dth| <= 0.0140 on every scene (the figures are printed)."""
    f, gt, ths = layered_scene(kind, model)
    check_gates(ln.segment(f, model), gt, ths, (kind, model))


def test_a_block_of_junk_flow_comes_out_none():
    """A 10 % block of uniform +-6 px flow on the one-layer scene: at least
    0.98 of it is NONE (measured 0.9938 for every model) and the rest of the
    frame keeps its one layer."""
    for model in MODELS:
        f, gt, ths = layered_scene("one", model, seed=1)
        junk = np.zeros(gt.shape, bool)
        junk[30:78, 50:90] = True   # 48 x 40 = 10 % of 120 x 160
        f[junk] = np.random.default_rng(7).uniform(-6, 6, (int(junk.sum()), 2)).astype(np.float32)
        r = ln.segment(f, model)
        share = float(np.mean(r.labels[junk] == ln.NONE))
        print(f"{model}: n {r.n}, NONE on the junk {share:.4f}, layer 0 elsewhere {np.mean(r.labels[~junk] == 0):.4f}")
        assert r.n == 1 and share >= 0.98
        assert np.mean(r.labels[~junk] == 0) >= 0.99


# ---- the tie rules ---------------------------------------------------------------------
def test_equal_counts_give_the_lower_hypothesis():
    assert ln.pick({}) is None
    assert ln.pick({3: 7, 5: 7, 9: 2}) == 3
    assert ln.pick({3: 6, 5: 7, 9: 7}) == 5
    # two cells of equal size, each a pure motion: both hypotheses count 512, the first is extracted first
    f = np.zeros((8, 128, 2), np.float32)
    f[:, 64:] = (4.0, -3.0)
    r = ln.segment(f, "translation", grid=2, smooth=0, min_support=0.5)
    assert r.n == 2 and np.array_equal(r.layers[0].theta, np.zeros(6))
    assert np.array_equal(r.layers[1].theta, [4.0, 0, 0, -3.0, 0, 0])
    assert np.all(r.labels[:, :64] == 0) and np.all(r.labels[:, 64:] == 1)
    assert [la.pixels for la in r.layers] == [512, 512] and [la.support for la in r.layers] == [512.0, 512.0]


def test_equal_residuals_give_the_lower_layer():
    H, W = 4, 6
    _, _, _, x, y = mn.frame_coords(H, W)
    u, v = np.zeros((H, W)), np.zeros((H, W))
    fin = np.ones((H, W), bool)
    ths = [[0.5, 0, 0, 0, 0, 0], [-0.5, 0, 0, 0, 0, 0], [0, 0, 0, 0.5, 0, 0]]   # r2 = 0.25 against each
    assert np.all(ln.assign(ths, x, y, u, v, fin, 1.0) == 0)
    assert np.all(ln.assign(ths[::-1], x, y, u, v, fin, 1.0) == 0)
    assert np.all(ln.assign(ths, x, y, u, v, fin, 0.25) == ln.NONE)     # r2 < c2 is strict
    fin[1, 2] = False
    lab = ln.assign([[0.75, 0, 0, 0, 0, 0]] + ths, x, y, u, v, fin, 1.0)
    assert lab[1, 2] == ln.NONE and (lab == 1).sum() == H * W - 1


def test_a_mode_tie_gives_the_smaller_value():
    lab = np.array([[0, 1, ln.NONE, ln.NONE]], np.uint8)
    # windows of radius 1 in a single row: {0, 1}, {0, 1, 255}, {1, 255, 255}, {255, 255}
    assert list(ln.mode_filter(lab, 2, 1)[0]) == [0, 0, ln.NONE, ln.NONE]
    lab = np.array([[1, ln.NONE], [ln.NONE, 1]], np.uint8)   # every window holds two of each: NONE loses
    assert np.all(ln.mode_filter(lab, 2, 1) == 1)
    assert np.array_equal(ln.mode_filter(lab, 2, 0), lab)
    # the frame's edge shortens the window: the corner sees 4 pixels, not 9
    lab = np.zeros((5, 5), np.uint8)
    lab[:2, :2] = 1
    out = ln.mode_filter(lab, 2, 1)
    assert out[0, 0] == 1 and out[0, 1] == 1 and out[1, 1] == 0 and out[0, 2] == 0   # 4 of 4, 4 of 6, 4 of 9, 2 of 6
