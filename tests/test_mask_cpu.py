"""CPU tests of the mask propagation (include/optflow.h, "Mask propagation"):
the arithmetic itself, on the numpy float64 restatement (tests/mask_numpy.py),
the scene of the quality tests along its layered flows, the Python validators,
the keyframe assignment of propagate_masks and the C ABI mirror.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import mask_numpy as mk


# ---- the interface exists ---------------------------------------------------
def test_package_exports_the_new_functions():
    import optical_flow
    for name in ("advance_mask", "MaskPropagator", "propagate_masks"):
        assert name in optical_flow.__all__ and callable(getattr(optical_flow, name))
    assert (optical_flow.MASK_CARRIED, optical_flow.MASK_VOTED, optical_flow.MASK_UNKNOWN,
            optical_flow.MASK_GIVEN) == (0, 1, 2, 3)
    p = inspect.signature(optical_flow.advance_mask).parameters
    assert list(p) == ["mask", "frame", "flow", "state", "vote_radius", "vote_range", "smooth", "return_status"]
    assert [p[k].default for k in list(p)[3:]] == [None, 8, 20.0, 1, False]
    p = inspect.signature(optical_flow.MaskPropagator.__init__).parameters
    assert list(p) == ["self", "H", "W", "channels", "method", "params", "vote_radius", "vote_range", "smooth",
                       "alpha1", "alpha2", "context"]
    assert [p[k].default for k in list(p)[3:]] == [3, "classic+nl-fast", None, 8, 20.0, 1, 0.01, 0.5, None]
    p = inspect.signature(optical_flow.MaskPropagator.push).parameters
    assert list(p) == ["self", "frame", "mask"] and p["mask"].default is None
    p = inspect.signature(optical_flow.propagate_masks).parameters
    assert list(p)[:2] == ["frames", "keyframes"] and p["return_status"].default is False and "scale" not in p


def test_c_abi_mirror_declares_the_four_entries():
    from optical_flow import _abi, _native
    for name, nargs in {"of_mask_advance": 11, "of_masks_open": 6, "of_masks_push": 5, "of_masks_close": 1}.items():
        assert name in _native.EXPORTED_SYMBOLS
        assert len(_native._SIGS[name][0]) == nargs
    assert _abi.OF_ABI_VERSION == 3


FIELDS = ["vote_radius", "smooth", "range", "alpha1", "alpha2"]


def test_header_constants_and_struct_match_the_mirror(tmp_path):
    from conftest import ROOT
    from optical_flow import _abi
    offs = ", ".join(f"offsetof(of_mask_opts, {f})" for f in FIELDS)
    src = ('#include "optflow.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%d %d %d %d %d %d %zu'
           + " %zu" * len(FIELDS) + '\\n", OF_MASK_CARRIED, OF_MASK_VOTED, OF_MASK_UNKNOWN, OF_MASK_GIVEN, '
           "OF_MASK_MAX_VOTE_RADIUS, OF_MASK_MAX_SMOOTH, sizeof(of_mask_opts), " + offs + ");}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[:6] == [_abi.OF_MASK_CARRIED, _abi.OF_MASK_VOTED, _abi.OF_MASK_UNKNOWN, _abi.OF_MASK_GIVEN,
                       _abi.MASK_MAX_VOTE_RADIUS, _abi.MASK_MAX_SMOOTH]
    assert out[:6] == [0, 1, 2, 3, 12, 2]
    assert out[6:] == [ctypes.sizeof(_abi.OfMaskOpts)] + [getattr(_abi.OfMaskOpts, f).offset for f in FIELDS]
    assert out[6] == 32 and [n for n, _ in _abi.OfMaskOpts._fields_] == FIELDS


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
MK = np.zeros((8, 9), np.uint8)
FL = np.zeros((8, 9, 2))
NAN_IM = np.full((8, 9), np.nan)
BAD_MASKS = [np.zeros((8, 9)), np.zeros((8, 9), np.float32), np.zeros((8,), np.uint8), np.zeros((8, 9, 1), np.uint8),
             np.zeros((0, 9), np.uint8), np.zeros((9, 8), np.uint8), "mask"]
BAD_OPTS = [dict(vote_radius=v) for v in (0, 13, -1, 2.0, "2", None, True, float("nan"))] + \
    [dict(smooth=v) for v in (-1, 3, 1.0, "1", None, True)] + \
    [dict(vote_range=v) for v in (0, -1.0, float("nan"), float("inf"), "20", None, True)]
BAD_ALPHAS = [dict(alpha1=v) for v in (-0.1, float("nan"), None, "0")] + \
    [dict(alpha2=v) for v in (-1, float("inf"), None, True)]


@pytest.mark.parametrize("kw", BAD_OPTS + [dict(mask=m) for m in BAD_MASKS[:5] + BAD_MASKS[6:]] + [
    dict(mask=None), dict(frame=np.zeros((9, 8))), dict(frame=np.zeros((8, 9, 5))), dict(frame=np.zeros((8, 9, 0))),
    dict(frame=np.zeros((8,))), dict(frame=IM.astype(str)), dict(frame=np.zeros((8, 9, 1, 1))),
    dict(flow=np.zeros((8, 9, 3))), dict(flow=np.zeros((9, 8, 2))), dict(flow=np.zeros((8, 9))), dict(flow=None),
    dict(state=np.zeros((9, 8), np.uint8)), dict(state=np.zeros((8, 9))), dict(state=np.full((8, 9), 256)),
    dict(state=np.full((8, 9), -1))])
def test_advance_mask_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(mask=MK, frame=IM, flow=FL)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.advance_mask(**a)


@pytest.mark.parametrize("kw", BAD_OPTS + BAD_ALPHAS)
def test_session_bad_options_raise_before_any_library_call(no_library, kw):
    import optical_flow
    with pytest.raises(ValueError):
        optical_flow.MaskPropagator(8, 9, 1, **kw)
    with pytest.raises(ValueError):
        optical_flow.propagate_masks([IM, IM], MK, **kw)


def test_session_shapes_raise_before_any_library_call(no_library):
    import optical_flow
    for H, W, ch in ((0, 9, 1), (8, -1, 1), (8.0, 9, 1), (8, 9, 2), (8, 9, 4), (8, 9, True), (46341, 46341, 1)):
        with pytest.raises(ValueError):
            optical_flow.MaskPropagator(H, W, ch)


@pytest.mark.parametrize("kw", [dict(keyframes=m) for m in BAD_MASKS] + [
    dict(keyframes={}), dict(keyframes={2: MK}), dict(keyframes={-1: MK}), dict(keyframes={0.0: MK}),
    dict(keyframes={True: MK}), dict(keyframes={"0": MK}), dict(keyframes={0: MK, 1: np.zeros((8, 9))}),
    dict(keyframes=None), dict(frames=[]), dict(frames=[IM, np.zeros((8, 8))]), dict(frames=[IM, NAN_IM]),
    dict(frames=[np.zeros((8, 9, 2))] * 2), dict(frames=[np.zeros((8, 9, 4))] * 2), dict(frames=[np.zeros(8)] * 2),
    dict(frames=[IM.astype(str)] * 2), dict(frames=[np.zeros((0, 9))] * 2)])
def test_propagate_masks_bad_arguments_raise_before_any_library_call(no_library, kw):
    import optical_flow
    a = dict(frames=[IM, IM], keyframes=MK)
    a.update(kw)
    with pytest.raises(ValueError):
        optical_flow.propagate_masks(**a)


# ---- the keyframe assignment of propagate_masks ----------------------------
class StubSession:
    """Stands in for MaskPropagator: a keyframe's mask (0 / 1 by then) comes
    back as it is, a later push returns the previous mask plus 1 (so a mask
    tells how many steps it is from its keyframe) and the log keeps the order
    of the pushes."""
    log = []

    def __init__(self, H, W, channels, *args, **kw):
        StubSession.log.append(("open", H, W, channels))
        self.m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        StubSession.log.append(("close",))

    def push(self, frame, mask=None):
        self.m = mask.copy() if mask is not None else self.m + 1
        self.last_status = np.full(self.m.shape, 3 if mask is not None else 0, np.uint8)
        StubSession.log.append(("push", int(frame.flat[0]), mask is not None))
        return self.m


@pytest.fixture
def stub(monkeypatch):
    from optical_flow import masks
    StubSession.log = []
    monkeypatch.setattr(masks, "MaskPropagator", StubSession)
    return StubSession


def _clip(T):
    return [np.full((4, 5), float(t)) for t in range(T)]


def test_single_mask_means_keyframe_0_propagated_forward(stub):
    import optical_flow
    out, st = optical_flow.propagate_masks(_clip(4), np.full((4, 5), 10, np.uint8), return_status=True)
    assert out.shape == (4, 4, 5) and out.dtype == np.uint8 and st.shape == (4, 4, 5) and st.dtype == np.uint8
    assert [int(o[0, 0]) for o in out] == [1, 2, 3, 4]
    assert [int(s[0, 0]) for s in st] == [3, 0, 0, 0]
    assert stub.log == [("open", 4, 5, 1), ("push", 0, True), ("push", 1, False), ("push", 2, False),
                        ("push", 3, False), ("close",)]
    only = optical_flow.propagate_masks(_clip(4), np.full((4, 5), 10, np.uint8))
    assert isinstance(only, np.ndarray) and np.array_equal(only, out)


def test_nearest_keyframe_ties_to_the_earlier_and_backward_runs(stub):
    import optical_flow
    keys = {2: np.full((4, 5), 20, np.uint8), 6: np.full((4, 5), 60, np.uint8)}
    out = optical_flow.propagate_masks(_clip(9), keys)
    # frames 0, 1 backward from 2; 3, 4 forward from 2 (4 is the tie); 5 backward from 6; 7, 8 forward from 6
    assert [int(o[0, 0]) for o in out] == [3, 2, 1, 2, 3, 2, 1, 2, 3]
    runs = []
    for e in stub.log:
        if e[0] == "open":
            runs.append([])
        elif e[0] == "push":
            runs[-1].append(e[1:])
    assert runs == [[(2, True), (3, False), (4, False)], [(2, True), (1, False), (0, False)],
                    [(6, True), (7, False), (8, False)], [(6, True), (5, False)]]
    assert [e[0] for e in stub.log].count("close") == 4  # sequential, one session each
    opens = [k for k, e in enumerate(stub.log) if e[0] == "open"]
    closes = [k for k, e in enumerate(stub.log) if e[0] == "close"]
    assert all(c < o for c, o in zip(closes, opens[1:]))


def test_keyframe_runs_cover_every_frame_once():
    from optical_flow.masks import _keyframe_runs
    assert _keyframe_runs(1, [0]) == [[0]]
    assert _keyframe_runs(3, [2]) == [[2, 1, 0]]
    assert _keyframe_runs(3, [0, 1, 2]) == [[0], [1], [2]]
    assert _keyframe_runs(6, [0, 5]) == [[0, 1, 2], [5, 4, 3]]
    rng = np.random.default_rng(1)
    for _ in range(50):
        T = int(rng.integers(1, 20))
        keys = sorted(set(int(k) for k in rng.integers(0, T, int(rng.integers(1, 5)))))
        seen = {}
        for run in _keyframe_runs(T, keys):
            assert run[0] in keys and all(abs(b - a) == 1 for a, b in zip(run, run[1:]))
            for t in run[1:]:
                assert t not in seen and t not in keys
                seen[t] = run[0]
        assert sorted(seen) == [t for t in range(T) if t not in keys]
        for t, k in seen.items():
            d = min(abs(t - q) for q in keys)
            assert abs(t - k) == d and k == min(q for q in keys if abs(t - q) == d)


def test_colour_frames_open_a_three_channel_session(stub):
    import optical_flow
    optical_flow.propagate_masks([np.zeros((4, 5, 3))] * 2, {1: np.ones((4, 5), np.uint8)})
    assert stub.log[0] == ("open", 4, 5, 3) and [e[1] for e in stub.log if e[0] == "push"] == [0, 0]


# ---- properties of the restatement ------------------------------------------
def _random_case(H, W, C, seed):
    rng = np.random.default_rng(seed)
    M = (rng.uniform(size=(H, W)) < 0.4).astype(np.uint8) * 9
    G = rng.uniform(0, 255, (H, W, C)).astype(np.float32)
    return rng, M, G


def test_zero_flow_with_all_states_0_keeps_the_mask():
    rng, M, G = _random_case(13, 17, 3, 1)
    z = np.zeros((13, 17, 2), np.float32)
    for S in (None, np.zeros((13, 17), np.uint8)):
        out, st = mk.advance(M, G, z, S, smooth=0)
        assert out.dtype == np.uint8 and np.array_equal(out, (M != 0).astype(np.uint8)) and (st == mk.CARRIED).all()


def test_integer_translation_shifts_the_mask_exactly():
    rng, M, G = _random_case(13, 17, 1, 2)
    f = np.zeros((13, 17, 2), np.float32)
    f[..., 0], f[..., 1] = -3.0, 2.0   # the current pixel (i, j) was at (i + 2, j - 3)
    out, st = mk.advance(M, G, f, None, vote_radius=1, smooth=0)
    want = np.zeros((13, 17), np.uint8)
    want[:-2, 3:] = (M != 0)[2:, :-3]
    dec = st == mk.CARRIED
    assert np.array_equal(dec[:-2, 3:], np.ones((11, 14), bool)) and not dec[-2:].any() and not dec[:, :3].any()
    assert np.array_equal(out[dec], want[dec])


def test_all_undecided_is_all_unknown_and_unmarked():
    rng, M, G = _random_case(9, 11, 3, 3)
    f = rng.uniform(-2, 2, (9, 11, 2)).astype(np.float32)
    for flow, S in ((f, np.ones((9, 11), np.uint8)), (np.full((9, 11, 2), np.nan, np.float32), None),
                    (np.full((9, 11, 2), 1e30, np.float32), None)):
        for smooth in (0, 1, 2):
            out, st = mk.advance(M, G, flow, S, smooth=smooth)
            assert not out.any() and (st == mk.UNKNOWN).all()


def test_vote_follows_the_colour_then_the_count():
    H, W = 9, 12
    G = np.full((H, W), 50.0, np.float32)
    G[:, 6:] = 200.0
    M = np.zeros((H, W), np.uint8)
    M[:, 6:] = 1                           # the bright half is the object
    S = np.zeros((H, W), np.uint8)
    S[3:6, 4:8] = 1                        # a patch across the edge is not trusted
    z = np.zeros((H, W, 2), np.float32)
    seen = set()
    out, st = mk.advance(M, G, z, S, vote_radius=3, vote_range=20.0, smooth=0, seen=seen)
    assert np.array_equal(out, M) and (st[3:6, 4:8] == mk.VOTED).all() and "voted-colour" in seen
    # a colour no neighbour comes near: the plain majority of the window decides
    G2 = G.copy()
    G2[4, 5] = 1000.0
    seen = set()
    out, st = mk.advance(M, G2, z, S, vote_radius=3, vote_range=20.0, smooth=0, seen=seen)
    assert "voted-count" in seen and st[4, 5] == mk.VOTED
    ok = (S == 0)[1:8, 2:9]
    assert out[4, 5] == (2 * int(M[1:8, 2:9][ok].sum()) >= int(ok.sum()))
    # a guide that is not finite weighs nothing
    G3 = G.copy()
    G3[4, 5] = np.nan
    o3, s3 = mk.advance(M, G3, z, S, vote_radius=3, vote_range=20.0, smooth=0)
    assert np.array_equal(o3, out) and np.array_equal(s3, st)


def test_smooth_1_clears_the_four_corners_of_a_rectangle_and_ties_keep_the_label():
    r = np.zeros((48, 64), np.uint8)
    r[10:28, 10:24] = 1                    # 14 wide, 18 tall
    out = mk.mode(r, 1)
    assert sorted(zip(*np.nonzero(out != r))) == [(10, 10), (10, 23), (27, 10), (27, 23)]
    # a 2 x 3 corner window (6 pixels) with 3 ones is a tie
    t = np.zeros((4, 6), np.uint8)
    t[0, 0] = t[1, 0] = t[1, 1] = 1
    seen = set()
    assert mk.mode(t, 1, seen)[0, 0] == 1 and "smooth-tie" in seen
    assert np.array_equal(mk.mode(t, 0), t)


def test_session_by_hand_order():
    frames = [np.full((3, 4), float(k), np.float32) for k in range(4)]
    m0, m2 = np.full((3, 4), 5, np.uint8), np.zeros((3, 4), np.uint8)
    pairs = []

    def pair(a, b):
        pairs.append((int(a[0, 0]), int(b[0, 0])))
        return np.zeros((3, 4, 2), np.float32), None

    res = mk.session(frames, [m0, None, m2, None], pair, lambda m, f, bw, sb: mk.advance(m, f, bw, sb))
    assert pairs == [(0, 1), (2, 3)]       # a keyframe estimates nothing
    assert [int(s[0, 0]) for _, s in res] == [mk.GIVEN, mk.CARRIED, mk.GIVEN, mk.CARRIED]
    assert res[0][0].all() and res[0][0].max() == 1 and res[1][0].all() and not res[2][0].any() and not res[3][0].any()


# ---- the scene, along the layered flows -------------------------------------
# per-frame IoU of frames 1 .. 8 against the true masks, pinned from the restatement
IOU_DEFAULTS = [0.9841, 0.9841, 0.9841, 0.9841, 0.9612, 0.9841, 0.9841, 0.9841]   # mean 0.981
IOU_SMOOTH_0 = [1.0, 1.0, 1.0, 1.0, 0.9767, 0.9805, 0.9805, 0.9882]               # mean 0.991
IOU_PLAIN = [0.9688, 0.9538, 0.9841, 0.9502, 0.8322, 0.7381, 0.6813, 0.62]        # mean 0.841, not recoloured
IOU_HELD_STILL = [0.647, 0.370, 0.203, 0.068, 0.0, 0.0, 0.0, 0.0]                  # mean 0.161
MEAN_LAYERED, MEAN_HELD_STILL = 0.981, 0.161


def _follow(scene, **kw):
    frames, masks, bw, states, _ = scene
    m, ious, sts = masks[0], [], []
    for s in range(1, len(frames)):
        m, st = mk.advance(m, frames[s], bw[s], states[s], **kw)
        ious.append(mk.iou(m, masks[s]))
        sts.append(st)
    return ious, sts


def test_scene_along_the_layered_flows():
    """inpaint_numpy.scene(0) recoloured (object around 200, background around
    90), the mask of frame 0 followed through frames 1 .. 8 along the layered
    flows with their states.  The figures are what this restatement gives and
    are pinned: mean IoU 0.981 at the defaults (every frame but one loses only
    the 4 corner pixels to smooth = 1), 0.991 at smooth 0, 0.841 on the scene
    as it is (no colour contrast to vote by), against 0.161 for the mask held
    still."""
    scene = mk.scene(0)
    frames, masks = scene[0], scene[1]
    held = [mk.iou(masks[0], masks[s]) for s in range(1, 9)]
    assert np.allclose(held, IOU_HELD_STILL, atol=5e-4) and abs(np.mean(held) - MEAN_HELD_STILL) < 5e-4
    ious, sts = _follow(scene)
    print("defaults:", [round(v, 4) for v in ious], round(float(np.mean(ious)), 4))
    assert np.allclose(ious, IOU_DEFAULTS, atol=5e-5) and abs(np.mean(ious) - MEAN_LAYERED) < 5e-4
    for st in sts:
        assert (st == mk.VOTED).any() and not (st == mk.UNKNOWN).any()
    ious0, _ = _follow(scene, smooth=0)
    print("smooth 0:", [round(v, 4) for v in ious0], round(float(np.mean(ious0)), 4))
    assert np.allclose(ious0, IOU_SMOOTH_0, atol=5e-5) and abs(np.mean(ious0) - 0.991) < 5e-4
    plain, _ = _follow(mk.scene(0, recoloured=False))
    print("not recoloured:", [round(v, 4) for v in plain], round(float(np.mean(plain)), 4))
    assert np.allclose(plain, IOU_PLAIN, atol=5e-5) and abs(np.mean(plain) - 0.841) < 5e-4


def test_scene_recolouring_and_states():
    frames, masks, bw, states, truth = mk.scene(0)
    plain = mk.scene(0, recoloured=False)
    for s in range(9):
        obj = masks[s] != 0
        assert frames[s].dtype == np.float32 and frames[s][obj].min() > 150 and frames[s][~obj].max() < 150
        assert np.array_equal(frames[s][~obj], truth[s][~obj])
        assert np.array_equal(plain[0][s], mk.ip.scene(0)[0][s])
    assert bw[0] is None and states[0] is None
    for s in range(1, 9):
        obj = masks[s] != 0
        step = np.unique(bw[s][obj].reshape(-1, 2), axis=0)
        assert step.shape == (1, 2) and np.array_equal(step[0], np.round(step[0])) and -4 <= step[0, 0] <= -3
        assert np.allclose(bw[s][~obj], np.float32([1.3, -0.7]))
        assert not states[s][obj].any() and set(np.unique(states[s])) == {0, 1, 2}
