"""CPU tests of the per-pixel data-term weight's surface (no GPU): the four
C entries exist and are bound, the keyword is where the issue puts it, and a
bad weight is refused before the library is touched."""
import ctypes
import inspect
import os

import numpy as np
import pytest

WEIGHTED = {"of_estimate_flow_weighted": "of_estimate_flow", "of_compute_flow_weighted": "of_compute_flow",
            "of_compute_flow_base_weighted": "of_compute_flow_base", "of_flow_operator_weighted": "of_flow_operator"}


def test_library_exports_and_native_binds_the_four_entries():
    from optical_flow import _native
    assert os.path.exists(_native.LIB_PATH), "build() first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, sibling in WEIGHTED.items():
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS
        args, res = _native._SIGS[name]
        sargs, sres = _native._SIGS[sibling]
        # the sibling's signature plus one const float *
        assert res is sres and len(args) == len(sargs) + 1
        extra = list(args)
        for a in sargs:
            extra.remove(a)
        assert extra == [_native._fp]
    assert lib.of_abi_version() == 3


def test_keyword_is_keyword_only_on_the_method_classes_and_not_an_attribute():
    import optical_flow
    from optical_flow.methods.base import BaseOpticalFlow
    from optical_flow.methods.config import load_of_method
    assert inspect.signature(optical_flow.estimate_flow).parameters["data_weight"].default is None
    for fn in (BaseOpticalFlow.compute_flow, BaseOpticalFlow.compute_flow_base):
        p = inspect.signature(fn).parameters["data_weight"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert inspect.signature(BaseOpticalFlow._operator_planes).parameters["data_weight"].default is None
    assert not hasattr(load_of_method("classic+nl-fast"), "data_weight")


@pytest.fixture
def no_library(monkeypatch):
    from optical_flow import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_native, "load_library", boom)
    monkeypatch.setattr(_native, "context", boom)
    monkeypatch.setattr(_native, "Context", boom)


def _bad(kind, H, W):
    w = np.ones((H, W))
    if kind == "shape":
        return np.ones((H, W + 1))
    if kind == "shape3":
        return np.ones((H, W, 1))
    w[H // 2, W // 3] = {"nan": np.nan, "inf": np.inf, "negative": -1e-3, "f32_overflow": 1e39}[kind]
    return w


@pytest.mark.parametrize("kind", ["shape", "shape3", "nan", "inf", "negative", "f32_overflow"])
@pytest.mark.parametrize("shape", [(8, 9, 3), (8, 9), (8, 9, 2)])
def test_estimate_flow_refuses_a_bad_weight_without_a_gpu(no_library, kind, shape):
    import optical_flow
    im = np.zeros(shape)
    with pytest.raises(ValueError):
        optical_flow.estimate_flow(im, im, "hs", data_weight=_bad(kind, 8, 9))


@pytest.mark.parametrize("kind", ["shape", "nan", "negative"])
def test_method_classes_refuse_a_bad_weight_without_a_gpu(no_library, kind):
    from optical_flow.methods.config import load_of_method
    o = load_of_method("ba")
    o.images = np.zeros((8, 9, 2))
    z = np.zeros((8, 9, 2))
    with pytest.raises(ValueError):
        o.compute_flow(z, data_weight=_bad(kind, 8, 9))
    with pytest.raises(ValueError):
        o.compute_flow_base(z, data_weight=_bad(kind, 8, 9))
    with pytest.raises(ValueError):
        o._operator_planes(z, None, z[..., 0], z[..., 0], z[..., 0], 0.0, data_weight=_bad(kind, 8, 9))


def test_weight_conversion():
    from optical_flow import _native
    assert _native.data_weight(None, 3, 4) is None
    m = np.zeros((3, 4), dtype=bool)
    m[1, 2] = True
    w = _native.data_weight(m, 3, 4)
    assert w.dtype == np.float32 and w.flags.c_contiguous and w[1, 2] == 1.0 and w.sum() == 1.0
    w = _native.data_weight(np.full((4, 3), 2.5).T, 3, 4)  # values above 1 and a transposed view are fine
    assert w.flags.c_contiguous and np.all(w == 2.5)
