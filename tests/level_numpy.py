"""One pyramid level's warping loop in Python, written once over a backend of
stages: compute_flow_base of HS (hs.py:109-142), BA (ba.py:143-206) and
Classic+NL (classic_nl.py:200-277) of the reference, transcribed.

level_loop owns the control flow and the elementwise glue; a backend supplies
the stages and the scalar type.  With OracleBackend (float64, oracle/) the
loop must reproduce the oracle's own level (oracle.compute_flow_base) to
1e-12 -- that pins the transcription; with GpuBackend (float32, the stage
entries of include/optflow.h) it must equal of_compute_flow_base bit for bit
-- that pins the level's glue and buffer handling (host_flow.hip).  The glue
runs in the backend's scalar type, one numpy operation per kernel operation,
so in float32 each is one rounding as in k_add_update, k_sub2, k_axpy_diff and
the weighted median's base store (sums and differences only: there is no
product a compiler could contract into an fma).

  glue                       kernel
  uv + clip(x)               k_add_update (HS); k_update_occ is the backend's update
  res - uv                   k_sub2
  uv + (res - uv)            k_axpy_diff, k_wmf's base store
  ||x|| < 1e-3               norm2() + the host's comparison (fp64 sum of fp32 squares)
"""
import ctypes as C

import numpy as np


def level_loop(B, ope, images, guide, uv0, weight=None, trace=None):
    """compute_flow_base(uv0) of `ope` on `images` ((H, W, 2 nc)) with the
    stages of backend B.  guide: (H, W, gc) or None (Classic+NL then takes the
    plain median, weighted_median.py:42-47).  weight: (H, W) or None.
    trace: a list that receives (iteration, linearisation, x, ||x||) of every
    solve, x before the clip."""
    T = B.dtype
    uv = np.asarray(uv0, dtype=T)
    meth = ope._METHOD
    mfsz = ope._mf_size(ope.median_filter_size)
    clip = bool(ope.limit_update)

    def note(it, jl, x):
        xn = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
        if trace is not None:
            trace.append((it, jl, x.copy(), xn))
        return xn

    if meth == 'hs':
        for it in range(int(ope.max_warping_iters)):
            D = B.partial_deriv(ope, images, uv, 0.5, True)
            coef, rhs = B.operator(ope, 0.0, uv, None, D, weight)
            x = B.solve(ope, coef, rhs)
            if note(it, 0, x) < 1e-3:
                break
            uv = uv + (np.clip(x, T(-1), T(1)) if clip else x)
            if mfsz:
                for _ in range(int(ope.mf_iter)):
                    uv = B.median(uv, mfsz)
        return uv

    assert meth in ('ba', 'classic_nl'), meth
    alpha = float(ope.alpha)
    blend = float(ope.blend) if meth == 'ba' else 0.5  # classic_nl.py:232 passes no blend
    wmf = meth == 'classic_nl' and mfsz and guide is not None
    n_lin = int(ope.max_linear)
    for it in range(int(ope.max_iters)):
        duv = None  # zeros in the reference
        # one linearisation per warp: the level fuses warp and assembly
        D = B.partial_deriv(ope, images, uv, blend, n_lin == 1)
        for jl in range(n_lin):
            coef, rhs = B.operator(ope, alpha, uv, duv, D, weight)
            x = B.solve(ope, coef, rhs)
            note(it, jl, x)
            if wmf:
                uv1, occ = B.update(uv, x, clip, images)
                res = B.wmf(ope, uv1, guide, occ)
            else:
                uv1, _ = B.update(uv, x, clip, None)
                res = B.median(uv1, mfsz) if mfsz else uv1
            duv = res - uv
        uv = uv + duv
    return uv


class OracleBackend:
    """The float64 stages of oracle/optflow_oracle.c."""
    dtype = np.float64

    def __init__(self):
        import oracle
        self.O = oracle

    def partial_deriv(self, ope, images, uv, blend, may_fuse):
        return self.O.partial_deriv(images, uv, ope.interpolation_method, ope.deriv_filter, blend)

    def operator(self, ope, alpha, uv, duv, D, weight):
        assert weight is None, "the oracle has no data weight"
        return self.O.flow_operator(ope.to_params(), alpha, uv, duv, *D)

    def solve(self, ope, coef, rhs):
        return self.O.unplanar(self.O.solve(ope.to_params(), coef, rhs)[0], False)

    def update(self, uv, x, clip, images):
        uv1 = uv + (np.clip(x, -1.0, 1.0) if clip else x)
        return uv1, (None if images is None else self.O.detect_occlusion(uv1, images))

    def median(self, uv, size):
        return self.O.median_filter(uv, size)

    def wmf(self, ope, uv1, guide, occ):
        return self.O.weighted_median(uv1, guide, occ, int(ope.area_hsz), float(ope.sigma_i))


class GpuBackend:
    """The library's stage entries; every array float32.  fused: the value of
    OF_OPT_FUSED_WARP the level under test runs with."""
    dtype = np.float32

    def __init__(self, fused):
        self.fused = bool(fused)

    @staticmethod
    def _f(a):
        return np.asarray(a).astype(np.float32)

    def partial_deriv(self, ope, images, uv, blend, may_fuse):
        from optical_flow.utils.derivatives import partial_deriv
        nc = images.shape[2] // 2
        if self.fused and may_fuse and nc in (1, 3):  # can_fuse_warp_op
            return ("fused", blend)
        return partial_deriv(images, uv, ope.interpolation_method, ope.deriv_filter, blend)

    def operator(self, ope, alpha, uv, duv, D, weight):
        if isinstance(D[0], str):  # "fused": ope.images are the level's
            assert duv is None
            return ope._warp_operator_planes(uv, alpha, D[1], weight)
        return ope._operator_planes(uv, duv, D[0], D[1], D[2], alpha, data_weight=weight)

    def solve(self, ope, coef, rhs):
        from optical_flow import _native as nat
        _, H, W = coef.shape
        P = ope.to_params()
        x = np.empty((2, H, W), dtype=np.float32)
        ctx = nat.context()
        ctx.check(ctx.lib.of_solve(ctx.handle, C.byref(P), nat.ptr(nat.f32(coef)), nat.ptr(nat.f32(rhs)), H, W,
                                   nat.ptr(x), None, None))
        return np.moveaxis(x, 0, 2).copy()

    def update(self, uv, x, clip, images):
        from optical_flow.utils.occlusion import flow_update
        if images is None:
            return self._f(flow_update(uv, x, clip)), None
        uv1, occ = flow_update(uv, x, clip, images)
        return self._f(uv1), self._f(occ)

    def median(self, uv, size):
        from optical_flow.utils.weighted_median import median_filter_flow
        return self._f(median_filter_flow(uv, size))

    def wmf(self, ope, uv1, guide, occ):
        from optical_flow.utils.weighted_median import denoise_color_weighted_medfilt2
        return self._f(denoise_color_weighted_medfilt2(uv1, guide, occ, int(ope.area_hsz), ope.median_filter_size,
                                                       float(ope.sigma_i)))


# ---- numpy model of of_flow_update (k_update_occ) ----------------------------
def _bilinear_clamped(a, r, q):
    H, W = a.shape
    i0 = np.floor(r).astype(int)
    j0 = np.floor(q).astype(int)
    fr, fc = r - i0, q - j0
    i1, j1 = np.minimum(i0 + 1, H - 1), np.minimum(j0 + 1, W - 1)
    return (1 - fr) * ((1 - fc) * a[i0, j0] + fc * a[i0, j1]) + fr * ((1 - fc) * a[i1, j0] + fc * a[i1, j1])


def flow_update_model(uv, x, clip, images, pitch, mutant=None):
    """(uv1, occ) as k_update_occ computes them, in float64 from the float32
    uv1: uv1 = uv + clip(x) stored in a plane of row pitch `pitch`, the left
    and upper neighbour's uv1 recomputed from uv and x at k - 1 and k - pitch.
    mutant: None, or a planted bug --
      'left_unclipped'  the left neighbour recomputed as uv + x
      'upper_at_W'      the upper neighbour read at k - W in the pitched plane
      'no_col0_guard'   d u / d x at column 0 taken against element k - 1
    Elements of the pitched plane that no pixel owns read as 0."""
    f = np.float32
    uv, x = np.asarray(uv).astype(f), np.asarray(x).astype(f)
    H, W = uv.shape[:2]
    xc = np.clip(x, f(-1), f(1)) if clip else x
    uv1 = (uv + xc).astype(np.float64)
    raw = (uv + x).astype(np.float64)

    def plane(a):  # flat pitched storage with one row of zeros in front
        p = np.zeros((H + 1, pitch))
        p[1:, :W] = a
        return p.reshape(-1)

    i, j = np.mgrid[0:H, 0:W]
    k = (i + 1) * pitch + j
    pu, pv = plane(uv1[..., 0]), plane(uv1[..., 1])
    left = plane(raw[..., 0])[k - 1] if mutant == 'left_unclipped' else pu[k - 1]
    up = pv[k - W] if mutant == 'upper_at_W' else pv[k - pitch]
    dudx = uv1[..., 0] - left
    if mutant != 'no_col0_guard':
        dudx = np.where(j > 0, dudx, 0.0)
    dvdy = np.where(i > 0, uv1[..., 1] - up, 0.0)
    div = dudx + dvdy
    odiv = np.exp(-div * div / (2 * 0.3 * 0.3))
    r = np.clip(i + uv1[..., 1], 0, H - 1)
    q = np.clip(j + uv1[..., 0], 0, W - 1)
    nc = images.shape[2] // 2
    it = sum(np.abs(_bilinear_clamped(images[..., nc + c], r, q) - images[..., c]) for c in range(nc))
    if nc > 1:
        it = it / nc
    return uv1, odiv * np.exp(-it * it / (2 * 20.0 * 20.0))
