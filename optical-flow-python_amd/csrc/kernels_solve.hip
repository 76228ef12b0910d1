// kernels_solve.hip — what the matrix-free solvers of the 2N x 2N flow system
// (base.py:87-172) share, and the diagnostics that belong to none of them.
// The solver families follow, one file each, and use only this file and the
// files before them: kernels_cg.hip (the fed CG: one launch per iteration),
// kernels_cgs.hip (its 'backslash' surrogate iteration k_cgs),
// kernels_cg_wg.hip (a whole CG solve in one workgroup), kernels_sor.hip
// (lexicographic SOR); kernels_gen.hip borrows precond, prologue_sum and
// write_partials.  Expects nothing before it but kernels.h.
// Held here: the per-block partials and their fixed-order sum, the 2x2 block /
// scalar Jacobi preconditioner of the general-operator CG, the fp64 residual
// of one pixel, the test whether x_lo is part of an iterate, and the norm and
// true-residual kernels.
// Shared invariant, the launch-boundary reduce: a global reduction is written
// as per-block partials (write_partials) and finished by every block of a
// later launch in the same fixed order (prologue_sum, cg_prologue), so all
// blocks derive bit-identical scalars and no agent-scope fence or atomic is
// needed (kernel boundaries give visibility).  A grid has at most
// PCG_MAX_BLOCKS blocks.
#include "kernels.h"

#define PCG_MAX_BLOCKS 512
static_assert(PCG_MAX_BLOCKS % 256 == 0,
              "the CG prologue sums PCG_MAX_BLOCKS / 256 partials per lane of a 256-thread block: a remainder would "
              "be left out");
// degree of the Chebyshev polynomial preconditioner of the 'backslash'
// surrogate (k_cgs, k_cg_small): 5 needs 0.70x the iterations of 3 on
// Classic+NL stage-2 systems (tools/poly_iters.py), and its two extra stencil
// stages run on the two waves of a k_cgs block that had idle time
#define CG_DEG 5

// (not to be merged with cg_inv, kernels_cg.hip, or cgw_inv, kernels_cg_wg.hip:
// this one divides and leaves the determinant to the compiler; they round otherwise)
template <bool BLOCK>
__device__ __forceinline__ float2 precond(float a, float c, float d, float2 r) {
  if (BLOCK) {
    const float det = a * d - c * c;
    if (det > 1e-30f * fabsf(a * d)) {
      const float inv = 1.0f / det;
      return make_float2((d * r.x - c * r.y) * inv, (a * r.y - c * r.x) * inv);
    }
  }
  // scalar Jacobi, base.py:129-131: 1/diag where |diag| > 1e-12 else 0
  return make_float2(fabsf(a) > 1e-12f ? r.x / a : 0.0f, fabsf(d) > 1e-12f ? r.y / d : 0.0f);
}

// fixed-order sum of NV partial arrays (stride nb) by the whole block;
// result broadcast to every thread
template <int NV>
__device__ __forceinline__ void prologue_sum(double (&out)[NV], const double *__restrict__ part, int nb, double *lds) {
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nt = blockDim.x * blockDim.y;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double s = 0.0;
    for (int b = tid; b < nb; b += nt) s += part[(size_t)v * PCG_MAX_BLOCKS + b];
    out[v] = wave_sum(s);
  }
  if ((tid & 63) == 0)
#pragma unroll
    for (int v = 0; v < NV; ++v) lds[v * 8 + (tid >> 6)] = out[v];
  __syncthreads();
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double s = 0.0;
    for (int w = 0; w < nt / 64; ++w) s += lds[v * 8 + w];
    out[v] = s;
  }
  __syncthreads();
}

// per-block partials -> part[v * PCG_MAX_BLOCKS + bid] (plain stores)
template <int NV>
__device__ __forceinline__ void write_partials(double (&v)[NV], double *part, double *lds, int slot = -1) {
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nt = blockDim.x * blockDim.y;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[k * 8 + (tid >> 6)] = v[k];
  __syncthreads();
  if (tid == 0) {
    const int bid = slot >= 0 ? slot : blockIdx.x + blockIdx.y * gridDim.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double s = 0.0;
      for (int w = 0; w < nt / 64; ++w) s += lds[k * 8 + w];
      part[(size_t)k * PCG_MAX_BLOCKS + bid] = s;
    }
  }
}

// b - A x at pixel (i, j) in fp64 from the fp32 operator; x + x_hi when xh
__device__ __forceinline__ double2 resid_px(const float *__restrict__ coef, size_t ps, const float2 *__restrict__ b,
                                           const float2 *__restrict__ x, const float2 *__restrict__ xh, int i, int j,
                                           int H, int W, int P) {
  const size_t k = (size_t)i * P + j;
  auto xv = [&](size_t e) {
    const float2 a = x ? x[e] : make_float2(0.f, 0.f);
    if (!xh) return make_double2(a.x, a.y);
    const float2 h = xh[e];
    return make_double2((double)a.x + (double)h.x, (double)a.y + (double)h.y);
  };
  const double2 xc = xv(k);
  const float2 bb = b[k];
  double su = (double)bb.x - ((double)coef[4 * ps + k] * xc.x + (double)coef[5 * ps + k] * xc.y);
  double sv = (double)bb.y - ((double)coef[5 * ps + k] * xc.x + (double)coef[6 * ps + k] * xc.y);
  if (j + 1 < W) {
    const double2 n = xv(k + 1);
    su += (double)coef[k] * n.x;
    sv += (double)coef[2 * ps + k] * n.y;
  }
  if (j > 0) {
    const double2 n = xv(k - 1);
    su += (double)coef[k - 1] * n.x;
    sv += (double)coef[2 * ps + k - 1] * n.y;
  }
  if (i + 1 < H) {
    const double2 n = xv(k + P);
    su += (double)coef[ps + k] * n.x;
    sv += (double)coef[3 * ps + k] * n.y;
  }
  if (i > 0) {
    const double2 n = xv(k - P);
    su += (double)coef[ps + k - P] * n.x;
    sv += (double)coef[3 * ps + k - P] * n.y;
  }
  return make_double2(su, sv);
}

// (k_cg_finalize and k_resid_part.)  After a residual replacement
// (k_cg_update, kernels_cg.hip) the iterate is x_hi + x_lo;
// x_lo is part of the iterate only if a CG launch after the replacement ran
// its sweep: a solve that the replacement itself finished (its residual
// already below atol, declared by launch upd_k, iter = upd_k - 1) never
// restarted x_lo, which then still holds x_hi's copy
__device__ __forceinline__ bool cg_xlo_live(const PcgState *st) { return st->iter >= st->upd_k; }

// ---------------------------------------------------------------------------
// sum of squares of a float2 field (HS early exit ||x||_2 < 1e-3, hs.py:127):
// partials then a one-block finish
__global__ __launch_bounds__(256) void k_norm2_part(const float2 *__restrict__ x, int H, int W, int P, double *part) {
  __shared__ double lds[32];
  double v[1] = {0.0};
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const float2 a = x[(size_t)i * P + j];
    v[0] += (double)a.x * a.x + (double)a.y * a.y;
  }
  write_partials<1>(v, part, lds);
}
// sum of squares of clip(x) - d (d may be null; clip to [-1, 1] when limit):
// the reference's display norm ||x - duv|| (classic_nl.py:255-256,
// ba.py:189-190, alt_ba.py:249-250), partials for k_norm2_final
__global__ __launch_bounds__(256) void k_step_norm2_part(const float2 *__restrict__ x, const float2 *__restrict__ d,
                                                         int limit, int H, int W, int P, double *part) {
  __shared__ double lds[32];
  double v[1] = {0.0};
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    float2 a = x[k];
    if (limit) a = make_float2(fminf(fmaxf(a.x, -1.f), 1.f), fminf(fmaxf(a.y, -1.f), 1.f));
    const double u = (double)a.x - (d ? (double)d[k].x : 0.0), w = (double)a.y - (d ? (double)d[k].y : 0.0);
    v[0] += u * u + w * w;
  }
  write_partials<1>(v, part, lds);
}
__global__ __launch_bounds__(256) void k_norm2_final(const double *part, int nb, double *result) {
  __shared__ double lds[32];
  double s[1];
  prologue_sum<1>(s, part, nb, lds);
  if (threadIdx.x == 0 && threadIdx.y == 0) *result = s[0];
}

// ---------------------------------------------------------------------------
// Diagnostic: the TRUE residual of a solve, ||b - A x||^2 and ||b||^2 in
// fp64 (A = D - N from the fp32 coefficient planes), independent of any
// solver recurrence.  Per-block partials, then a one-block finish into
// out[0..1].
// fp64 true residual of x (+ x_hi when st says a residual replacement ran)
__global__ __launch_bounds__(256) void k_resid_part(const float *__restrict__ coef, size_t ps,
                                                    const float2 *__restrict__ b, const float2 *__restrict__ x,
                                                    const float2 *__restrict__ xh, const PcgState *st, int H, int W,
                                                    int P, double *part) {
  __shared__ double lds[64];
  double v[2] = {0.0, 0.0};
  const float2 *xhi = xh && st && st->upd_k ? xh : nullptr;
  const float2 *xlo = xhi && !cg_xlo_live(st) ? nullptr : x;
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    const float2 bb = b[k];
    const double2 r = resid_px(coef, ps, b, xlo, xhi, i, j, H, W, P);
    v[0] += r.x * r.x + r.y * r.y;
    v[1] += (double)bb.x * bb.x + (double)bb.y * bb.y;
  }
  write_partials<2>(v, part, lds);
}
__global__ __launch_bounds__(256) void k_resid_final(const double *part, int nb, double *out) {
  __shared__ double lds[64];
  double s[2];
  prologue_sum<2>(s, part, nb, lds);
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    out[0] = s[0];
    out[1] = s[1];
  }
}
