// kernels_cg_wg.hip — a whole CG solve in ONE workgroup, for the coarse
// pyramid levels: k_cg_small (vectors in global memory, at most CG_SMALL_PX
// pixels) and k_cg_reg (vectors in registers, at most CG_REG_PX pixels), with
// their arguments (CgSmallArgs) and the cgw_ helpers.  Expects
// kernels_solve.hip before it (CG_DEG, resid_px); it shares no code with the
// fed CG of kernels_cg.hip / kernels_cgs.hip, only the PcgState it ends in
// and k_cg_finalize, which adds x_hi after a residual replacement.
// Shared by both kernels: one launch of one workgroup is the solve; scipy's
// control flow; the preconditioner is the template pair <DEG, BLOCK>; sweeps
// are separated by workgroup barriers and every dot product is a fixed-order
// fp64 sum over the workgroup (deterministic); thread 0 writes the final
// state.  CGW_ / cgw_ names belong to this file (CGR_ to k_cg_reg).
#include "kernels.h"

// ---------------------------------------------------------------------------
// k_cg_small: a whole CG solve in ONE workgroup, for levels of at most
// CG_SMALL_PX pixels.  At the coarse pyramid levels a fused k_cgs launch is
// latency-bound (~23 us however few rows: its 7-stage row pipeline is walked
// by one wave per band), and a solve is one launch per iteration; here the
// whole solve is one launch.  Textbook preconditioned CG with the control
// flow of scipy.sparse.linalg.cg (base.py:116-136): x0 = 0, stop when
// ||r|| < rtol ||b|| before an iteration, at most maxiter iterations.
// Preconditioner as in the fused kernels: DEG = CG_DEG is k_cgs's Chebyshev
// polynomial in the 2x2 block-Jacobi splitting A = D - N (Horner, DEG
// neighbour sums), DEG 0 = D^-1 (2x2 blocks if BLOCK, else scipy's scalar
// Jacobi).  Vectors live in global memory (L2-resident at these sizes);
// sweeps are separated by workgroup barriers; reductions are fixed-order fp64.
#define CGW_BX 64
#define CGW_BY 16
#ifndef CG_SMALL_PX
#define CG_SMALL_PX 4096
#endif

struct CgSmallArgs {
  const float *coef;  // 7 planes, plane stride ps
  size_t ps;
  const float2 *b;
  float2 *x, *r, *p, *q, *y, *t;
  int H, W, P;
  double rtol;
  int maxiter;
  float poly[8];
  PcgState *st;
  float2 *xh;      // 'backslash': x_hi of the residual replacement (k_cg_update)
  double upd_rel;  // ... done once at ||r|| < upd_rel ||b|| (0: never)
};

// (not to be merged with precond, kernels_solve.hip, or cg_inv, kernels_cg.hip:
// plain product difference and rcp here; they round otherwise)
template <bool BLOCK>
__device__ __forceinline__ void cgw_inv(const float *cf, size_t ps, size_t k, float &ia, float &ic, float &id) {
  const float a = cf[4 * ps + k], cc = cf[5 * ps + k], d = cf[6 * ps + k];
  ia = fabsf(a) > 1e-12f ? __builtin_amdgcn_rcpf(a) : 0.f;  // base.py:129-131
  id = fabsf(d) > 1e-12f ? __builtin_amdgcn_rcpf(d) : 0.f;
  ic = 0.f;
  if (BLOCK) {
    const float det = a * d - cc * cc;
    const bool ok = det > 1e-30f * fabsf(a * d);
    const float inv = __builtin_amdgcn_rcpf(det);
    ia = ok ? d * inv : ia;
    id = ok ? a * inv : id;
    ic = ok ? -cc * inv : 0.f;
  }
}
template <bool BLOCK>
__device__ __forceinline__ float2 cgw_minv(const float *cf, size_t ps, size_t k, float2 f) {
  float ia, ic, id;
  cgw_inv<BLOCK>(cf, ps, k, ia, ic, id);
  return make_float2(ia * f.x + ic * f.y, ic * f.x + id * f.y);
}
// (N f)(i, j): edge weight x neighbour value over the 4 neighbours, u and v
__device__ __forceinline__ float2 cgw_nsum(const float *cf, size_t ps, const float2 *f, int i, int j, int H, int W,
                                           int P) {
  const size_t k = (size_t)i * P + j;
  float su = 0.f, sv = 0.f;
  if (j > 0) {
    const float2 n = f[k - 1];
    su += cf[k - 1] * n.x;
    sv += cf[2 * ps + k - 1] * n.y;
  }
  if (j + 1 < W) {
    const float2 n = f[k + 1];
    su += cf[k] * n.x;
    sv += cf[2 * ps + k] * n.y;
  }
  if (i > 0) {
    const float2 n = f[k - P];
    su += cf[ps + k - P] * n.x;
    sv += cf[3 * ps + k - P] * n.y;
  }
  if (i + 1 < H) {
    const float2 n = f[k + P];
    su += cf[ps + k] * n.x;
    sv += cf[3 * ps + k] * n.y;
  }
  return make_float2(su, sv);
}
// fixed-order fp64 sum over the workgroup, returned to every thread
__device__ __forceinline__ double cgw_sum(double v, double *lds) {
  const int tid = threadIdx.x + threadIdx.y * CGW_BX;
  v = wave_sum(v);
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < CGW_BX * CGW_BY / 64; ++w) s += lds[w];
  __syncthreads();
  return s;
}

#define CGW_FOR_PIXELS(H, W)                                  \
  for (int i = threadIdx.y; i < (H); i += CGW_BY)             \
    for (int j = threadIdx.x; j < (W); j += CGW_BX)

template <int DEG, bool BLOCK>
__global__ __launch_bounds__(CGW_BX *CGW_BY) void k_cg_small(CgSmallArgs g) {
  __shared__ double lds[CGW_BX * CGW_BY / 64];
  const int H = g.H, W = g.W, P = g.P;
  const size_t ps = g.ps;
  const float *cf = g.coef;
  double acc = 0.0;
  CGW_FOR_PIXELS(H, W) {
    const size_t k = (size_t)i * P + j;
    const float2 bb = g.b[k];
    g.x[k] = make_float2(0.f, 0.f);
    g.r[k] = bb;
    g.p[k] = make_float2(0.f, 0.f);
    acc += (double)(bb.x * bb.x + bb.y * bb.y);
  }
  double rr = cgw_sum(acc, lds);
  const double bnorm = sqrt(rr), atol = g.rtol * bnorm;
  double rho_prev = 1.0;
  int it = 0, done = 0, upd = 0;
  for (;; ++it) {
    if (!upd && it > 0 && sqrt(rr) < g.upd_rel * bnorm) {
      // residual replacement (see k_cg_update): r = b - A x in fp64, x_hi = x,
      // x_lo = 0; p and rho_prev are kept
      acc = 0.0;
      CGW_FOR_PIXELS(H, W) {
        const size_t k = (size_t)i * P + j;
        const double2 rv = resid_px(cf, ps, g.b, g.x, nullptr, i, j, H, W, P);
        const float2 rf = make_float2((float)rv.x, (float)rv.y);
        g.r[k] = rf;
        g.xh[k] = g.x[k];
        acc += (double)rf.x * rf.x + (double)rf.y * rf.y;
      }
      rr = cgw_sum(acc, lds);  // (barrier: every x read done)
      CGW_FOR_PIXELS(H, W) g.x[(size_t)i * P + j] = make_float2(0.f, 0.f);
      __syncthreads();
      upd = 1;
    }
    if (rr == 0.0 && it == 0) { done = 3; break; }
    if (sqrt(rr) < atol || rr == 0.0) { done = 1; break; }
    if (it >= g.maxiter) { done = 2; break; }
    // z = M^-1 r (into t), rho = r.z
    acc = 0.0;
    if (DEG == 0) {
      CGW_FOR_PIXELS(H, W) {
        const size_t k = (size_t)i * P + j;
        const float2 rk = g.r[k], z = cgw_minv<BLOCK>(cf, ps, k, rk);
        g.t[k] = z;
        acc += (double)(rk.x * z.x + rk.y * z.y);
      }
    } else {
      // Horner: g_DEG-1 = c_DEG-1 y + c_DEG B y, g_i = c_i y + B g_i+1, z = g_0
      CGW_FOR_PIXELS(H, W) {
        const size_t k = (size_t)i * P + j;
        g.y[k] = cgw_minv<BLOCK>(cf, ps, k, g.r[k]);
      }
      __syncthreads();
      CGW_FOR_PIXELS(H, W) {
        const size_t k = (size_t)i * P + j;
        const float2 ny = cgw_minv<BLOCK>(cf, ps, k, cgw_nsum(cf, ps, g.y, i, j, H, W, P)), yk = g.y[k];
        g.t[k] = make_float2(g.poly[DEG - 1] * yk.x + g.poly[DEG] * ny.x, g.poly[DEG - 1] * yk.y + g.poly[DEG] * ny.y);
      }
      float2 *src = g.t, *dst = g.q;
#pragma unroll
      for (int d = DEG - 2; d >= 0; --d) {
        __syncthreads();
        CGW_FOR_PIXELS(H, W) {
          const size_t k = (size_t)i * P + j;
          const float2 ng = cgw_minv<BLOCK>(cf, ps, k, cgw_nsum(cf, ps, src, i, j, H, W, P)), yk = g.y[k];
          const float2 v = make_float2(g.poly[d] * yk.x + ng.x, g.poly[d] * yk.y + ng.y);
          dst[k] = v;
          if (d == 0) {
            const float2 rk = g.r[k];
            acc += (double)(rk.x * v.x + rk.y * v.y);
          }
        }
        float2 *tmp = src;
        src = dst;
        dst = tmp;
      }
      if (src != g.t) {  // z into t
        __syncthreads();
        CGW_FOR_PIXELS(H, W) {
          const size_t k = (size_t)i * P + j;
          g.t[k] = src[k];
        }
      }
    }
    const double rho = cgw_sum(acc, lds);  // (barrier: t complete)
    const float beta = it == 0 ? 0.f : (float)(rho / rho_prev);
    CGW_FOR_PIXELS(H, W) {
      const size_t k = (size_t)i * P + j;
      const float2 z = g.t[k], pk = g.p[k];
      g.p[k] = make_float2(z.x + beta * pk.x, z.y + beta * pk.y);
    }
    __syncthreads();
    acc = 0.0;
    CGW_FOR_PIXELS(H, W) {  // q = A p = D p - N p
      const size_t k = (size_t)i * P + j;
      const float2 pk = g.p[k], np = cgw_nsum(cf, ps, g.p, i, j, H, W, P);
      const float a = cf[4 * ps + k], cc = cf[5 * ps + k], d = cf[6 * ps + k];
      const float2 qk = make_float2(a * pk.x + cc * pk.y - np.x, cc * pk.x + d * pk.y - np.y);
      g.q[k] = qk;
      acc += (double)(pk.x * qk.x + pk.y * qk.y);
    }
    const double pq = cgw_sum(acc, lds);
    if (!(pq > 0.0) || !(rho > 0.0)) { done = 1; break; }  // underflow (see cg_prologue)
    const float alpha = (float)(rho / pq);
    acc = 0.0;
    CGW_FOR_PIXELS(H, W) {
      const size_t k = (size_t)i * P + j;
      const float2 pk = g.p[k], qk = g.q[k], xk = g.x[k], rk = g.r[k];
      g.x[k] = make_float2(xk.x + alpha * pk.x, xk.y + alpha * pk.y);
      const float2 rn = make_float2(rk.x - alpha * qk.x, rk.y - alpha * qk.y);
      g.r[k] = rn;
      acc += (double)(rn.x * rn.x + rn.y * rn.y);
    }
    rr = cgw_sum(acc, lds);
    rho_prev = rho;
  }
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    g.st->iter = it;
    g.st->done = done;
    g.st->rr = rr;
    g.st->bnorm = bnorm;
    g.st->atol = atol;
    g.st->upd_k = upd;
  }
}
template __global__ void k_cg_small<CG_DEG, true>(CgSmallArgs);
template __global__ void k_cg_small<0, false>(CgSmallArgs);

// ---------------------------------------------------------------------------
// k_cg_reg: the same whole-solve-in-one-workgroup CG (scipy control flow,
// same preconditioners, the 'backslash' residual replacement) for levels of
// at most CG_REG_PX = 2048 pixels (17x30 and 34x60 at 1080p), with every
// vector in REGISTERS: thread t owns the pixels e = t + 512 m (m < CGR_M) of
// the dense row-major index e = i W + j, holds their coefficients, D^-1 and
// x, r, p, y, g, q, and exchanges neighbour values through a double-buffered
// LDS copy of the one field a stencil application reads (one barrier per
// exchange: 6 per iteration at degree 5), and reduces dot products through
// per-wave LDS slots in a fixed order (one barrier each; deterministic).
// k_cg_small walked every vector through global memory with a barrier per
// sweep: ~14 us per iteration at 17x30 / 34x60.
// 512 threads (2 waves per SIMD: up to 256 VGPRs) x 4 pixels; 1024 x 4
// spilled 656 B/lane at the 128 VGPRs a 1024-thread block allows, 1024 x 2
// still 100 B/lane
#define CGR_T 512
#define CGR_M 4
#define CG_REG_PX (CGR_T * CGR_M)

template <int DEG, bool BLOCK>
__global__ __launch_bounds__(CGR_T) void k_cg_reg(CgSmallArgs g) {
  __shared__ float2 ex[2][CG_REG_PX];
  // (u, v) weights of the edges right of / below every pixel: the left / up
  // weights of pixel e are those of e - 1 / e - W (registers held all four
  // and spilled 100 B/lane at 256 VGPRs)
  __shared__ float2 w_rt[CG_REG_PX], w_dn[CG_REG_PX];
  __shared__ double red[2][CGR_T / 64][2];
  const int tid = threadIdx.x + threadIdx.y * CGW_BX, wv = tid >> 6;
  const int H = g.H, W = g.W, P = g.P, N = H * W;
  const size_t ps = g.ps;
  const float *cf = g.coef;
  int e[CGR_M];
  bool ok[CGR_M], hl[CGR_M], hu[CGR_M];  // pixel owned; has a left / upper neighbour
  // coefficients: weights of the edges right / down (u, v), the 2x2 block
  // (a, c, d) and its inverse (ia, ic, id)
  float wr_u[CGR_M], wd_u[CGR_M], wr_v[CGR_M], wd_v[CGR_M];
  float ca[CGR_M], cc[CGR_M], cd[CGR_M], ia[CGR_M], ic[CGR_M], id[CGR_M];
  float2 x[CGR_M], r[CGR_M], p[CGR_M];
  // pitched offset of owned pixel m (a macro: lambdas taking the arrays by
  // reference made them addressable and spilled them)
#define CGR_KOF(m) ((size_t)((ok[m] ? e[m] : 0) / W) * P + ((ok[m] ? e[m] : 0) % W))
#pragma unroll
  for (int m = 0; m < CGR_M; ++m) {
    e[m] = tid + CGR_T * m;
    ok[m] = e[m] < N;
    const int ee = ok[m] ? e[m] : 0;
    const int i = ee / W, j = ee - i * W;
    const size_t k = (size_t)i * P + j;
    hl[m] = ok[m] && j > 0;
    hu[m] = ok[m] && i > 0;
    wr_u[m] = ok[m] && j + 1 < W ? cf[k] : 0.f;
    wd_u[m] = ok[m] && i + 1 < H ? cf[ps + k] : 0.f;
    wr_v[m] = ok[m] && j + 1 < W ? cf[2 * ps + k] : 0.f;
    wd_v[m] = ok[m] && i + 1 < H ? cf[3 * ps + k] : 0.f;
    if (ok[m]) {
      w_rt[ee] = make_float2(wr_u[m], wr_v[m]);
      w_dn[ee] = make_float2(wd_u[m], wd_v[m]);
    }
    ca[m] = ok[m] ? cf[4 * ps + k] : 0.f;
    cc[m] = ok[m] ? cf[5 * ps + k] : 0.f;
    cd[m] = ok[m] ? cf[6 * ps + k] : 0.f;
    if (ok[m]) {
      cgw_inv<BLOCK>(cf, ps, k, ia[m], ic[m], id[m]);
    } else {
      ia[m] = ic[m] = id[m] = 0.f;
    }
    x[m] = make_float2(0.f, 0.f);
    r[m] = ok[m] ? g.b[k] : make_float2(0.f, 0.f);
    p[m] = make_float2(0.f, 0.f);
  }
  __syncthreads();  // w_rt / w_dn complete
  int buf = 0, rb = 0;
  // left / up weights of owned pixel m (0 without that neighbour)
#define CGR_WL(m) (hl[m] ? w_rt[e[m] - 1] : make_float2(0.f, 0.f))
#define CGR_WU(m) (hu[m] ? w_dn[e[m] - W] : make_float2(0.f, 0.f))
  // neighbour sum N f of owned pixel m after exch(f)
  // (macro, not a lambda taking the array: an array reference kept the
  // Horner temporaries addressable and spilled them to scratch)
#define CGR_EXCH(f)                                  \
  {                                                   \
    _Pragma("unroll") for (int m = 0; m < CGR_M; ++m) \
      if (ok[m]) ex[buf][e[m]] = (f)[m];              \
    __syncthreads();                                  \
  }
#define nsum(m)                                                                                              \
  ({                                                                                                         \
    const float2 *X_ = ex[buf];                                                                              \
    const int c_ = ok[m] ? e[m] : 0;                                                                         \
    const float2 L_ = X_[max(c_ - 1, 0)], R_ = X_[min(c_ + 1, N - 1)], U_ = X_[max(c_ - W, 0)],              \
                 D_ = X_[min(c_ + W, N - 1)];                                                                \
    const float2 a_ = CGR_WL(m), b_ = CGR_WU(m);                                                             \
    make_float2(a_.x * L_.x + wr_u[m] * R_.x + b_.x * U_.x + wd_u[m] * D_.x,                                 \
                a_.y * L_.y + wr_v[m] * R_.y + b_.y * U_.y + wd_v[m] * D_.y);                                \
  })
#define minv(m, f)                                                                                           \
  ({                                                                                                         \
    const float2 f_ = (f);                                                                                   \
    make_float2(ia[m] * f_.x + ic[m] * f_.y, ic[m] * f_.x + id[m] * f_.y);                                   \
  })
  // fixed-order fp64 sums of two per-thread values over the workgroup
  auto reduce2 = [&](double v0, double v1, double &s0, double &s1) {
    v0 = wave_sum(v0);
    v1 = wave_sum(v1);
    if ((tid & 63) == 0) {
      red[rb][wv][0] = v0;
      red[rb][wv][1] = v1;
    }
    __syncthreads();
    s0 = 0.0;
    s1 = 0.0;
#pragma unroll
    for (int w = 0; w < CGR_T / 64; ++w) {
      s0 += red[rb][w][0];
      s1 += red[rb][w][1];
    }
    rb ^= 1;
  };
  double acc0 = 0.0;
#pragma unroll
  for (int m = 0; m < CGR_M; ++m) acc0 += (double)(r[m].x * r[m].x + r[m].y * r[m].y);
  double rr, dummy;
  reduce2(acc0, 0.0, rr, dummy);
  const double bnorm = sqrt(rr), atol = g.rtol * bnorm;
  double rho_prev = 1.0;
  int it = 0, done = 0, upd = 0;
  for (;; ++it) {
    if (!upd && it > 0 && sqrt(rr) < g.upd_rel * bnorm) {
      // residual replacement (see k_cg_update): r = b - A x in fp64, x_hi = x,
      // x_lo = 0; p and rho_prev are kept
      CGR_EXCH(x);
      acc0 = 0.0;
#pragma unroll
      for (int m = 0; m < CGR_M; ++m) {
        const float2 *X = ex[buf];
        const int c = ok[m] ? e[m] : 0;
        const float2 L = X[max(c - 1, 0)], R = X[min(c + 1, N - 1)], U = X[max(c - W, 0)], D = X[min(c + W, N - 1)];
        const float2 bm = ok[m] ? g.b[CGR_KOF(m)] : make_float2(0.f, 0.f);
        const float2 a = CGR_WL(m), b = CGR_WU(m);
        const double su = (double)bm.x - ((double)ca[m] * x[m].x + (double)cc[m] * x[m].y) +
                          (double)a.x * L.x + (double)wr_u[m] * R.x + (double)b.x * U.x +
                          (double)wd_u[m] * D.x;
        const double sv = (double)bm.y - ((double)cc[m] * x[m].x + (double)cd[m] * x[m].y) +
                          (double)a.y * L.y + (double)wr_v[m] * R.y + (double)b.y * U.y +
                          (double)wd_v[m] * D.y;
        r[m] = ok[m] ? make_float2((float)su, (float)sv) : make_float2(0.f, 0.f);
        acc0 += (double)r[m].x * r[m].x + (double)r[m].y * r[m].y;
        if (ok[m]) g.xh[CGR_KOF(m)] = x[m];  // x_hi (read back by k_cg_finalize)
        x[m] = make_float2(0.f, 0.f);
      }
      buf ^= 1;
      reduce2(acc0, 0.0, rr, dummy);
      upd = 1;
    }
    if (rr == 0.0 && it == 0) { done = 3; break; }
    if (sqrt(rr) < atol || rr == 0.0) { done = 1; break; }
    if (it >= g.maxiter) { done = 2; break; }
    // z = M^-1 r (Horner in B = D^-1 N), rho = r.z
    float2 z[CGR_M];
    if (DEG == 0) {
#pragma unroll
      for (int m = 0; m < CGR_M; ++m) z[m] = minv(m, r[m]);
    } else {
      float2 y[CGR_M];
#pragma unroll
      for (int m = 0; m < CGR_M; ++m) y[m] = minv(m, r[m]);
      CGR_EXCH(y);
#pragma unroll
      for (int m = 0; m < CGR_M; ++m) {
        const float2 ny = minv(m, nsum(m));
        z[m] = make_float2(g.poly[DEG - 1] * y[m].x + g.poly[DEG] * ny.x, g.poly[DEG - 1] * y[m].y + g.poly[DEG] * ny.y);
      }
      buf ^= 1;
#pragma unroll
      for (int d = DEG - 2; d >= 0; --d) {
        CGR_EXCH(z);
#pragma unroll
        for (int m = 0; m < CGR_M; ++m) {
          const float2 ng = minv(m, nsum(m));
          z[m] = make_float2(g.poly[d] * y[m].x + ng.x, g.poly[d] * y[m].y + ng.y);
        }
        buf ^= 1;
      }
    }
    acc0 = 0.0;
#pragma unroll
    for (int m = 0; m < CGR_M; ++m) acc0 += (double)(r[m].x * z[m].x + r[m].y * z[m].y);
    double rho;
    reduce2(acc0, 0.0, rho, dummy);
    const float beta = it == 0 ? 0.f : (float)(rho / rho_prev);
#pragma unroll
    for (int m = 0; m < CGR_M; ++m) p[m] = make_float2(z[m].x + beta * p[m].x, z[m].y + beta * p[m].y);
    // q = A p = D p - N p, pq = p.q
    CGR_EXCH(p);
    float2 q[CGR_M];
    acc0 = 0.0;
#pragma unroll
    for (int m = 0; m < CGR_M; ++m) {
      const float2 np = nsum(m);
      q[m] = make_float2(ca[m] * p[m].x + cc[m] * p[m].y - np.x, cc[m] * p[m].x + cd[m] * p[m].y - np.y);
      acc0 += (double)(p[m].x * q[m].x + p[m].y * q[m].y);
    }
    buf ^= 1;
    double pq;
    reduce2(acc0, 0.0, pq, dummy);
    if (!(pq > 0.0) || !(rho > 0.0)) { done = 1; break; }  // underflow (see cg_prologue)
    const float alpha = (float)(rho / pq);
    acc0 = 0.0;
#pragma unroll
    for (int m = 0; m < CGR_M; ++m) {
      x[m] = make_float2(x[m].x + alpha * p[m].x, x[m].y + alpha * p[m].y);
      r[m] = make_float2(r[m].x - alpha * q[m].x, r[m].y - alpha * q[m].y);
      acc0 += (double)(r[m].x * r[m].x + r[m].y * r[m].y);
    }
    reduce2(acc0, 0.0, rr, dummy);
    rho_prev = rho;
  }
#pragma unroll
  for (int m = 0; m < CGR_M; ++m)
    if (ok[m]) {
      g.x[CGR_KOF(m)] = x[m];
    }
  if (tid == 0) {
    g.st->iter = it;
    g.st->done = done;
    g.st->rr = rr;
    g.st->bnorm = bnorm;
    g.st->atol = atol;
    g.st->upd_k = upd;
  }
#undef CGR_EXCH
#undef nsum
#undef minv
#undef CGR_KOF
#undef CGR_WL
#undef CGR_WU
}
template __global__ void k_cg_reg<CG_DEG, true>(CgSmallArgs);
template __global__ void k_cg_reg<0, false>(CgSmallArgs);
