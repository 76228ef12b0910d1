// kernels_cg.hip — the fed CG: preconditioned CG with the exact control flow
// of scipy.sparse.linalg.cg (x0 = 0, stop when ||r|| < rtol ||b|| before an
// iteration, at most maxiter iterations), ONE launch per iteration.  Holds
// what both fused iteration kernels use (PcgArgs, the raw-buffer and packed
// fp32 helpers, CgCoef / CgInv, the launch prologue cg_prologue), scipy's
// Jacobi iteration k_cg ('pcg'), and the launches around an iteration:
// k_pcg_check, the residual replacement k_cg_update, k_cg_finalize.  The
// 'backslash' iteration k_cgs follows in kernels_cgs.hip.  Expects
// kernels_solve.hip before it (PCG_MAX_BLOCKS, CG_DEG, write_partials,
// prologue_sum, resid_px, cg_xlo_live).
// Shared by these kernels: every global reduction is finished in the
// PROLOGUE of the next launch (the launch-boundary reduce of
// kernels_solve.hip) from partials ping-ponged by iteration parity.
// Launches of a finished solve return after the prologue, so the host can
// enqueue iterations in chunks and poll a pinned status word.  Every launch
// of a solve has the same grid (PcgArgs.nb blocks of 64 x 4 threads).
#include "kernels.h"

struct PcgArgs {
  const float *coef;  // 7 planes, plane stride ps
  float2 *x;
  const float2 *r_in, *p_old;  // iterate k-1
  float2 *r_out, *p_new;       // iterate k
  const float2 *b;
  int H, W, P;
  size_t ps;
  int nb;  // blocks of this grid (== blocks of every launch of the solve)
  // per-block partial sums [5][PCG_MAX_BLOCKS], ping-ponged by iteration
  // parity: launch k reads launch k-1's (part_rd) and writes its own
  // (part_wr).  One buffer would race: a block that starts after another
  // block of the same grid has finished would read a mix of both launches.
  const double *part_rd;
  double *part_wr;
  PcgState *st;
  CgFlag *hflag;  // mapped host memory (may be null)
  double rtol;
  int maxiter;
  float poly[8];  // k_cgs: M^-1 = (poly[0] + poly[1] B + ... + poly[CG_DEG] B^CG_DEG) D^-1
  // 'backslash' residual replacement (k_cg_update; null / 0 for 'pcg'):
  // x_hi (the iterate at the replacement) and the relative residual at which
  // it acts
  float2 *xh;
  double upd_rel;
};

// ---------------------------------------------------------------------------
// q-free fused CG iteration on raw buffer loads (k_cg): the production CG
// kernel.  Textbook CG algebra with the rho recurrence and the
// launch-boundary reduction, but
//  - q_{k-1} = A p_{k-1} is recomputed from p_{k-1} (read anyway, 2-row
//    halo) instead of being stored and re-read: 76 B/px per iteration
//    (r, x read+write; p_old read; p_new write; 7 coefficient planes);
//  - every load is a raw buffer load whose out-of-image offsets (rows outside
//    [0, H), columns outside [0, W)) return 0 by the hardware range check, so
//    the stencil needs no boundary branches, and stores from halo lanes are
//    dropped the same way;
//  - the first iteration and an odd width are template parameters (the
//    preconditioner is scipy's scalar Jacobi, cg_inv<false>); dot products
//    are formed per lane in fp32 over the lane's two pixels and accumulated
//    in fp64;
//  - the launch prologue issues the partial-sum loads, the state loads and
//    the first pipeline rows together (one memory round trip, not four).
// Geometry: a wave owns PCG_SW = 124 output columns; lane l holds columns
// jc = j0 - 2 + 2l and jc + 1, so lanes 0 and 63 carry the strip halo and all
// horizontal neighbours are DPP wave shifts.  A band of R rows is swept top
// to bottom; step t prefetches row t+1 (coefficients, r_in) and p_old of row
// t+2, forms r, z, p of row t and finishes row t-1 (q = A p, stores, dots).
#define PCG_SW 124
#define CG_OOB 0x80000000u

typedef float cg_f2 __attribute__((ext_vector_type(2)));
typedef float cg_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t cg_rsrc(const void *p, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)min(bytes, (size_t)0x7fffffff), 0x00020000);
}
__device__ __forceinline__ cg_f2 cg_ld2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(cg_f2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ cg_f4 cg_ld4(__amdgpu_buffer_rsrc_t r, unsigned voff) {
  return __builtin_bit_cast(cg_f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0));
}
__device__ __forceinline__ void cg_st4(__amdgpu_buffer_rsrc_t r, unsigned voff, cg_f4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) int, v), r, (int)voff,
                                         0, 0);
}

struct CgCoef {  // one row, the lane's two pixels (x: first, y: second)
  cg_f2 wxu, wyu, wxv, wyv, a, c, d;
  float wlu, wlv;  // weight of the edge to the left of the first pixel
};

template <bool ODD>
__device__ __forceinline__ cg_f2 cg_mask1(cg_f2 v, bool ok1) {
  if (ODD && !ok1) v.y = 0.f;
  return v;
}
template <bool ODD>
__device__ __forceinline__ cg_f4 cg_mask1(cg_f4 v, bool ok1) {
  if (ODD && !ok1) { v.z = 0.f; v.w = 0.f; }
  return v;
}

// (A f)(row) for f = (u0, v0, u1, v1) rows up / mid / dn; wu = vertical
// weights of the row above (u: .x/.y = pixel 0/1 of wyu, v likewise)
__device__ __forceinline__ cg_f4 cg_apply(cg_f4 up, cg_f4 mid, cg_f4 dn, const CgCoef &c, cg_f2 wuu, cg_f2 wuv) {
  // a lane holds two columns of a CG strip: wave_from_prev (common.h) is the
  // column left of them, wave_from_next the column right, 0 beyond the strip
  const float Lu = wave_from_prev(mid.z), Lv = wave_from_prev(mid.w);
  const float Ru = wave_from_next(mid.x), Rv = wave_from_next(mid.y);
  const float s0u = c.wlu * Lu + c.wxu.x * mid.z + wuu.x * up.x + c.wyu.x * dn.x;
  const float s0v = c.wlv * Lv + c.wxv.x * mid.w + wuv.x * up.y + c.wyv.x * dn.y;
  const float s1u = c.wxu.x * mid.x + c.wxu.y * Ru + wuu.y * up.z + c.wyu.y * dn.z;
  const float s1v = c.wxv.x * mid.y + c.wxv.y * Rv + wuv.y * up.w + c.wyv.y * dn.w;
  cg_f4 o;
  o.x = c.a.x * mid.x + c.c.x * mid.y - s0u;
  o.y = c.c.x * mid.x + c.d.x * mid.y - s0v;
  o.z = c.a.y * mid.z + c.c.y * mid.w - s1u;
  o.w = c.c.y * mid.z + c.d.y * mid.w - s1v;
  return o;
}

// inverse of the preconditioner block of both pixels: (ia, ic, id) with
// M^-1 (ru, rv) = (ia ru + ic rv, ic ru + id rv)
struct CgInv {
  cg_f2 ia, ic, id;
};
// (not to be merged with precond, kernels_solve.hip, or cgw_inv,
// kernels_cg_wg.hip: explicit fma determinant and rcp here; they round otherwise)
template <bool BLOCK>
__device__ __forceinline__ CgInv cg_inv(const CgCoef &c) {
  CgInv o;
  if (BLOCK) {
    // the 2x2 inverse where det > 1e-30 |a d| (explicit fma: the same
    // rounding wherever the inverse is formed), else scalar Jacobi.  On an
    // assembled operator every lane passes, so the fallback's reciprocals
    // and selects sit behind a wave-uniform branch: lanes that pass get the
    // same values either way
    bool ok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float a = c.a[e], cc = c.c[e], d = c.d[e];
      const float det = __builtin_fmaf(a, d, -(cc * cc));
      ok[e] = det > 1e-30f * fabsf(a * d);
      const float inv = __builtin_amdgcn_rcpf(det);
      o.ia[e] = d * inv;
      o.id[e] = a * inv;
      o.ic[e] = -cc * inv;
    }
    if (__builtin_amdgcn_ballot_w64(!(ok[0] && ok[1])) != 0) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float a = c.a[e], d = c.d[e];
        const float ja = fabsf(a) > 1e-12f ? __builtin_amdgcn_rcpf(a) : 0.f;
        const float jd = fabsf(d) > 1e-12f ? __builtin_amdgcn_rcpf(d) : 0.f;
        o.ia[e] = ok[e] ? o.ia[e] : ja;
        o.id[e] = ok[e] ? o.id[e] : jd;
        o.ic[e] = ok[e] ? o.ic[e] : 0.f;
      }
    }
    return o;
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    // scalar Jacobi, base.py:129-131: 1/diag where |diag| > 1e-12 else 0
    o.ia[e] = fabsf(c.a[e]) > 1e-12f ? __builtin_amdgcn_rcpf(c.a[e]) : 0.f;
    o.id[e] = fabsf(c.d[e]) > 1e-12f ? __builtin_amdgcn_rcpf(c.d[e]) : 0.f;
    o.ic[e] = 0.f;
  }
  return o;
}
__device__ __forceinline__ cg_f4 cg_minv(const CgInv &m, cg_f4 r) {
  cg_f4 z;
  z.x = m.ia.x * r.x + m.ic.x * r.y;
  z.y = m.ic.x * r.x + m.id.x * r.y;
  z.z = m.ia.y * r.z + m.ic.y * r.w;
  z.w = m.ic.y * r.z + m.id.y * r.w;
  return z;
}
__device__ __forceinline__ float cg_dot(cg_f4 a, cg_f4 b) { return a.x * b.x + a.y * b.y + (a.z * b.z + a.w * b.w); }

// The lane's fixed-order partial sums of the 5 arrays of a 256-thread block
// (nb <= PCG_MAX_BLOCKS: at most PCG_MAX_BLOCKS / 256 terms per lane), every
// load issued before the first add.  A loop per array (the earlier form)
// waited for each array's loads before issuing the next array's: five memory
// round trips per launch, the first also draining the pipeline rows issued
// ahead of the prologue.  The same terms in the same order: the same sums.
__device__ __forceinline__ void cg_lane_partials(double (&S)[5], const double *__restrict__ part, int nb, int tid) {
  constexpr int MT = PCG_MAX_BLOCKS / 256;
  double t[MT][5];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int b = tid + m * 256, bc = b < nb ? b : 0;
#pragma unroll
    for (int v = 0; v < 5; ++v) t[m][v] = part[(size_t)v * PCG_MAX_BLOCKS + bc];
  }
#pragma unroll
  for (int v = 0; v < 5; ++v) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < MT; ++m) s = tid + m * 256 < nb ? s + t[m][v] : s;
    S[v] = s;
  }
}

// Launch prologue of k_cg / k_cgs: fixed-order sum of the previous launch's
// per-block partials (pq, qz, qMq, rz, rr) -> alpha_{k-1}, rho_k (CG
// recurrence), beta_k, scipy's convergence test; the lead block records the
// state.  Returns true when this launch has nothing to do.
template <bool FIRST>
__device__ __forceinline__ bool cg_prologue(const PcgArgs &g, int k, double *lds, float *alpha, float *beta,
                                            bool *xlo_zero = nullptr) {
  __shared__ int s_exit, s_xz;
  __shared__ float s_ab[2];
  const int tid = threadIdx.x + threadIdx.y * 64;
  int st_done = 0, st_updk = 0;
  double st_atol = 0.0, st_rho = 0.0;
  if (tid == 0) {
    st_done = g.st->done;
    st_atol = g.st->atol;
    st_updk = g.st->upd_k;
    if (k >= 2) st_rho = g.st->rho[(k - 1) & 1];  // launch k-1's recurrence value of r.z
  }
  // after a residual replacement (k_cg_update between launches k-1 and k)
  // S[4] is already the replaced residual's r.r: the update wrote it into
  // launch k-1's partials
  double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (!FIRST) {
    cg_lane_partials(S, g.part_rd, g.nb, tid);
#pragma unroll
    for (int v = 0; v < 5; ++v) S[v] = wave_sum(S[v]);
    if ((tid & 63) == 0)
#pragma unroll
      for (int v = 0; v < 5; ++v) lds[v * 8 + (tid >> 6)] = S[v];
  }
  __syncthreads();
  if (tid == 0) {
    int done = st_done ? -1 : 0;
    float al = 0.f, be = 0.f;
    const bool xz = !FIRST && st_updk == k;
    s_xz = xz;
    if (!FIRST && !done) {
#pragma unroll
      for (int v = 0; v < 5; ++v) S[v] = lds[v * 8] + lds[v * 8 + 1] + lds[v * 8 + 2] + lds[v * 8 + 3];
      const double rn = sqrt(S[4]);
      const double atol = k == 1 ? g.rtol * rn : st_atol;
      if (k == 1 && S[4] == 0.0) done = 3;
      else if (rn < atol || S[4] == 0.0) done = 1;  // exact solution: nothing left to divide
      const double a_ = S[3] / S[0];
      const double rho = S[3] - 2.0 * a_ * S[1] + a_ * a_ * S[2];
      // p.Ap, r.z or the recurrence's next r.z not positive: fp32 rounding
      // at the noise floor (rtol 0 runs past the representable residual; A
      // and M are SPD, so only rounding makes them vanish): stop there
      if (!done && (!(S[0] > 0.0) || !(S[3] > 0.0) || !(rho > 0.0))) done = 1;
      // the r.z the last sweep formed (S[3]) off the recurrence's prediction
      // of it by more than 10 % (they agree to ~1e-6 above the noise floor):
      // conjugacy is lost, restart with beta = 0 (a preconditioned steepest
      // descent step never increases the A-norm error) instead of letting
      // the recurrence drive the iterate away
      const bool drift = k >= 2 && !(fabs(S[3] - st_rho) <= 0.1 * S[3]);
      if (!done && k - 1 >= g.maxiter) done = 2;
      if (blockIdx.x == 0 && blockIdx.y == 0) {
        if (k == 1) { g.st->bnorm = rn; g.st->atol = atol; }
        g.st->iter = k - 1;
        g.st->rr = S[4];
        g.st->rho[k & 1] = rho;
        if (done) g.st->done = done;
        // residual replacement due (k_cg_update): read by update launches only
        if (!done && g.upd_rel > 0.0 && k >= 2 && rn < g.upd_rel * g.st->bnorm && !g.st->upd_due)
          g.st->upd_due = k;
      }
      al = (float)a_;
      be = drift ? 0.f : (float)(rho / S[3]);
    }
    if (FIRST && blockIdx.x == 0 && blockIdx.y == 0) {
      g.st->iter = 0;
      g.st->maxiter = g.maxiter;
    }
    if (g.hflag && blockIdx.x == 0 && blockIdx.y == 0 && done >= 0) {
      if (done > 0) {
        __hip_atomic_store(&g.hflag->iter, k - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&g.hflag->done, done, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      __hip_atomic_store(&g.hflag->k, k, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    s_exit = done;
    s_ab[0] = al;
    s_ab[1] = be;
  }
  __syncthreads();
  *alpha = s_ab[0];
  *beta = s_ab[1];
  if (xlo_zero) *xlo_zero = s_xz;
  return s_exit != 0;
}

template <bool FIRST, bool ODD>
__global__ __launch_bounds__(256) void k_cg(PcgArgs g, int k, int R, int nbands) {
  __shared__ double lds[64];
  const int H = g.H, W = g.W;
  const unsigned rowb4 = (unsigned)g.P * 4u, rowb8 = (unsigned)g.P * 8u;
  const size_t vbytes = (size_t)H * g.P * 8;
  const __amdgpu_buffer_rsrc_t rc = cg_rsrc(g.coef, g.ps * 7 * 4);
  const __amdgpu_buffer_rsrc_t rin = cg_rsrc(FIRST ? g.b : g.r_in, vbytes);
  const __amdgpu_buffer_rsrc_t rpo = cg_rsrc(g.p_old, vbytes);
  const __amdgpu_buffer_rsrc_t rx = cg_rsrc(g.x, vbytes);
  const __amdgpu_buffer_rsrc_t rro = cg_rsrc(g.r_out, vbytes);
  const __amdgpu_buffer_rsrc_t rpn = cg_rsrc(g.p_new, vbytes);
  const unsigned ps4 = (unsigned)(g.ps * 4);
  // XCD-aware tile order (common.h): neighbouring strips / band groups share
  // their halo rows in one L2.  The partials slot is the tile, so the
  // fixed-order sums (and the iterates) do not depend on the order
  const int tile = of_xcd_tile(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
  const int tby = tile / (int)gridDim.x, tbx = tile - tby * (int)gridDim.x;
  // threadIdx.y is wave-uniform (64 x 4 blocks): make every row index scalar
  const int lane = threadIdx.x, band = tby * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int jc = tbx * PCG_SW - 2 + 2 * lane;
  const bool ok0 = jc >= 0 && jc < W, ok1 = jc + 1 < W && jc >= 0;
  const bool out_lane = lane >= 1 && lane <= 62;
  const unsigned off4 = ok0 ? (unsigned)jc * 4u : CG_OOB, off8 = ok0 ? (unsigned)jc * 8u : CG_OOB;
  const unsigned soff8 = ok0 && out_lane ? (unsigned)jc * 8u : CG_OOB;
  const bool live = band < nbands;
  const int r0 = band * R, r1 = min(r0 + R, H);

  auto o4 = [&](int t) { return (unsigned)t < (unsigned)H ? off4 + (unsigned)t * rowb4 : CG_OOB; };
  auto o8 = [&](int t) { return (unsigned)t < (unsigned)H ? off8 + (unsigned)t * rowb8 : CG_OOB; };
  auto load_coef = [&](int t, CgCoef &c) {
    const unsigned v = o4(t);
    c.wxu = cg_mask1<ODD>(cg_ld2(rc, v, 0), ok1);
    c.wyu = cg_mask1<ODD>(cg_ld2(rc, v, ps4), ok1);
    c.wxv = cg_mask1<ODD>(cg_ld2(rc, v, 2 * ps4), ok1);
    c.wyv = cg_mask1<ODD>(cg_ld2(rc, v, 3 * ps4), ok1);
    c.a = cg_mask1<ODD>(cg_ld2(rc, v, 4 * ps4), ok1);
    c.c = cg_mask1<ODD>(cg_ld2(rc, v, 5 * ps4), ok1);
    c.d = cg_mask1<ODD>(cg_ld2(rc, v, 6 * ps4), ok1);
  };
  auto load_wy = [&](int t, cg_f2 &wu, cg_f2 &wv) {
    const unsigned v = o4(t);
    wu = cg_mask1<ODD>(cg_ld2(rc, v, ps4), ok1);
    wv = cg_mask1<ODD>(cg_ld2(rc, v, 3 * ps4), ok1);
  };
  auto load_po = [&](int t) { return FIRST ? cg_f4{0.f, 0.f, 0.f, 0.f} : cg_mask1<ODD>(cg_ld4(rpo, o8(t)), ok1); };
  auto load_rin = [&](int t) { return cg_mask1<ODD>(cg_ld4(rin, o8(t)), ok1); };

  // ---- pipeline preamble (independent of alpha/beta: issued before the
  // prologue's reduction so the two memory round trips overlap).  Rows live
  // in 4-slot register rings indexed by (row - (r0 - 1)) & 3, and the row
  // loop is unrolled by 4, so the pipeline advances without register moves.
  CgCoef C[4];   // coefficients, rows t-2 (vertical weights only) .. t+1
  cg_f4 PO[4];   // p_old, rows t-1 .. t+2
  cg_f4 RI[2];   // r_in, rows t, t+1
  if (live) {
    const int t = r0 - 1;
    load_wy(t - 2, C[2].wyu, C[2].wyv);
    load_coef(t - 1, C[3]);
    load_coef(t, C[0]);
    PO[3] = load_po(t - 1);
    PO[0] = load_po(t);
    PO[1] = load_po(t + 1);
    RI[0] = load_rin(t);
  }

  float alpha = 0.f, beta = 0.f;
  if (cg_prologue<FIRST>(g, k, lds, &alpha, &beta)) return;

  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
    const cg_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    cg_f4 PP[4] = {zero4, zero4, zero4, zero4};  // p, rows t-2 .. t
    cg_f4 RR[2] = {zero4, zero4}, ZZ[2] = {zero4, zero4}, XX[2] = {zero4, zero4};  // rows t-1, t
    CgInv MI[2];
    C[3].wlu = wave_from_prev(C[3].wxu.y);
    C[3].wlv = wave_from_prev(C[3].wxv.y);
    MI[1] = cg_inv<false>(C[3]);
    const bool dm0 = out_lane && ok0, dm1 = out_lane && ok1;  // pixels whose dots count
    for (int t0 = r0 - 1; t0 <= r1; t0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u;
        if (t > r1) break;
        CgCoef &cm2 = C[(u + 2) & 3], &cm1 = C[(u + 3) & 3], &c0 = C[u & 3], &cp1 = C[(u + 1) & 3];
        // prefetch: coefficients and r_in of row t+1, p_old of row t+2, x of row t
        load_coef(t + 1, cp1);
        RI[(u + 1) & 1] = load_rin(t + 1);
        PO[(u + 2) & 3] = load_po(t + 2);
        // (the x load and the stores below are issued at every step, outside
        // the band with an out-of-range offset: under a branch they lower
        // the compiler's s_waitcnt vmcnt to the fewest operations of any
        // path, and the wait then covers loads of this step)
        XX[u & 1] = FIRST ? zero4 : cg_mask1<ODD>(cg_ld4(rx, t >= r0 && t < r1 ? o8(t) : CG_OOB), ok1);
        // r, z, p of row t
        c0.wlu = wave_from_prev(c0.wxu.y);
        c0.wlv = wave_from_prev(c0.wxv.y);
        MI[u & 1] = cg_inv<false>(c0);
        cg_f4 r = RI[u & 1];
        if (!FIRST) r -= alpha * cg_apply(PO[(u + 3) & 3], PO[u & 3], PO[(u + 1) & 3], c0, cm1.wyu, cm1.wyv);
        const cg_f4 z = cg_minv(MI[u & 1], r);
        cg_f4 p = FIRST ? z : z + beta * PO[u & 3];
        const bool rv = (unsigned)t < (unsigned)H;
        if (!(rv && ok0)) { p.x = 0.f; p.y = 0.f; }
        if (!(rv && ok1)) { p.z = 0.f; p.w = 0.f; }
        PP[u & 3] = p;
        RR[u & 1] = r;
        ZZ[u & 1] = z;
        // finish row t-1
        const int o = t - 1;
        const cg_f4 pm1 = PP[(u + 3) & 3], rm1 = RR[(u + 1) & 1], zm1 = ZZ[(u + 1) & 1];
        unsigned so = o >= r0 ? soff8 + (unsigned)o * rowb8 : CG_OOB;
        asm("" : "+v"(so));  // keeps the select (else the stores go back under the branch)
        cg_st4(rro, so, rm1);
        cg_st4(rpn, so, pm1);
        cg_st4(rx, so, FIRST ? zero4 : XX[(u + 1) & 1] + alpha * PO[(u + 3) & 3]);
        if (o >= r0) {
          const cg_f4 q = cg_apply(PP[(u + 2) & 3], pm1, p, cm1, cm2.wyu, cm2.wyv);
          const cg_f4 mq = cg_minv(MI[(u + 1) & 1], q);
          // per-lane fp32 dots over the two pixels (halo lanes / padding masked)
          cg_f4 qm = q, rm = rm1;  // select, not multiply: halo lanes may hold inf/nan
          if (!dm0) { qm.x = 0.f; qm.y = 0.f; rm.x = 0.f; rm.y = 0.f; }
          if (!dm1) { qm.z = 0.f; qm.w = 0.f; rm.z = 0.f; rm.w = 0.f; }
          acc[0] += (double)cg_dot(pm1, qm);
          acc[1] += (double)cg_dot(qm, zm1);
          acc[2] += (double)cg_dot(qm, mq);
          acc[3] += (double)cg_dot(rm, zm1);
          acc[4] += (double)cg_dot(rm, rm1);
        }
      }
    }
  }
  write_partials<5>(acc, g.part_wr, lds, tile);
}

// The body of k_pcg_check, below, and of nothing else: the convergence test
// of cg_prologue on the last enqueued iterate.  Not cg_prologue<false>
// because that launch is not an iteration: it writes no host flag (the host
// reads the state back after it), offers no residual replacement and has no
// drift restart, since no sweep follows it; alpha and beta are formed as a
// prologue forms them and go unused.  Returns 1 when the solve is finished
// (state written).
__device__ __forceinline__ int pcg_prologue(const PcgArgs &g, int k, double *lds, float *alpha, float *beta) {
  __shared__ int s_exit;
  __shared__ float s_ab[2];
  double S[5];
  prologue_sum<5>(S, g.part_rd, g.nb, lds);  // of K_{k-1}: pq, qz, qMq, rz, rr
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const bool lead = blockIdx.x == 0 && blockIdx.y == 0;
    const double rn = sqrt(S[4]);
    const double atol = k == 1 ? g.rtol * rn : g.st->atol;
    int done = 0;
    if (k == 1 && S[4] == 0.0) done = 3;
    else if (rn < atol || S[4] == 0.0) done = 1;  // exact solution: nothing left to divide
    const double al = S[3] / S[0];
    const double rho = S[3] - 2.0 * al * S[1] + al * al * S[2];
    if (!done && (!(S[0] > 0.0) || !(S[3] > 0.0) || !(rho > 0.0))) done = 1;  // noise floor (cg_prologue)
    else if (!done && k - 1 >= g.maxiter) done = 2;
    if (lead) {
      if (k == 1) { g.st->bnorm = rn; g.st->atol = atol; }
      g.st->iter = k - 1;
      g.st->rr = S[4];
      g.st->rho[k & 1] = rho;
      if (done) g.st->done = done;
    }
    s_exit = done;
    s_ab[0] = (float)al;
    s_ab[1] = (float)(rho / S[3]);
  }
  __syncthreads();
  *alpha = s_ab[0];
  *beta = s_ab[1];
  return s_exit;
}

// after the last enqueued iteration: apply the convergence test to the last
// iterate and record the final state (1 block)
__global__ __launch_bounds__(256) void k_pcg_check(PcgArgs g, int k) {
  __shared__ double lds[64];
  if (g.st->done) return;
  float a, b;
  pcg_prologue(g, k, lds, &a, &b);
  if (threadIdx.x == 0 && threadIdx.y == 0 && !g.st->done) {
    g.st->iter = k - 1;
    g.st->done = 2;
  }
}

// ---------------------------------------------------------------------------
// Residual replacement of the 'backslash' surrogate (reliable update,
// Sleijpen & van der Vorst 1996): the fp32 CG's recursive residual drifts
// from b - A x by ~eps |A| |x| (|A||x| / |b| ~ 145 on Classic+NL robust
// stages, tools/fp32_floor.py), 6x the 1e-6 target at 1080p.  Once the
// recursive residual has fallen below upd_rel ||b|| (sqrt(rtol): 1e-3), ONE
// launch between CG launches k-1 and k replaces it by the true residual
// b - A x_{k-1}, evaluated in fp64 (stored fp32) from the fp32 operator, and
// moves x_{k-1} into x_hi; launch k restarts x_lo from 0 (cg_prologue: xz)
// and takes r.r from the replacement.  The second segment's x_lo is small,
// so its own drift is ~1e-3 of the first's and the recursive residual then
// tracks the true residual of x_hi + x_lo (fp64 sum) to the end; the solve's
// result is fl32(x_hi + x_lo) (k_cg_finalize).  p, the partials and the rho
// recurrence are kept (the replacement moves r by ~1e-5 of ||r||, far inside
// the 10 % restart test).  Enqueued every few launches; it acts at most once
// per solve and otherwise returns after its prologue, so the result does not
// depend on how many were enqueued.  Grid: the solve's nb blocks, each
// writing one r.r partial (fixed pixel set and order: deterministic).
// Reads x (halo), b, 7 coefficient planes; writes r, x_hi: 60 B/px.
__global__ __launch_bounds__(256) void k_cg_update(PcgArgs g, int k) {
  __shared__ double lds[64];
  __shared__ int s_act;
  const int tid = threadIdx.x + threadIdx.y * 64;
  if (tid == 0) {
    // every block decides alike: upd_due was set by an earlier CG launch's
    // prologue (its recursive residual below upd_rel ||b||), and st->upd_k
    // is written only with this k
    const int updk = g.st->upd_k;
    s_act = !g.st->done && k >= 2 && (updk == k || (updk == 0 && g.st->upd_due > 0));
  }
  __syncthreads();
  if (!s_act) return;
  const int bid = blockIdx.x + blockIdx.y * gridDim.x;
  const int H = g.H, W = g.W, P = g.P, n = H * W;
  float2 *r = const_cast<float2 *>(g.r_in);
  double acc[1] = {0.0};
  for (int e = bid * 256 + tid; e < n; e += g.nb * 256) {
    const int i = e / W, j = e - i * W;
    const size_t kk = (size_t)i * P + j;
    const double2 rv = resid_px(g.coef, g.ps, g.b, g.x, nullptr, i, j, H, W, P);
    const float2 rf = make_float2((float)rv.x, (float)rv.y);
    r[kk] = rf;
    g.xh[kk] = g.x[kk];
    acc[0] += (double)rf.x * rf.x + (double)rf.y * rf.y;
  }
  // the replaced r.r into launch k-1's partial slot 4, which launch k's
  // prologue sums (each block writes only its own slot; no block of this
  // launch reads the partials)
  write_partials<1>(acc, const_cast<double *>(g.part_rd) + 4 * PCG_MAX_BLOCKS, lds);
  if (tid == 0 && bid == 0) {
    g.st->upd_k = k;
    if (g.hflag) __hip_atomic_store(&g.hflag->upd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// the solve's result: x = fl32(x_hi + x_lo) after a residual replacement
// (k_cg_update / k_cg_small), else x unchanged
__global__ __launch_bounds__(256) void k_cg_finalize(float2 *x, const float2 *__restrict__ xh,
                                                     const PcgState *st, int H, int W, int P) {
  if (!st->upd_k) return;
  const bool lo = cg_xlo_live(st);
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    const float2 a = lo ? x[k] : make_float2(0.f, 0.f), h = xh[k];
    x[k] = make_float2((float)((double)a.x + (double)h.x), (float)((double)a.y + (double)h.y));
  }
}
