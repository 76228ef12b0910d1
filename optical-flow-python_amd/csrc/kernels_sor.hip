// kernels_sor.hip — lexicographic SOR of the flow system in three forms that
// produce the same iterate and sweep count bitwise: k_sor_lex (one launch per
// sweep, with k_sor_init / k_sor_final), k_sor_pipe (many sweeps in flight in
// one persistent launch, with k_sor_pipe_final) and k_sor_wg (the same
// pipeline in one workgroup for levels of at most 64 rows).  Holds their
// arguments (SorArgs, SorPipeArgs, SorWgArgs), the relaxation of one point
// (sor_relax and its companions), the sc1 hand-off helpers and the three unit
// bodies (sor_strip, sorp_unit, sorw_unit), which differ in hand-off and
// prefetch shape and are kept apart on purpose.  Expects kernels_solve.hip
// before it (PCG_MAX_BLOCKS); it shares nothing with the CG files.
// Shared by the three forms: a wave owns a strip of 64 rows of one half (u or
// v) and walks its anti-diagonals; every multiply-add of the relaxation is an
// explicit fma, so the rounding is fixed by the source; units are taken in
// dependency order, so a wait is only ever for a unit already running; every
// wait is bounded and reports through a fail word.
#include "kernels.h"

// ---------------------------------------------------------------------------
// Lexicographic SOR, exactly the reference's sweep order (base.py:138-172).
// The reference walks the 2N rows of the CSR matrix in order: all u unknowns
// in Fortran order (index i + j*H: down each column, columns left to right),
// then all v unknowns in the same order, each row relaxed in place
//   x_r <- (1 - w) x_r + w (b_r - sum_{c != r} A_rc x_c) / A_rr
// (rows with |A_rr| < 1e-15 skipped), and stops after the first sweep with
// ||x - x_old|| < tol ||x|| (at most max_iters sweeps, x0 = 0).
//
// With A = D - N (2x2 blocks D = [[a, c], [c, d]], N = edge weights), row
// (i, j) of the u half reads u(i-1, j), u(i, j-1) already relaxed this
// sweep, u(i+1, j), u(i, j+1) not yet, and v(i, j) of the previous sweep;
// the v half reads v neighbours the same way and the NEW u(i, j).  So a
// sweep is a Gauss-Seidel pass over the u plane followed by one over the v
// plane, and the update of (i, j) depends only on (i-1, j) and (i, j-1):
// every anti-diagonal i + j = const may be relaxed at once without changing
// a single operand.  The GPU form keeps the reference's iterate exactly
// (up to fp32 rounding):
//   - a launch is one sweep; each 64-thread block (one wave) owns a strip of
//     64 rows of ONE half (u or v); lane l = row i0 + l walks its own row,
//     and at step t relaxes column t - l, so the wave's active points form an
//     anti-diagonal: the up neighbour (relaxed by lane l-1 at step t-1) and
//     the down neighbour (lane l+1's not-yet-relaxed next point) arrive by
//     DPP lane shifts, left / right are the lane's own previous / next point;
//   - strips hand rows to each other through global memory: strip s needs
//     the relaxed last row of strip s-1 (same half), and the v strip s needs
//     the relaxed u of its own rows; producers publish their completed step
//     count every SOR_G steps (sc1 stores of x, s_waitcnt vmcnt(0), sc1 flag
//     store) and consumers poll with sc1 loads and read x only with sc1 loads
//     (MI355X_MICROARCH.md, hand-off table row 1: no L1 copy of x is ever
//     used, so no acquire fence is needed);
//   - blocks take their strip from a ticket counter in dependency order (u
//     strips 0.., then v strips 0..), so a block only ever waits for blocks
//     that hold lower tickets and are therefore already running: the launch
//     cannot deadlock whatever the dispatch order or occupancy;
//   - the stopping test of sweep k-1 runs in the prologue of launch k on the
//     per-strip fp64 partials (fixed order, so every block agrees), ping-
//     ponged by sweep parity.
// prefetch distance in steps (<= 7: ring of 8) and steps between progress
// publications: 7 / 32 vs 4 / 64 = 0.94 vs 1.15 ms per 480x640 sweep, the
// same iterate (profiles/r3i_sor_ab.log; 16 / 8 steps: 0.89 / 0.91 ms).
// Round 4: 8 steps (the round-3 note that 8 steps changed the iterate was the
// compiler contracting the relaxation differently in that build; with
// sor_relax's explicit fmas every setting gives the same iterate), which lets
// the pipelined kernel's sweeps trail each other closely (host_core.h
// OF_SOR_PIPE_WAVES note).
#ifndef SOR_D
#define SOR_D 7
#endif
#ifndef SOR_G
#define SOR_G 8
#endif
#define SOR_MAXS (PCG_MAX_BLOCKS / 2)

struct SorArgs {
  const float *coef;  // 7 planes {wx_u, wy_u, wx_v, wy_v, a, c, d}, plane stride ps
  const float2 *b;
  float2 *x;
  int H, W, P;
  size_t ps;
  int nstrips;          // strips per half; blocks per launch = 2 * nstrips
  int stride;           // progress stamp of launch k = k * stride + steps done
  unsigned *ticket;     // reset per solve
  int *prog;            // [2][SOR_MAXS] progress stamps, reset per solve
  int *fail;            // set when a hand-off wait gave up (reset per solve)
  const double *part_rd;  // [2 * nstrips][2] (dn, xn) of the previous sweep
  double *part_wr;
  PcgState *st;
  float omega;
  double tol;
  int maxiter;
};

__device__ __forceinline__ float2 sor_ld(const float2 *p) {
  const uint64_t v = __hip_atomic_load((const uint64_t *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_bit_cast(float2, v);
}
__device__ __forceinline__ void sor_st(float2 *p, float2 v) {
  __hip_atomic_store((uint64_t *)p, __builtin_bit_cast(uint64_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int sor_poll(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wave-uniform wait until *p >= need (need is wave-uniform).  Bounded: a
// producer that never arrives (a bug, never the schedule: producers hold
// lower tickets) ends the wait after ~2^21 polls with *fail set, so the
// launch always drains; the host turns *fail into an error.
__device__ __forceinline__ void sor_wait(const int *p, int need, int &known, int *fail) {
  for (int n = 0; known < need; ++n) {
    known = __builtin_amdgcn_readfirstlane(sor_poll(p));
    if (known >= need) break;
    if (n > (1 << 21)) {
      if (threadIdx.x == 0) __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      known = need;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// The relaxation of one point (base.py:161-163), x <- (1 - w) x + w (b -
// sigma) / a_rr with sigma = sum_{c != r} A_rc x_c = -(N x)_r + c x_other,
// shared by k_sor_lex and k_sor_pipe.  Every multiply-add is an explicit
// fmaf and the fp64 sums explicit fma: left to the compiler, the two kernels
// contracted different subsets of the products (the pipelined one packed
// some into v_pk_mul_f32 + v_add), so their iterates differed in the last
// bit; spelled out, the rounding is fixed by the source.
// SOR_RCP: multiply by 1 / a_rr formed at prefetch time instead of dividing
// on the step's dependency chain (an IEEE division is ~8 dependent
// instructions); rounds differently from the division (<= 1.5 ulp)
#ifndef SOR_RCP
#define SOR_RCP 0
#endif
__device__ __forceinline__ float sor_relax(float bb, float wl, float left, float wr, float right, float wd, float down,
                                           float wu, float up, float cc, float other, float dg, float old, float om,
                                           float om1) {
  float sgm = fmaf(wl, left, bb);
  sgm = fmaf(wr, right, sgm);
  sgm = fmaf(wd, down, sgm);
  sgm = fmaf(wu, up, sgm);
  sgm = fmaf(-cc, other, sgm);
#if SOR_RCP
  // dg holds 1 / a_rr here (0 where |a_rr| < 1e-15: the row is skipped)
  return dg == 0.f ? old : fmaf(om1, old, (om * sgm) * dg);
#else
  return fabsf(dg) < 1e-15f ? old : fmaf(om1, old, (om * sgm) / dg);
#endif
}
// v & (c ? ~0 : 0), opaque to the compiler (see the SOR prefetch rings)
__device__ __forceinline__ float sorw_keep(float v, bool c) {
  float r;
  asm("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(0u - (unsigned)c));
  return r;
}
// global (not generic) float pointers: global_load, counted in vmcnt only
typedef const __attribute__((address_space(1))) float sorw_gf;
// the diagonal as sor_relax takes it
__device__ __forceinline__ float sor_dg(float a) {
#if SOR_RCP
  return fabsf(a) < 1e-15f ? 0.f : 1.0f / a;
#else
  return a;
#endif
}
// ||x_new - x_old||^2 and ||x_new||^2 partial sums (fp64)
__device__ __forceinline__ void sor_acc(float nw, float old, double &dn, double &xn) {
  const double dd = (double)nw - (double)old;
  dn = fma(dd, dd, dn);
  xn = fma((double)nw, (double)nw, xn);
}

// one strip of one half: PH 0 relaxes u (x.x), PH 1 relaxes v (x.y)
template <int PH>
__device__ __forceinline__ void sor_strip(const SorArgs &a, int s, int k, double &dn, double &xn) {
  const int lane = threadIdx.x, H = a.H, W = a.W, P = a.P;
  const int i0 = s * 64, i = i0 + lane;
  const bool rowok = i < H;
  const size_t ps = a.ps;
  const float *wxp = a.coef + (PH ? 2 : 0) * ps, *wyp = a.coef + (PH ? 3 : 1) * ps;
  const float *dgp = a.coef + (PH ? 6 : 4) * ps, *ccp = a.coef + 5 * ps;
  const size_t row = (size_t)(rowok ? i : 0) * P;
  const bool has_up = s > 0, has_dn = i0 + 64 < H;
  const size_t row_up = (size_t)(has_up ? i0 - 1 : 0) * P, row_dn = (size_t)(has_dn ? i0 + 64 : 0) * P;
  const int nsteps = W + 63;
  const int base = k * a.stride;
  int *my = a.prog + PH * SOR_MAXS + s;
  const int *pup = a.prog + PH * SOR_MAXS + (s > 0 ? s - 1 : 0);
  const int *pu = a.prog + s;  // v half: the u strip of the same rows
  int known_up = 0, known_u = 0;
  const float om = a.omega, om1 = 1.0f - a.omega;

  // prefetch ring: column j of lane l lives in slot (j + l) & 7 = t & 7
  float2 X[8], XU[8], XD[8];
  float WX[8], WY[8], DG[8], CC[8], BB[8], WYU[8];
  auto fetch = [&](int t) {  // column t + SOR_D - lane
    const int tp = t + SOR_D, jp = tp - lane, q = tp & 7;
    // wave-uniform waits before reading relaxed values of other strips
    // lane 0 reads row i0-1 at column tp: strip s-1's lane 63 relaxes it at
    // its step tp + 63
    if (has_up && tp >= 0 && tp < W) sor_wait(pup, base + tp + 64, known_up, a.fail);
    // v half: lane l reads the relaxed u of (i0 + l, tp - l), done at the u
    // strip's step tp
    if (PH == 1 && tp >= 0 && tp < nsteps) sor_wait(pu, base + tp + 1, known_u, a.fail);
    const bool ok = rowok && jp >= 0 && jp < W;
    const size_t o = row + (ok ? jp : 0);
    X[q] = ok ? sor_ld(a.x + o) : make_float2(0.f, 0.f);
    WX[q] = ok && jp + 1 < W ? wxp[o] : 0.f;
    WY[q] = ok && i + 1 < H ? wyp[o] : 0.f;
    DG[q] = ok ? sor_dg(dgp[o]) : 0.f;
    CC[q] = ok ? ccp[o] : 0.f;
    BB[q] = ok ? (PH ? a.b[o].y : a.b[o].x) : 0.f;
    if (lane == 0) {
      const bool u = has_up && jp >= 0 && jp < W;
      XU[q] = u ? sor_ld(a.x + row_up + jp) : make_float2(0.f, 0.f);
      WYU[q] = u ? wyp[row_up + jp] : 0.f;
    }
    if (lane == 63) {
      const bool d = has_dn && jp >= 0 && jp < W;
      XD[q] = d ? sor_ld(a.x + row_dn + jp) : make_float2(0.f, 0.f);
    }
  };
#pragma unroll
  for (int t = -SOR_D; t < 0; ++t) fetch(t);

  float res = 0.f, wx_prev = 0.f, wy_prev = 0.f;
  for (int t0 = 0; t0 < nsteps; t0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u;
      if (t >= nsteps) break;
      fetch(t);
      const int j = t - lane, q = t & 7, q1 = (t + 1) & 7;
      const bool act = rowok && j >= 0 && j < W;
      const float2 xo = X[q];
      const float old = PH ? xo.y : xo.x, other = PH ? xo.x : xo.y;
      // right neighbour: this lane's next point (not yet relaxed)
      const float right = PH ? X[q1].y : X[q1].x;
      // (a lane holds one row of an SOR strip: wave_from_prev, common.h, is the
      // row above, wave_from_next the row below)
      // down neighbour: lane l+1's next point; the last lane reads strip s+1
      float down = wave_from_next(right);
      if (lane == 63) down = PH ? XD[q].y : XD[q].x;
      // up neighbour: lane l-1's point of the previous step; lane 0 strip s-1
      float up = wave_from_prev(res), wu = wave_from_prev(wy_prev);
      if (lane == 0) {
        up = PH ? XU[q].y : XU[q].x;
        wu = WYU[q];
      }
      float nw = sor_relax(BB[q], wx_prev, res, WX[q], right, WY[q], down, wu, up, CC[q], other, DG[q], old, om, om1);
      if (act) {
        const size_t o = row + j;
        sor_st(a.x + o, PH ? make_float2(other, nw) : make_float2(nw, other));
        sor_acc(nw, old, dn, xn);
      } else {
        nw = 0.f;
      }
      res = nw;
      wx_prev = act ? WX[q] : 0.f;
      wy_prev = act ? WY[q] : 0.f;
      if (((t + 1) & (SOR_G - 1)) == 0 || t + 1 == nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(my, base + t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_sor_lex(SorArgs a, int k) {
  __shared__ int s_exit;
  const int lane = threadIdx.x;
  const int nb = 2 * a.nstrips;
  int tk = 0;
  if (lane == 0) tk = (int)atomicAdd(a.ticket, 1u) - k * nb;
  tk = __builtin_amdgcn_readfirstlane(__shfl(tk, 0, 64));
  if (lane == 0) {
    int done = a.st->done ? -1 : 0;
    if (!done && k > 0) {
      double dn = 0.0, xn = 0.0;
      for (int b = 0; b < nb; ++b) {  // fixed order: identical in every block
        dn += a.part_rd[2 * b];
        xn += a.part_rd[2 * b + 1];
      }
      done = sqrt(dn) < a.tol * sqrt(xn) ? 1 : (k >= a.maxiter ? 2 : 0);
      if (tk == 0) {
        a.st->iter = k;
        a.st->rr = dn;
        a.st->xnorm2 = xn;
        if (done) a.st->done = done;
      }
    }
    s_exit = done;
  }
  __syncthreads();
  if (s_exit) return;
  double dn = 0.0, xn = 0.0;
  const int ph = tk >= a.nstrips ? 1 : 0, s = ph ? tk - a.nstrips : tk;
  if (ph) sor_strip<1>(a, s, k, dn, xn);
  else sor_strip<0>(a, s, k, dn, xn);
  dn = wave_sum(dn);
  xn = wave_sum(xn);
  if (lane == 0) {
    const int slot = ph * a.nstrips + s;  // fixed slot per strip: deterministic sums
    a.part_wr[2 * slot] = dn;
    a.part_wr[2 * slot + 1] = xn;
  }
}

__global__ __launch_bounds__(64) void k_sor_init(SorArgs a) {
  for (int e = threadIdx.x + blockIdx.x * 64; e < a.H * a.P; e += gridDim.x * 64) a.x[e] = make_float2(0.f, 0.f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.st->iter = 0;
    a.st->maxiter = a.maxiter;
    a.st->done = a.maxiter <= 0 ? 2 : 0;
  }
}

// after the last enqueued sweep k-1: its stopping test (1 wave)
__global__ __launch_bounds__(64) void k_sor_final(SorArgs a, int k) {
  if (threadIdx.x != 0 || a.st->done) return;
  double dn = 0.0, xn = 0.0;
  for (int b = 0; b < 2 * a.nstrips; ++b) {
    dn += a.part_rd[2 * b];
    xn += a.part_rd[2 * b + 1];
  }
  a.st->iter = k;
  a.st->rr = dn;
  a.st->xnorm2 = xn;
  a.st->done = sqrt(dn) < a.tol * sqrt(xn) ? 1 : 2;
}

// ---------------------------------------------------------------------------
// Pipelined lexicographic SOR: many sweeps in flight in ONE persistent launch.
//
// k_sor_lex runs one sweep per launch, so sweep k+1 starts only when the last
// strip of sweep k has ended, and a 480x640 sweep keeps 16 waves busy on a
// 1024-SIMD chip.  But Gauss-Seidel in lexicographic order needs, at point
// (i, j) of sweep k+1, only values sweep k has already produced there: the
// old u, v at (i, j), (i, j+1), (i+1, j), which sweep k wrote when its own
// wavefront passed.  So sweep k+1 can trail sweep k at a fixed distance, and
// so on: sweeps k+1, k+2, ... run side by side, each a wavefront behind the
// previous one.  Every point is still relaxed from exactly the operands of
// the reference's order, so the iterate is bitwise the one of k_sor_lex.
//
// Sweep k writes buffer k mod S of a ring of S (its own "new" values) and
// reads the previous sweep's values from buffer (k-1) mod S (sweep 0 from the
// zero field x).  So x_k survives until sweep k+S, and the stopping test of
// sweep k (which needs all of its strips) may be decided after later sweeps
// have started: the first sweep that passes ||x_k - x_{k-1}|| < tol ||x_k||
// sets *stop = k, later sweeps abandon their work, and k_sor_pipe_final
// copies buffer k mod S into x.  A unit (k, half, strip) that would
// overwrite buffer k mod S first waits for sweep k-S's decision.
//
// Units are taken from a ticket counter in dependency order (sweep, then u
// strips, then v strips), by waves of a persistent grid (one wave per CU, the
// configuration of the sc1 hand-off, MI355X_MICROARCH.md "hand-offs" row 1):
// every wait is on a lower ticket, so the launch cannot deadlock.  A unit
// waits (wave-uniform polls of progress stamps = sweep * stride + steps) for
//   - strip s-1 of its own sweep and half (the relaxed row above),
//   - (v half) the u strip of its own rows in its own sweep,
//   - strip s of sweep k-1's v half (old u, v of its rows: the v strip runs
//     behind the u strip, so this covers both) and strip s+1 of sweep k-1's
//     same half (the old row below).
// The stopping test sums the per-strip fp64 partials in the same fixed order
// as k_sor_lex; the last unit of a sweep to finish (an atomic count) decides.
// Every wait is bounded and also ends when *fail or an earlier *stop is seen,
// so the grid always drains.
#define SOR_RING_MAX 32
struct SorPipeArgs {
  const float *coef;  // 7 planes, plane stride ps
  const float2 *b;
  const float2 *x0;   // zero field: the "previous sweep" of sweep 0
  float2 *ring;       // S buffers of H x P float2, stride bstride
  size_t bstride;
  int H, W, P;
  size_t ps;
  int nstrips, S, stride;
  unsigned *ticket;
  int *fail;
  int *stop;          // first sweep whose test passed / hit maxiter (0x7fffffff until then)
  int *cnt;           // [S] finished units per ring slot (monotone)
  int *dec;           // [S] (sweep + 1) * 4 + done code, once decided
  int *prog;          // [S][2][SOR_MAXS] progress stamps
  double *part;       // [S][2 * SOR_MAXS][2] per-strip (dn, xn)
  double *res;        // [S][2] the decided sweep's (dn, xn)
  float omega;
  double tol;
  int maxiter;
};

__device__ __forceinline__ float sor_ld1(const float *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double sor_ldd(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sor_std(double *p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave-uniform wait until *p >= need; false when the unit must be abandoned
// (a later poll of *stop shows an earlier sweep finished the solve, or *fail)
__device__ __forceinline__ bool sorp_wait(const SorPipeArgs &a, const int *p, int need, int &known, int k) {
  for (int n = 0; known < need; ++n) {
    known = __builtin_amdgcn_readfirstlane(sor_poll(p));
    if (known >= need) break;
    if ((n & 31) == 31) {
      const int st = __builtin_amdgcn_readfirstlane(sor_poll(a.stop));
      const int fl = __builtin_amdgcn_readfirstlane(sor_poll(a.fail));
      if (st < k || fl) return false;
    }
    if (n > (1 << 21)) {
      if (threadIdx.x == 0) __hip_atomic_store(a.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

// unit (k, PH, s): strip s of half PH in sweep k; false if abandoned.  The
// relaxation below is k_sor_lex's, operand for operand.
template <int PH>
__device__ __forceinline__ bool sorp_unit(const SorPipeArgs &a, int k, int s, double &dn, double &xn) {
  const int lane = threadIdx.x, H = a.H, W = a.W, P = a.P;
  const int i0 = s * 64, i = i0 + lane;
  const bool rowok = i < H;
  const size_t ps = a.ps;
  const float *wxp = a.coef + (PH ? 2 : 0) * ps, *wyp = a.coef + (PH ? 3 : 1) * ps;
  const float *dgp = a.coef + (PH ? 6 : 4) * ps, *ccp = a.coef + 5 * ps;
  const size_t row = (size_t)(rowok ? i : 0) * P;
  const bool has_up = s > 0, has_dn = i0 + 64 < H;
  const size_t row_up = (size_t)(has_up ? i0 - 1 : 0) * P, row_dn = (size_t)(has_dn ? i0 + 64 : 0) * P;
  const int nsteps = W + 63;
  const int S = a.S, cur = k % S, prv = (k + S - 1) % S;
  float2 *xc = a.ring + (size_t)cur * a.bstride;
  const float2 *xp = k > 0 ? a.ring + (size_t)prv * a.bstride : a.x0;
  const int base = k * a.stride, pbase = (k - 1) * a.stride;
  int *pk = a.prog + cur * 2 * SOR_MAXS;
  const int *pp = a.prog + prv * 2 * SOR_MAXS;
  int *my = pk + PH * SOR_MAXS + s;
  const int *pup = pk + PH * SOR_MAXS + (s > 0 ? s - 1 : 0);
  const int *pu = pk + s;                                       // (k, u, s)
  const int *pold = pp + SOR_MAXS + s;                          // (k-1, v, s)
  const int *pdn = pp + PH * SOR_MAXS + (has_dn ? s + 1 : s);   // (k-1, PH, s+1)
  int known_up = 0, known_u = 0, known_old = 0, known_dn = 0;
  const float om = a.omega, om1 = 1.0f - a.omega;
  bool alive = true;

  float2 X[8], XU[8], XD[8];
  float WX[8], WY[8], DG[8], CC[8], BB[8], WYU[8];
  auto fetch = [&](int t) {  // column t + SOR_D - lane
    const int tp = t + SOR_D, jp = tp - lane, q = tp & 7;
    if (has_up && tp >= 0 && tp < W) alive = alive && sorp_wait(a, pup, base + tp + 64, known_up, k);
    if (PH == 1 && tp >= 0 && tp < nsteps) alive = alive && sorp_wait(a, pu, base + tp + 1, known_u, k);
    if (k > 0 && tp >= 0 && tp < nsteps) alive = alive && sorp_wait(a, pold, pbase + tp + 1, known_old, k);
    if (k > 0 && has_dn && tp - 63 >= 0 && tp - 63 < W)
      alive = alive && sorp_wait(a, pdn, pbase + tp - 62, known_dn, k);
    const bool ok = rowok && jp >= 0 && jp < W;
    const size_t o = row + (ok ? jp : 0);
    if (PH == 0) X[q] = ok ? sor_ld(xp + o) : make_float2(0.f, 0.f);
    else X[q] = ok ? make_float2(sor_ld1((const float *)(xc + o)), sor_ld1((const float *)(xp + o) + 1))
                   : make_float2(0.f, 0.f);
    WX[q] = ok && jp + 1 < W ? wxp[o] : 0.f;
    WY[q] = ok && i + 1 < H ? wyp[o] : 0.f;
    DG[q] = ok ? sor_dg(dgp[o]) : 0.f;
    CC[q] = ok ? ccp[o] : 0.f;
    BB[q] = ok ? (PH ? a.b[o].y : a.b[o].x) : 0.f;
    if (lane == 0) {
      const bool u = has_up && jp >= 0 && jp < W;
      XU[q] = u ? sor_ld(xc + row_up + jp) : make_float2(0.f, 0.f);
      WYU[q] = u ? wyp[row_up + jp] : 0.f;
    }
    if (lane == 63) {
      const bool d = has_dn && jp >= 0 && jp < W;
      XD[q] = d ? sor_ld(xp + row_dn + jp) : make_float2(0.f, 0.f);
    }
  };
#pragma unroll
  for (int t = -SOR_D; t < 0; ++t) fetch(t);
  if (!alive) return false;

  int stop_seen = 0x7fffffff;
  float res = 0.f, wx_prev = 0.f, wy_prev = 0.f;
  for (int t0 = 0; t0 < nsteps; t0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u;
      if (t >= nsteps) break;
      fetch(t);
      const int j = t - lane, q = t & 7, q1 = (t + 1) & 7;
      const bool act = rowok && j >= 0 && j < W;
      const float2 xo = X[q];
      const float old = PH ? xo.y : xo.x, other = PH ? xo.x : xo.y;
      const float right = PH ? X[q1].y : X[q1].x;
      float down = wave_from_next(right);
      if (lane == 63) down = PH ? XD[q].y : XD[q].x;
      float up = wave_from_prev(res), wu = wave_from_prev(wy_prev);
      if (lane == 0) {
        up = PH ? XU[q].y : XU[q].x;
        wu = WYU[q];
      }
      float nw = sor_relax(BB[q], wx_prev, res, WX[q], right, WY[q], down, wu, up, CC[q], other, DG[q], old, om, om1);
      if (act) {
        const size_t o = row + j;
        sor_st(xc + o, PH ? make_float2(other, nw) : make_float2(nw, other));
        sor_acc(nw, old, dn, xn);
      } else {
        nw = 0.f;
      }
      res = nw;
      wx_prev = act ? WX[q] : 0.f;
      wy_prev = act ? WY[q] : 0.f;
      if (((t + 1) & (SOR_G - 1)) == 0 || t + 1 == nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(my, base + t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // *stop as read at the previous publication (its load had a whole
        // publication interval to return): abandon a sweep past the answer
        if (stop_seen < k || !alive) return false;
        stop_seen = __builtin_amdgcn_readfirstlane(sor_poll(a.stop));
      }
    }
  }
  return alive;
}

__global__ __launch_bounds__(64) void k_sor_pipe(SorPipeArgs a) {
  const int lane = threadIdx.x, n2 = 2 * a.nstrips;
  for (;;) {
    int tk = 0;
    if (lane == 0) tk = (int)atomicAdd(a.ticket, 1u);
    tk = __builtin_amdgcn_readfirstlane(__shfl(tk, 0, 64));
    const int k = tk / n2, r = tk - k * n2;
    if (k >= a.maxiter) return;
    if (__builtin_amdgcn_readfirstlane(sor_poll(a.stop)) < k || __builtin_amdgcn_readfirstlane(sor_poll(a.fail)))
      return;
    const int cur = k % a.S;
    if (k >= a.S) {
      // ring slot `cur` still holds sweep k - S: wait for its decision; if it
      // ended the solve, this and every later unit is void
      int known = 0;
      const int need = (k - a.S + 1) * 4;
      if (!sorp_wait(a, a.dec + cur, need, known, k)) return;
      if (known & 3) return;
    }
    const int ph = r >= a.nstrips ? 1 : 0, s = ph ? r - a.nstrips : r;
    double dn = 0.0, xn = 0.0;
    const bool ok = ph ? sorp_unit<1>(a, k, s, dn, xn) : sorp_unit<0>(a, k, s, dn, xn);
    if (!ok) continue;  // abandoned: the next ticket sees *stop / *fail and ends the wave
    dn = wave_sum(dn);
    xn = wave_sum(xn);
    if (lane == 0) {
      double *pt = a.part + ((size_t)cur * 2 * SOR_MAXS + r) * 2;  // fixed slot per strip, as k_sor_lex
      sor_std(pt, dn);
      sor_std(pt + 1, xn);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int c = atomicAdd(a.cnt + cur, 1) + 1;
      if (c == (k / a.S + 1) * n2) {
        // the last unit of sweep k: its stopping test (k_sor_lex's prologue)
        double sd = 0.0, sx = 0.0;
        for (int b = 0; b < n2; ++b) {
          const double *q = a.part + ((size_t)cur * 2 * SOR_MAXS + b) * 2;
          sd += sor_ldd(q);
          sx += sor_ldd(q + 1);
        }
        const int done = sqrt(sd) < a.tol * sqrt(sx) ? 1 : (k + 1 >= a.maxiter ? 2 : 0);
        sor_std(a.res + 2 * cur, sd);
        sor_std(a.res + 2 * cur + 1, sx);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(a.dec + cur, (k + 1) * 4 + done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done) atomicMin(a.stop, k);
      }
    }
  }
}

// after k_sor_pipe: x <- the decided sweep's buffer; the state as k_sor_final
// records it (iter = sweeps done, rr = ||dx||^2, xnorm2 = ||x||^2)
__global__ __launch_bounds__(256) void k_sor_pipe_final(SorPipeArgs a, float2 *x, PcgState *st) {
  const int K = *a.stop;
  if (K == 0x7fffffff || *a.fail) return;
  const int cur = K % a.S;
  const float2 *src = a.ring + (size_t)cur * a.bstride;
  OF_FOR_PIXELS(a.H, a.W) {
    if (j >= a.W) continue;
    const size_t o = (size_t)i * a.P + j;
    x[o] = src[o];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    st->iter = K + 1;
    st->rr = a.res[2 * cur];
    st->xnorm2 = a.res[2 * cur + 1];
    st->done = a.dec[cur] & 3;
  }
}

// ---------------------------------------------------------------------------
// k_sor_wg: the pipelined lexicographic SOR of a small level (<= 64 rows: one
// strip per half) in ONE workgroup, with the sweep ring and the progress
// stamps in LDS.  Same schedule as k_sor_pipe -- unit (sweep k, half) relaxes
// the anti-diagonals of the strip, sweep k+1 trails sweep k, sweep k writes
// ring slot k mod S and reads slot k-1 mod S, a slot is reused only after the
// decision of the sweep that held it -- and the same relaxation operand for
// operand (sor_relax), so the iterate and the sweep count are k_sor_lex's
// bitwise.  What changes is the hand-off: in k_sor_pipe every unit is a wave
// somewhere on the chip, and a sweep's rows reach the next sweep through L2
// (sc1 stores, a stamp every SOR_G steps after s_waitcnt vmcnt(0), polled with
// sc1 loads): ~1 us per hand-off, so at 30x40 a sweep costs ~27 us for ~70
// relaxation steps.  Here the waves share one CU's LDS: a stamp is a ds_write
// and a poll a ds_read.
//
// Units are static: wave w takes tickets w, w + nw, ... in order (ticket 2k =
// (k, u), 2k + 1 = (k, v)); every wait is on a lower ticket (the u unit of
// its sweep, the v unit of the previous sweep, the decision of sweep k - S),
// and all waves of a workgroup are resident, so the lowest unfinished ticket
// can always proceed: no deadlock.  Waits are bounded (fail) and end on an
// earlier decision (stop), so every wave reaches the final barrier.
// waves per workgroup: 8 (2 per SIMD) keep the unit's prefetch ring and both
// halves' code in registers (a 16-wave build has 128 VGPRs and spills)
#define SORW_MAXW 8
struct SorWgArgs {
  const float *coef;  // 7 planes, plane stride ps
  const float2 *b;
  float2 *x;          // the solution (pitched), written from the decided slot
  int H, W, P;
  size_t ps;
  int S, nw;          // ring depth, waves
  float omega;
  double tol;
  int maxiter;
  PcgState *st;
  int *fail;          // global: set when a wait gave up (the host reruns per sweep)
};
struct SorWgShared {  // LDS after the ring
  int prog[SORW_MAXW + 2][2];  // [slot][half] progress stamps (sweep * stride + steps)
  int dec[SORW_MAXW + 2];      // (sweep + 1) * 4 + done code, once decided
  int cnt[SORW_MAXW + 2];      // finished units per slot (monotone)
  double part[SORW_MAXW + 2][2][2];
  double res[SORW_MAXW + 2][2];
  int stop, fail;
};
// LDS stamps without acquire / release: at workgroup scope those also wait
// for the wave's outstanding global loads (s_waitcnt vmcnt(0)), i.e. for the
// coefficient prefetch SOR_D steps ahead, every step (1.5 us per step
// measured), and so does an inline-asm wait with a memory clobber.  Not
// needed: the LDS executes a CU's DS instructions in order, so a unit's data
// ds_writes land before its later stamp ds_write, and a reader's data
// ds_reads (issued after the stamp value they depend on returned) see them.
// Only the compiler must keep LDS accesses on their side of a stamp access:
// signal fences (no instruction).
__device__ __forceinline__ int sorw_ld(const int *p) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  return v;
}
__device__ __forceinline__ void sorw_st(int *p, int v) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// wave-uniform wait until *p >= need; false when abandoned (an earlier sweep
// decided, or a wait gave up)
__device__ __forceinline__ bool sorw_wait(SorWgShared &sh, const int *p, int need, int &known, int k) {
  for (int n = 0; known < need; ++n) {
    known = __builtin_amdgcn_readfirstlane(sorw_ld(p));
    if (known >= need) break;
    if ((n & 15) == 15 &&
        (__builtin_amdgcn_readfirstlane(sorw_ld(&sh.stop)) < k || __builtin_amdgcn_readfirstlane(sorw_ld(&sh.fail))))
      return false;
    if (n > (1 << 22)) {
      if ((threadIdx.x & 63) == 0) sorw_st(&sh.fail, 1);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

// the dynamic LDS of k_sor_wg: [S][H][W] float2 sweep ring, then
// SorWgShared, addressed from the symbol (LDS instructions, not flat ones:
// a flat access counts in both vmcnt and lgkmcnt, so waiting for it would
// also wait for the global coefficient prefetch)
extern __shared__ double sorw_lds[];
__device__ __forceinline__ float2 *sorw_ring() { return reinterpret_cast<float2 *>(sorw_lds); }
__device__ __forceinline__ SorWgShared &sorw_sh(const SorWgArgs &a) {
  return *reinterpret_cast<SorWgShared *>(sorw_ring() + (size_t)a.S * a.H * a.W);
}

template <int PH>
__device__ __forceinline__ bool sorw_unit(const SorWgArgs &a, int k, int stride, double &dn, double &xn) {
  float2 *ring = sorw_ring();
  SorWgShared &sh = sorw_sh(a);
  const int lane = threadIdx.x & 63, H = a.H, W = a.W;
  const bool rowok = lane < H;
  const size_t ps = a.ps;
  // global (not generic) pointers: global_load, counted in vmcnt only
  typedef const __attribute__((address_space(1))) float gf;
  gf *cf = (gf *)a.coef;
  gf *bp = (gf *)a.b + PH;  // b's component of this half (float2 planes)
  gf *wxp = cf + (PH ? 2 : 0) * ps, *wyp = cf + (PH ? 3 : 1) * ps;
  gf *dgp = cf + (PH ? 6 : 4) * ps, *ccp = cf + 5 * ps;
  const size_t row = (size_t)(rowok ? lane : 0) * a.P;
  const int lrow = (rowok ? lane : 0) * W;
  const int nsteps = W + H - 1;  // lane H - 1 relaxes column W - 1 at step W + H - 2
  const int S = a.S, cur = k % S, prv = (k + S - 1) % S;
  float *xc = reinterpret_cast<float *>(ring + (size_t)cur * H * W);
  const float2 *xp = ring + (size_t)prv * H * W;
  const int base = k * stride, pbase = (k - 1) * stride;
  int *my = &sh.prog[cur][PH];
  const int *pu = &sh.prog[cur][0];    // (k, u)
  const int *pold = &sh.prog[prv][1];  // (k - 1, v)
  int known_u = 0, known_old = 0;
  const float om = a.omega, om1 = 1.0f - a.omega;

  // coefficients of column t + SOR_D - lane, SOR_D steps ahead (global, L2)
  float WX[8], WY[8], DG[8], CC[8], BB[8];
  // every load unconditional at a clamped address, the value selected after
  // it: loads under a branch make the compiler wait for all of them
  // (vmcnt(0)) at every step instead of for the one SOR_D steps old
  // The raw values go into the ring and are masked at the step that uses
  // them (+0 where the reference has no entry), by an AND the compiler cannot
  // see through: a mask or select it can see becomes a masked load, whose
  // value is then waited for at once (vmcnt(0)) instead of SOR_D steps later
  auto keep = [](float v, bool c) {
    float r;
    asm("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(0u - (unsigned)c));
    return r;
  };
  auto fetch = [&](int t) {
    const int tp = t + SOR_D, jp = tp - lane, q = tp & 7;
    const size_t o = row + min(max(jp, 0), W - 1);
    WX[q] = wxp[o];
    WY[q] = wyp[o];
    DG[q] = dgp[o];
    CC[q] = ccp[o];
    BB[q] = bp[2 * o];
  };
  // the old (and, for v, this sweep's u) values of column jn of this lane's row
  auto xval = [&](int jn) {
    const bool ok = rowok && jn >= 0 && jn < W;
    const int e = lrow + min(max(jn, 0), W - 1);
    const float2 o = xp[e];
    const float u = PH ? xc[2 * e] : o.x;
    return make_float2(keep(u, ok && (PH || k > 0)), keep(o.y, ok && k > 0));
  };
#pragma unroll
  for (int t = -SOR_D; t < 0; ++t) fetch(t);
  // The waits of a group of 8 steps at once, before the group (a wait in
  // every step made each step ~650 instructions of control flow): step t
  // reads column t + 1 - lane, relaxed by (k-1, v) and (v half) by (k, u) at
  // their step t + 1, so the group [t0, t0 + 7] needs their progress t0 + 9.
  bool alive = true;
  auto group_wait = [&](int t0) {
    const int need = min(t0 + 9, nsteps);
    if (k > 0) alive = alive && sorw_wait(sh, pold, pbase + need, known_old, k);
    if (PH == 1) alive = alive && sorw_wait(sh, pu, base + need, known_u, k);
  };
  group_wait(0);
  if (!alive) return false;
  float2 Xq = xval(-lane);
  float res = 0.f, wx_prev = 0.f, wy_prev = 0.f;
  // whole groups: the steps past nsteps relax nothing (every lane's column
  // is past W) and store nothing
  for (int t0 = 0; t0 < nsteps; t0 += 8) {
    group_wait(t0);
    if (!alive) return false;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u;
      fetch(t);
      const float2 Xn = xval(t + 1 - lane);
      const int j = t - lane, q = t & 7;
      const bool act = rowok && j >= 0 && j < W;
      const float wxq = keep(WX[q], act && j + 1 < W), wyq = keep(WY[q], act && lane + 1 < H);
      const float dgq = keep(sor_dg(DG[q]), act), ccq = keep(CC[q], act), bbq = keep(BB[q], act);
      const float old = PH ? Xq.y : Xq.x, other = PH ? Xq.x : Xq.y;
      const float right = PH ? Xn.y : Xn.x;
      float down = wave_from_next(right);
      float up = wave_from_prev(res), wu = wave_from_prev(wy_prev);
      if (lane == 0) {  // no strip above
        up = 0.f;
        wu = 0.f;
      }
      float nw = sor_relax(bbq, wx_prev, res, wxq, right, wyq, down, wu, up, ccq, other, dgq, old, om, om1);
      if (act) {
        xc[2 * (lrow + j) + PH] = nw;
        sor_acc(nw, old, dn, xn);
      } else {
        nw = 0.f;
      }
      res = nw;
      wx_prev = wxq;
      wy_prev = wyq;
      Xq = Xn;
    }
    if (lane == 0) sorw_st(my, base + min(t0 + 8, nsteps));
  }
  return alive;
}

__global__ __launch_bounds__(SORW_MAXW * 64) void k_sor_wg(SorWgArgs a) {
  float2 *ring = sorw_ring();
  SorWgShared &sh = sorw_sh(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int stride = a.W + a.H + 1;  // > steps of a unit
  if (threadIdx.x < SORW_MAXW + 2) {
    sh.prog[threadIdx.x][0] = sh.prog[threadIdx.x][1] = -1;
    sh.dec[threadIdx.x] = 0;
    sh.cnt[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) {
    sh.stop = 0x7fffffff;
    sh.fail = 0;
  }
  __syncthreads();
  if (wave < a.nw) {
    for (int tk = wave;; tk += a.nw) {
      const int k = tk >> 1, ph = tk & 1;
      if (k >= a.maxiter) break;
      if (__builtin_amdgcn_readfirstlane(sorw_ld(&sh.stop)) < k || __builtin_amdgcn_readfirstlane(sorw_ld(&sh.fail)))
        break;
      const int cur = k % a.S;
      if (k >= a.S) {
        // slot `cur` still holds sweep k - S: wait for its decision; if it
        // ended the solve, this and every later unit is void
        int known = 0;
        if (!sorw_wait(sh, &sh.dec[cur], (k - a.S + 1) * 4, known, k)) break;
        if (known & 3) break;
      }
      double dn = 0.0, xn = 0.0;
      const bool ok = ph ? sorw_unit<1>(a, k, stride, dn, xn) : sorw_unit<0>(a, k, stride, dn, xn);
      if (!ok) break;
      dn = wave_sum(dn);
      xn = wave_sum(xn);
      if (lane == 0) {
        sh.part[cur][ph][0] = dn;
        sh.part[cur][ph][1] = xn;
        const int c = __hip_atomic_fetch_add(&sh.cnt[cur], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) + 1;
        if (c == (k / a.S + 1) * 2) {
          // the last unit of sweep k: its stopping test, k_sor_lex's order
          double sd = 0.0, sx = 0.0;
          for (int b = 0; b < 2; ++b) {
            sd += sh.part[cur][b][0];
            sx += sh.part[cur][b][1];
          }
          const int done = sqrt(sd) < a.tol * sqrt(sx) ? 1 : (k + 1 >= a.maxiter ? 2 : 0);
          sh.res[cur][0] = sd;
          sh.res[cur][1] = sx;
          if (done) __hip_atomic_fetch_min(&sh.stop, k, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
          sorw_st(&sh.dec[cur], (k + 1) * 4 + done);
        }
      }
    }
  }
  __syncthreads();
  const int K = sh.stop;
  if (sh.fail || K == 0x7fffffff) {
    if (threadIdx.x == 0) __hip_atomic_store(a.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int cur = K % a.S;
  const float2 *src = ring + (size_t)cur * a.H * a.W;
  for (int e = threadIdx.x; e < a.H * a.W; e += blockDim.x) {
    const int i = e / a.W, j = e - i * a.W;
    a.x[(size_t)i * a.P + j] = src[e];
  }
  if (threadIdx.x == 0) {
    a.st->iter = K + 1;
    a.st->rr = sh.res[cur][0];
    a.st->xnorm2 = sh.res[cur][1];
    a.st->done = sh.dec[cur] & 3;
  }
}
