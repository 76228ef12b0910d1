// kernels_screen.hip — the screened Poisson solver behind the blind temporal
// consistency (include/optflow.h, "Blind temporal consistency"): the multilevel
// schedule of kernels_poisson.hip over the whole frame, every cell's integer
// diagonal d joined by a real screening term q >= 0.  The finest level's
// operator, screening plane, right-hand side and start from the processed
// frame and either given anchor and weight planes or the previous output
// warped along the flow under the fusion's weight (k_scr_setup), the coarser
// levels' screening planes (k_scr_coarsen_q; their d and wt are
// k_psn_coarsen's), red-black Gauss-Seidel on an LDS tile with halo, the
// channels one after the other over one LDS plane (k_scr_smooth), the
// residual's restriction (k_scr_restrict), the coarsest level relaxed in one
// workgroup per channel (k_scr_coarsest) and the result's way back into a
// frame (k_scr_store).  The correction is k_psn_prolong's.  Every step is
// elementwise; all arithmetic in fp64 with no contraction, in the order the
// header states, so a numpy float64 restatement gives the same bits.
//
// Levels and windows as in kernels_poisson.hip; here a level's window is its
// whole grid plus an apron of the coarsest level's one cell on every side.
// Per cell of the window: d and wt as there (0 outside the frame), q the
// screening term (0.0 outside the frame); a cell is solved for where
// (double)d + q > 0.  Expects kernels_sample.hip and kernels_poisson.hip
// before it.
#include "kernels.h"

#define SCR_R (PSN_T + 4 * PSN_MAX_SWEEPS)

// The finest level from the frame-sized planes.  P: the target, H x W x CT
// interleaved fp32.  With F == nullptr the anchor A (H x W x CT interleaved
// fp64) and the screening plane Q (H x W fp64) are given; otherwise F is the
// pitched flow to the previous frame, S its state (dense bytes or nullptr), wgt
// the fusion's weight of the previous frame (H x W fp32) and O the previous
// output (H x W x CT fp32): where the flow is finite, lands inside the frame
// and S is 0 (fuse_sample's rule), q = lambda * (double)wgt and the anchor is
// O's bilinear sample where the flow lands; elsewhere both are 0.0.  One thread
// per cell of the window.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_scr_setup(const float *__restrict__ P, const double *__restrict__ A, const double *__restrict__ Q,
            const float *__restrict__ wgt, double lambda, const float2 *__restrict__ F, int FP,
            const uint8_t *__restrict__ S, const float *__restrict__ O, int H, int W, PsnWin win,
            int *__restrict__ d, ushort4 *__restrict__ wt, double *__restrict__ q, double *__restrict__ b,
            double *__restrict__ x) {
  OF_NOCONTRACT
  const size_t plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const int gi = win.r0 + i, gj = win.c0 + j;
    const size_t o = (size_t)i * win.w + j;
    if (!(gi >= 0 && gi < H && gj >= 0 && gj < W)) {
      d[o] = 0;
      wt[o] = make_ushort4(0, 0, 0, 0);
      q[o] = 0.0;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        b[c * plane + o] = 0.0;
        x[c * plane + o] = 0.0;
      }
      continue;
    }
    const size_t go = (size_t)gi * W + gj;
    const bool up = gi > 0, down = gi < H - 1, left = gj > 0, right = gj < W - 1;
    d[o] = (int)up + (int)down + (int)left + (int)right;
    wt[o] = make_ushort4(up, down, left, right);
    double qq = 0.0, a[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a[c] = 0.0;
    if (F) {
      const float2 g = F[(size_t)gi * FP + gj];
      const double r = (double)gi + (double)g.y, s = (double)gj + (double)g.x;
      if (__builtin_isfinite(g.x) && __builtin_isfinite(g.y) && in_frame(r, s, H, W) && !(S && S[go] != 0)) {
        qq = lambda * (double)wgt[go];
        const BilTap t = bil_tap(r, s, H, W);
#pragma unroll
        for (int c = 0; c < CT; ++c) a[c] = bil_at(O, CT, c, t);
      }
    } else {
      qq = Q[go];
#pragma unroll
      for (int c = 0; c < CT; ++c) a[c] = A[go * CT + c];
    }
    q[o] = qq;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const double pc = (double)P[go * CT + c];
      double g = 0.0;
      if (up) g = g + (pc - (double)P[(go - W) * CT + c]);
      if (down) g = g + (pc - (double)P[(go + W) * CT + c]);
      if (left) g = g + (pc - (double)P[(go - 1) * CT + c]);
      if (right) g = g + (pc - (double)P[(go + 1) * CT + c]);
      b[c * plane + o] = g + qq * a[c];
      x[c * plane + o] = pc;
    }
  }
}

// The next level's screening plane, the Galerkin term of piecewise-constant
// transfer: ((q(c00) + q(c01)) + q(c10)) + q(c11) of the four children (a
// child outside the frame holds 0.0).  fw: the fine window's width; one thread
// per coarse cell.
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_scr_coarsen_q(const double *__restrict__ fq, int fw, PsnWin win, double *__restrict__ q) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const size_t o00 = (size_t)(2 * i) * fw + 2 * j;
    q[(size_t)i * win.w + j] = ((fq[o00] + fq[o00 + 1]) + fq[o00 + fw]) + fq[o00 + fw + 1];
  }
}

// `sweeps` red-black Gauss-Seidel sweeps of one level, xin -> xout, as
// k_psn_smooth (same tile, halo and colour order) with the real diagonal: a
// solved cell becomes (b + wt_n x_n over the coupled neighbours up, down,
// left, right) / ((double)d + q).  The tile's wt and (double)d + q, formed
// here once, go to LDS once per workgroup; the channels then take turns on
// one LDS plane of x, so the footprint (38400 B) does not depend on CT.
template <int CT>
__global__ void __launch_bounds__(PSN_THREADS)
k_scr_smooth(const int *__restrict__ d, const ushort4 *__restrict__ wt, const double *__restrict__ q,
             const double *__restrict__ b, const double *__restrict__ xin, double *__restrict__ xout, PsnWin win,
             int gx, int sweeps) {
  OF_NOCONTRACT
  __shared__ double s_x[SCR_R * SCR_R];
  __shared__ double s_g[SCR_R * SCR_R];
  __shared__ ushort4 s_w[SCR_R * SCR_R];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int halo = 2 * sweeps, R = PSN_T + 2 * halo;
  const int i0 = tyi * PSN_T - halo, j0 = txi * PSN_T - halo;  // the region's origin in the window
  const size_t plane = (size_t)win.h * win.w;
  const int tid = threadIdx.x;
  for (int e = tid; e < R * R; e += PSN_THREADS) {
    const int ly = e / R, lx = e - ly * R;
    const int i = i0 + ly, j = j0 + lx;
    const bool in = i >= 0 && i < win.h && j >= 0 && j < win.w;
    const size_t o = in ? (size_t)i * win.w + j : 0;
    s_g[e] = in ? (double)d[o] + q[o] : 0.0;
    s_w[e] = in ? wt[o] : make_ushort4(0, 0, 0, 0);
  }
  const int half = R / 2;  // R is even: cells of one colour per row
  for (int c = 0; c < CT; ++c) {
    const double *__restrict__ xc = xin + c * plane;
    const double *__restrict__ bc = b + c * plane;
    for (int e = tid; e < R * R; e += PSN_THREADS) {
      const int ly = e / R, lx = e - ly * R;
      const int i = i0 + ly, j = j0 + lx;
      const bool in = i >= 0 && i < win.h && j >= 0 && j < win.w;
      s_x[e] = in ? xc[(size_t)i * win.w + j] : 0.0;
    }
    __syncthreads();
    for (int pass = 0; pass < 2 * sweeps; ++pass) {
      const int k = pass & 1;
      for (int e = tid; e < (R - 2) * half; e += PSN_THREADS) {
        const int ly = 1 + e / half, m = e - (ly - 1) * half;
        // the columns of row ly with (window row + r0 + window column + c0) & 1 == k
        const int lx = 2 * m + ((win.r0 + i0 + ly + win.c0 + j0 + k) & 1);
        if (lx < 1 || lx > R - 2) continue;
        const int p = ly * R + lx;
        const double dg = s_g[p];
        if (!(dg > 0.0)) continue;
        const ushort4 wq = s_w[p];
        double t = bc[(size_t)(i0 + ly) * win.w + (j0 + lx)];  // a solved cell lies inside the window
        if (wq.x) t = t + (double)wq.x * s_x[p - R];
        if (wq.y) t = t + (double)wq.y * s_x[p + R];
        if (wq.z) t = t + (double)wq.z * s_x[p - 1];
        if (wq.w) t = t + (double)wq.w * s_x[p + 1];
        s_x[p] = t / dg;
      }
      __syncthreads();
    }
    double *__restrict__ yc = xout + c * plane;
    for (int e = tid; e < PSN_T * PSN_T; e += PSN_THREADS) {
      const int ty = e / PSN_T, tx = e - ty * PSN_T;
      const int i = i0 + halo + ty, j = j0 + halo + tx;
      if (i >= win.h || j >= win.w) continue;
      yc[(size_t)i * win.w + j] = s_x[(halo + ty) * R + halo + tx];
    }
    __syncthreads();  // the next channel overwrites s_x
  }
}

// the residual b - ((double)d + q) x + wt_n x_n (neighbours up, down, left,
// right) of cell o of a level, 0 where it is not solved for
template <int CT>
__device__ __forceinline__ void scr_residual(const int *__restrict__ d, const ushort4 *__restrict__ wt,
                                             const double *__restrict__ q, const double *__restrict__ b,
                                             const double *__restrict__ x, size_t plane, int w, size_t o,
                                             double r[CT]) {
  OF_NOCONTRACT
  const double dg = (double)d[o] + q[o];
  const ushort4 wq = wt[o];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    double t = 0.0;
    if (dg > 0.0) {
      const double *__restrict__ xc = x + c * plane;
      t = b[c * plane + o] - dg * xc[o];
      if (wq.x) t = t + (double)wq.x * xc[o - w];
      if (wq.y) t = t + (double)wq.y * xc[o + w];
      if (wq.z) t = t + (double)wq.z * xc[o - 1];
      if (wq.w) t = t + (double)wq.w * xc[o + 1];
    }
    r[c] = t;
  }
}

// The coarse right-hand side: ((res(c00) + res(c01)) + res(c10)) + res(c11) of
// the four children on the solved coarse cells ((double)d + q > 0), 0 on the
// others; the coarse unknown starts from 0.  fd .. fx: the fine level; one
// thread per coarse cell.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_scr_restrict(const int *__restrict__ fd, const ushort4 *__restrict__ fwt, const double *__restrict__ fq,
               const double *__restrict__ fb, const double *__restrict__ fx, int fh, int fw,
               const int *__restrict__ d, const double *__restrict__ q, PsnWin win, double *__restrict__ b,
               double *__restrict__ x) {
  OF_NOCONTRACT
  const size_t fplane = (size_t)fh * fw, plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const size_t o = (size_t)i * win.w + j;
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    if ((double)d[o] + q[o] > 0.0) {
      const size_t o00 = (size_t)(2 * i) * fw + 2 * j;
      double r[CT];
      scr_residual<CT>(fd, fwt, fq, fb, fx, fplane, fw, o00, acc);
      scr_residual<CT>(fd, fwt, fq, fb, fx, fplane, fw, o00 + 1, r);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = acc[c] + r[c];
      scr_residual<CT>(fd, fwt, fq, fb, fx, fplane, fw, o00 + fw, r);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = acc[c] + r[c];
      scr_residual<CT>(fd, fwt, fq, fb, fx, fplane, fw, o00 + fw + 1, r);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = acc[c] + r[c];
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      b[c * plane + o] = acc[c];
      x[c * plane + o] = 0.0;
    }
  }
}

// The coarsest level, at most PSN_CMAX cells, relaxed `sweeps` times in LDS in
// place: one workgroup per channel (blockIdx.x), the same red-black sweep as
// k_scr_smooth.
__global__ void __launch_bounds__(PSN_THREADS)
k_scr_coarsest(const int *__restrict__ d, const ushort4 *__restrict__ wt, const double *__restrict__ q,
               const double *__restrict__ b, double *__restrict__ x, PsnWin win, int sweeps) {
  OF_NOCONTRACT
  __shared__ double s_x[PSN_CMAX], s_b[PSN_CMAX], s_g[PSN_CMAX];
  __shared__ ushort4 s_w[PSN_CMAX];
  const int n = win.h * win.w, tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  for (int e = tid; e < n; e += PSN_THREADS) {
    s_x[e] = x[base + e];
    s_b[e] = b[base + e];
    s_g[e] = (double)d[e] + q[e];
    s_w[e] = wt[e];
  }
  __syncthreads();
  for (int pass = 0; pass < 2 * sweeps; ++pass) {
    const int k = pass & 1;
    for (int e = tid; e < n; e += PSN_THREADS) {
      const int i = e / win.w, j = e - i * win.w;
      const double dg = s_g[e];
      if (!(dg > 0.0) || ((win.r0 + i + win.c0 + j) & 1) != k) continue;
      const ushort4 wq = s_w[e];
      double t = s_b[e];
      if (wq.x) t = t + (double)wq.x * s_x[e - win.w];
      if (wq.y) t = t + (double)wq.y * s_x[e + win.w];
      if (wq.z) t = t + (double)wq.z * s_x[e - 1];
      if (wq.w) t = t + (double)wq.w * s_x[e + 1];
      s_x[e] = t / dg;
    }
    __syncthreads();
  }
  for (int e = tid; e < n; e += PSN_THREADS) x[base + e] = s_x[e];
}

// The result as a frame, H x W x CT interleaved: (float)x into outf and x into
// outd, whichever is not nullptr (the window covers the frame).  One thread
// per pixel.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_scr_store(const double *__restrict__ x, PsnWin win, int H, int W, float *__restrict__ outf,
            double *__restrict__ outd) {
  const size_t plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t go = (size_t)i * W + j;
    const size_t o = (size_t)(i - win.r0) * win.w + (j - win.c0);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const double v = x[c * plane + o];
      if (outf) outf[go * CT + c] = (float)v;
      if (outd) outd[go * CT + c] = v;
    }
  }
}
