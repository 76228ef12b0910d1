// kernels_poisson.hip — the multilevel Poisson solver behind the blended
// inpainting fill (include/optflow.h, "Gradient-domain blending"): the finest
// level's operator and right-hand side from the label, value and source planes
// (k_psn_setup), the Galerkin operators of the coarser levels (k_psn_coarsen),
// red-black Gauss-Seidel on an LDS tile with halo (k_psn_smooth), the
// residual's restriction (k_psn_restrict), the scaled piecewise-constant
// correction (k_psn_prolong), the coarsest level relaxed in one workgroup per
// channel (k_psn_coarsest) and the results' way back into frames
// (k_psn_store, k_blend_labels, k_blend_store).  Every step is elementwise: no
// reductions, no data-dependent stopping, so the schedule depends on the frame
// size and the options alone.  All arithmetic in fp64 with no contraction, in
// the order the header states, so a numpy float64 restatement gives the same
// bits.
//
// A level works on a window of its grid, the grid anchored at the frame's
// origin (cell (I, J) of level l+1 covers cells 2I, 2I+1 x 2J, 2J+1 of level
// l): rows r0 .. r0 + h - 1, columns c0 .. c0 + w - 1, the windows nested (h,
// w, r0, c0 double from level to level) and at least one cell wider than the
// cells that are solved for on every side, so a solved cell's neighbours are
// always inside the window.  Per cell of the window: d, the diagonal (0: not
// solved for), wt, the weights of the neighbours up, down, left, right (0: no
// coupling), x and b planar, C planes of h x w doubles.
#include "kernels.h"

#define PSN_FIXED 0
#define PSN_UNKNOWN 1
#define PSN_EXCLUDED 2
#define PSN_MAX_C 4
#define PSN_CMAX 1024        // cells of the coarsest window at most
#define PSN_OMEGA 1.5        // the coarse correction's factor
#define PSN_T 32             // k_psn_smooth's tile: 32 x 32 cells
#define PSN_MAX_SWEEPS 2     // ... relaxed up to twice per launch: a halo of 2 cells per sweep
#define PSN_R (PSN_T + 4 * PSN_MAX_SWEEPS)
#define PSN_THREADS 256

struct PsnWin {  // a level's window
  int r0, c0, h, w;
};

// the label of pixel (i, j), positions outside the frame counting as excluded
__device__ __forceinline__ int psn_label(const uint8_t *__restrict__ lab, int i, int j, int H, int W) {
  return (i >= 0 && i < H && j >= 0 && j < W) ? (int)lab[(size_t)i * W + j] : PSN_EXCLUDED;
}

// The finest level from the frame-sized planes: lab H x W bytes, vf H x W x C
// interleaved fp32 (the fixed pixels' values, the unknown ones' start), s
// likewise and hs H x W bytes (the guidance) or both nullptr; vu, like vf, the
// unknown pixels' start where it is not vf's (or nullptr).  With `keep` the
// window's x is a previous solve's and stays where the pixel is not unknown
// (the fixed values are then read from it).  One thread per cell of the window.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_psn_setup(const uint8_t *__restrict__ lab, const float *__restrict__ vf, const float *__restrict__ vu,
            const float *__restrict__ s,
            const uint8_t *__restrict__ hs, int H, int W, PsnWin win, int keep, int *__restrict__ d,
            ushort4 *__restrict__ wt, double *x, double *__restrict__ b) {
  OF_NOCONTRACT
  const size_t plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const int gi = win.r0 + i, gj = win.c0 + j;
    const size_t o = (size_t)i * win.w + j;
    const int l = psn_label(lab, gi, gj, H, W);
    const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W;
    const size_t go = in ? (size_t)gi * W + gj : 0;
    // neighbours up, down, left, right
    const int ni[4] = {gi - 1, gi + 1, gi, gi}, nj[4] = {gj, gj, gj - 1, gj + 1};
    const int no[4] = {-win.w, win.w, -1, 1};
    int ln[4] = {PSN_EXCLUDED, PSN_EXCLUDED, PSN_EXCLUDED, PSN_EXCLUDED};
    int deg = 0;
    if (l == PSN_UNKNOWN) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ln[k] = psn_label(lab, ni[k], nj[k], H, W);
        deg += ln[k] != PSN_EXCLUDED;
      }
    }
    const bool solved = l == PSN_UNKNOWN && deg > 0;
    d[o] = solved ? deg : 0;
    // an unknown neighbour of a solved cell has this cell as a neighbour that is not excluded: it is solved too
    wt[o] = solved ? make_ushort4(ln[0] == PSN_UNKNOWN, ln[1] == PSN_UNKNOWN, ln[2] == PSN_UNKNOWN, ln[3] == PSN_UNKNOWN)
                   : make_ushort4(0, 0, 0, 0);
    const bool hp = solved && s && hs[go] != 0;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (!keep || l == PSN_UNKNOWN)
        x[c * plane + o] = in ? (double)((vu && l == PSN_UNKNOWN) ? vu : vf)[go * CT + c] : 0.0;
      double rhs = 0.0;
      if (solved) {
        double g = 0.0, f = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (ln[k] == PSN_EXCLUDED) continue;
          const size_t gn = (size_t)ni[k] * W + nj[k];
          if (hp && hs[gn] != 0) g = g + ((double)s[go * CT + c] - (double)s[gn * CT + c]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (ln[k] != PSN_FIXED) continue;
          const size_t gn = (size_t)ni[k] * W + nj[k];
          f = f + (keep ? x[c * plane + (size_t)((ptrdiff_t)o + no[k])] : (double)vf[gn * CT + c]);
        }
        rhs = g + f;
      }
      b[c * plane + o] = rhs;
    }
  }
}

// The next level's operator, the Galerkin one of piecewise-constant transfer,
// in integers: with the children c00 c01 / c10 c11 of a cell
//   up = up(c00) + up(c01); down = down(c10) + down(c11)
//   left = left(c00) + left(c10); right = right(c01) + right(c11)
//   d = d(c00) + d(c01) + d(c10) + d(c11) - 2 (right(c00) + right(c10) + down(c00) + down(c01))
// fw: the fine window's width; one thread per coarse cell.
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_psn_coarsen(const int *__restrict__ fd, const ushort4 *__restrict__ fwt, int fw, PsnWin win, int *__restrict__ d,
              ushort4 *__restrict__ wt) {
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const size_t o00 = (size_t)(2 * i) * fw + 2 * j, o01 = o00 + 1, o10 = o00 + fw, o11 = o10 + 1;
    const ushort4 a = fwt[o00], bq = fwt[o01], cq = fwt[o10], e = fwt[o11];  // .x up .y down .z left .w right
    const size_t o = (size_t)i * win.w + j;
    wt[o] = make_ushort4(a.x + bq.x, cq.y + e.y, a.z + cq.z, bq.w + e.w);
    d[o] = fd[o00] + fd[o01] + fd[o10] + fd[o11] - 2 * ((int)a.w + (int)cq.w + (int)a.y + (int)bq.y);
  }
}

// `sweeps` red-black Gauss-Seidel sweeps of one level, xin -> xout: colour
// k = 0, then 1, a solved cell with (row + column) & 1 == k of the level's grid
// becoming (b + wt_n x_n over the coupled neighbours up, down, left, right) / d.
// One workgroup per 32 x 32 tile of the window (gx tiles across, 1-D grid in
// the XCD-aware order): the tile and a halo of 2 cells per sweep go to LDS with
// their d and wt; every colour pass relaxes all cells of the LDS region but its
// outermost ring, so a stale value moves inwards one ring per pass and stops
// short of the tile, whose cells come out as a sweep over the whole level
// would leave them.  Two buffers: a tile's halo is its neighbours' interior.
template <int CT>
__global__ void __launch_bounds__(PSN_THREADS)
k_psn_smooth(const int *__restrict__ d, const ushort4 *__restrict__ wt, const double *__restrict__ b,
             const double *__restrict__ xin, double *__restrict__ xout, PsnWin win, int gx, int sweeps) {
  OF_NOCONTRACT
  __shared__ double s_x[CT][PSN_R * PSN_R];
  __shared__ int s_d[PSN_R * PSN_R];
  __shared__ ushort4 s_w[PSN_R * PSN_R];
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
    s_d[e] = in ? d[o] : 0;
    s_w[e] = in ? wt[o] : make_ushort4(0, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < CT; ++c) s_x[c][e] = in ? xin[c * plane + o] : 0.0;
  }
  __syncthreads();
  const int half = R / 2;  // R is even: cells of one colour per row
  for (int pass = 0; pass < 2 * sweeps; ++pass) {
    const int k = pass & 1;
    for (int e = tid; e < (R - 2) * half; e += PSN_THREADS) {
      const int ly = 1 + e / half, m = e - (ly - 1) * half;
      // the columns of row ly with (window row + r0 + window column + c0) & 1 == k
      const int lx = 2 * m + ((win.r0 + i0 + ly + win.c0 + j0 + k) & 1);
      if (lx < 1 || lx > R - 2) continue;
      const int q = ly * R + lx;
      const int dq = s_d[q];
      if (dq <= 0) continue;
      const ushort4 wq = s_w[q];
      const size_t o = (size_t)(i0 + ly) * win.w + (j0 + lx);  // a solved cell lies inside the window
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        double t = b[c * plane + o];
        if (wq.x) t = t + (double)wq.x * s_x[c][q - R];
        if (wq.y) t = t + (double)wq.y * s_x[c][q + R];
        if (wq.z) t = t + (double)wq.z * s_x[c][q - 1];
        if (wq.w) t = t + (double)wq.w * s_x[c][q + 1];
        s_x[c][q] = t / (double)dq;
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < PSN_T * PSN_T; e += PSN_THREADS) {
    const int ty = e / PSN_T, tx = e - ty * PSN_T;
    const int i = i0 + halo + ty, j = j0 + halo + tx;
    if (i >= win.h || j >= win.w) continue;
    const int q = (halo + ty) * R + halo + tx;
    const size_t o = (size_t)i * win.w + j;
#pragma unroll
    for (int c = 0; c < CT; ++c) xout[c * plane + o] = s_x[c][q];
  }
}

// the residual b - d x + wt_n x_n (neighbours up, down, left, right) of cell o
// of a level, 0 where it is not solved for
template <int CT>
__device__ __forceinline__ void psn_residual(const int *__restrict__ d, const ushort4 *__restrict__ wt,
                                             const double *__restrict__ b, const double *__restrict__ x, size_t plane,
                                             int w, size_t o, double r[CT]) {
  OF_NOCONTRACT
  const int dq = d[o];
  const ushort4 wq = wt[o];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    double t = 0.0;
    if (dq > 0) {
      const double *__restrict__ xc = x + c * plane;
      t = b[c * plane + o] - (double)dq * xc[o];
      if (wq.x) t = t + (double)wq.x * xc[o - w];
      if (wq.y) t = t + (double)wq.y * xc[o + w];
      if (wq.z) t = t + (double)wq.z * xc[o - 1];
      if (wq.w) t = t + (double)wq.w * xc[o + 1];
    }
    r[c] = t;
  }
}

// The coarse right-hand side: ((res(c00) + res(c01)) + res(c10)) + res(c11) of
// the four children on the solved coarse cells, 0 on the others; the coarse
// unknown starts from 0.  fd .. fx: the fine level; one thread per coarse cell.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_psn_restrict(const int *__restrict__ fd, const ushort4 *__restrict__ fwt, const double *__restrict__ fb,
               const double *__restrict__ fx, int fh, int fw, const int *__restrict__ d, PsnWin win,
               double *__restrict__ b, double *__restrict__ x) {
  OF_NOCONTRACT
  const size_t fplane = (size_t)fh * fw, plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const size_t o = (size_t)i * win.w + j;
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    if (d[o] > 0) {
      const size_t o00 = (size_t)(2 * i) * fw + 2 * j;
      double r[CT];
      psn_residual<CT>(fd, fwt, fb, fx, fplane, fw, o00, acc);
      psn_residual<CT>(fd, fwt, fb, fx, fplane, fw, o00 + 1, r);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = acc[c] + r[c];
      psn_residual<CT>(fd, fwt, fb, fx, fplane, fw, o00 + fw, r);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = acc[c] + r[c];
      psn_residual<CT>(fd, fwt, fb, fx, fplane, fw, o00 + fw + 1, r);
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

// x = x + PSN_OMEGA * e(parent) on the solved cells of the fine level; cw: the
// coarse window's width; one thread per fine cell.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_psn_prolong(const int *__restrict__ d, PsnWin win, double *__restrict__ x, const double *__restrict__ e, int cw) {
  OF_NOCONTRACT
  const size_t plane = (size_t)win.h * win.w, cplane = (size_t)(win.h / 2) * cw;
  OF_FOR_PIXELS_XCD(win.h, win.w) {
    if (j >= win.w) continue;
    const size_t o = (size_t)i * win.w + j;
    if (d[o] <= 0) continue;
    const size_t p = (size_t)(i >> 1) * cw + (j >> 1);
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c * plane + o] = x[c * plane + o] + PSN_OMEGA * e[c * cplane + p];
  }
}

// The coarsest level, at most PSN_CMAX cells, relaxed `sweeps` times in LDS in
// place: one workgroup per channel (blockIdx.x), the same red-black sweep as
// k_psn_smooth.
__global__ void __launch_bounds__(PSN_THREADS)
k_psn_coarsest(const int *__restrict__ d, const ushort4 *__restrict__ wt, const double *__restrict__ b,
               double *__restrict__ x, PsnWin win, int sweeps) {
  OF_NOCONTRACT
  __shared__ double s_x[PSN_CMAX], s_b[PSN_CMAX];
  __shared__ int s_d[PSN_CMAX];
  __shared__ ushort4 s_w[PSN_CMAX];
  const int n = win.h * win.w, tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  for (int e = tid; e < n; e += PSN_THREADS) {
    s_x[e] = x[base + e];
    s_b[e] = b[base + e];
    s_d[e] = d[e];
    s_w[e] = wt[e];
  }
  __syncthreads();
  for (int pass = 0; pass < 2 * sweeps; ++pass) {
    const int k = pass & 1;
    for (int e = tid; e < n; e += PSN_THREADS) {
      const int i = e / win.w, j = e - i * win.w;
      const int dq = s_d[e];
      if (dq <= 0 || ((win.r0 + i + win.c0 + j) & 1) != k) continue;
      const ushort4 wq = s_w[e];
      double t = s_b[e];
      if (wq.x) t = t + (double)wq.x * s_x[e - win.w];
      if (wq.y) t = t + (double)wq.y * s_x[e + win.w];
      if (wq.z) t = t + (double)wq.z * s_x[e - 1];
      if (wq.w) t = t + (double)wq.w * s_x[e + 1];
      s_x[e] = t / (double)dq;
    }
    __syncthreads();
  }
  for (int e = tid; e < n; e += PSN_THREADS) x[base + e] = s_x[e];
}

// of_poisson_solve's result: H x W x C interleaved fp64, the window's x inside
// the window and (double) of vf elsewhere.  One thread per pixel.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_psn_store(const float *__restrict__ vf, const double *__restrict__ x, PsnWin win, int H, int W,
            double *__restrict__ out) {
  const size_t plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t go = (size_t)i * W + j;
    const int li = i - win.r0, lj = j - win.c0;
    const bool in = x && li >= 0 && li < win.h && lj >= 0 && lj < win.w;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      out[go * CT + c] = in ? x[c * plane + (size_t)li * win.w + lj] : (double)vf[go * CT + c];
  }
}

// The two stages' label planes of a blended fill from Om, the frame's grown
// mask, and st, the status plane of the fill with the mask grown by one more:
// hs = (st == FILLED); stage 1: unknown on Om & hs, excluded on Om & !hs, fixed
// elsewhere; stage 2: unknown on Om & !hs, fixed elsewhere.
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_blend_labels(const uint8_t *__restrict__ Om, const uint8_t *__restrict__ st, int H, int W, uint8_t *__restrict__ lab1,
               uint8_t *__restrict__ lab2, uint8_t *__restrict__ hs) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j;
    const bool om = Om[o] != 0, h = st[o] == OF_INPAINT_FILLED;
    lab1[o] = om ? (h ? PSN_UNKNOWN : PSN_EXCLUDED) : PSN_FIXED;
    lab2[o] = (om && !h) ? PSN_UNKNOWN : PSN_FIXED;
    hs[o] = h ? 1 : 0;
  }
}

// The blended frame: (float) of the window's x on Om (x nullptr: Om is empty),
// the frame's own value elsewhere; status KEPT outside Om, FILLED on Om & hs,
// SPATIAL on Om & !hs (status may be nullptr).
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_blend_store(const float *__restrict__ I, const uint8_t *__restrict__ Om, const uint8_t *__restrict__ hs,
              const double *__restrict__ x, PsnWin win, int H, int W, float *__restrict__ out,
              uint8_t *__restrict__ status) {
  const size_t plane = (size_t)win.h * win.w;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t go = (size_t)i * W + j;
    const int li = i - win.r0, lj = j - win.c0;
    const bool om = x && Om[go] != 0 && li >= 0 && li < win.h && lj >= 0 && lj < win.w;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      out[go * CT + c] = om ? (float)x[c * plane + (size_t)li * win.w + lj] : I[go * CT + c];
    if (status) status[go] = !om ? OF_INPAINT_KEPT : (hs[go] ? OF_INPAINT_FILLED : OF_INPAINT_SPATIAL);
  }
}
