// kernels_track.hip — dense point trajectories (Sundaram, Brox and Keutzer,
// ECCV 2010): a table of points carried from frame to frame by the forward
// flow, ended by the forward-backward test, the frame border or a motion
// boundary, and re-seeded on a grid wherever the picture has structure and no
// live track covers the cell.  Flows are pitched float2, the gray plane
// pitched fp32, the table dense (xy float2, status and start per track).  All
// arithmetic in fp64 from the fp32 inputs with no contraction, in the order
// include/optflow.h states (of_track_advance, of_track_seed), so a numpy
// float64 restatement gives the same bits.  H * W < 2^31 (checked on the host).
// Expects kernels_sample.hip before it (in_frame, bil_tap, bil2); trk_near is
// what kernels_fuse.hip, included after this file, uses as well.
#include "kernels.h"

#define TRK_BLOCK 256  // every kernel here: 1-D blocks of four waves

// near(x, n): the nearest index, clamped (NaN gives 0, so it never leaves the plane)
__device__ __forceinline__ int trk_near(double x, int n) {
  return (int)fmin(fmax(floor(x + 0.5), 0.0), (double)(n - 1));
}

// One thread per track: follow F (frame k -> k+1) from the point, and end the
// track where it leaves the frame (2), where the backward flow B does not lead
// back (1) or where F has a motion boundary at the point (3), in that order.
// A track that is not alive is copied.  in and out may be the same table.
__global__ void __launch_bounds__(TRK_BLOCK)
k_track_advance(const float2 *__restrict__ F, const float2 *__restrict__ B, int H, int W, int P, double alpha1,
                double alpha2, double beta1, double beta2, int n, const float2 *xy_in, const uint8_t *st_in,
                float2 *xy_out, uint8_t *st_out) {
  OF_NOCONTRACT
  const int t = blockIdx.x * TRK_BLOCK + threadIdx.x;
  if (t >= n) return;
  const float2 p = xy_in[t];
  const uint8_t s = st_in[t];
  xy_out[t] = p;
  st_out[t] = s;
  if (s != OF_TRACK_ALIVE) return;
  const double xd = p.x, yd = p.y;
  if (!in_frame(yd, xd, H, W)) {
    st_out[t] = OF_TRACK_LEFT_FRAME;
    return;
  }
  double u, v, bu, bv;
  bil2(F, W, P, bil_tap(yd, xd, H, W), u, v);
  const double x1 = xd + u, y1 = yd + v;
  if (!in_frame(y1, x1, H, W)) {
    st_out[t] = OF_TRACK_LEFT_FRAME;
    return;
  }
  bil2(B, W, P, bil_tap(y1, x1, H, W), bu, bv);
  const double du = u + bu, dv = v + bv;
  const double err = du * du + dv * dv;
  const double mag = u * u + v * v;
  const double thr = alpha1 * (mag + (bu * bu + bv * bv)) + alpha2;
  if (!(err <= thr)) {
    st_out[t] = OF_TRACK_OCCLUDED;
    return;
  }
  const int i = trk_near(yd, H), j = trk_near(xd, W);
  const int jm = max(j - 1, 0), jp = min(j + 1, W - 1), im = max(i - 1, 0), ip = min(i + 1, H - 1);
  const float2 fl = F[(size_t)i * P + jm], fr = F[(size_t)i * P + jp];
  const float2 fu = F[(size_t)im * P + j], fd = F[(size_t)ip * P + j];
  const double ux = (double)fr.x - (double)fl.x, uy = (double)fd.x - (double)fu.x;
  const double vx = (double)fr.y - (double)fl.y, vy = (double)fd.y - (double)fu.y;
  const double g = 0.25 * ((ux * ux + uy * uy) + (vx * vx + vy * vy));
  if (!(g <= beta1 * mag + beta2)) {
    st_out[t] = OF_TRACK_MOTION_BOUNDARY;
    return;
  }
  xy_out[t] = make_float2((float)x1, (float)y1);
}

// One thread per track: an alive track occupies the seeding cell of its
// nearest pixel.  occ: ncj-wide bytes, zeroed before; every writer stores 1.
__global__ void __launch_bounds__(TRK_BLOCK)
k_track_mark(int n, const float2 *__restrict__ xy, const uint8_t *__restrict__ st, int H, int W, int step, int ncj,
             uint8_t *__restrict__ occ) {
  const int t = blockIdx.x * TRK_BLOCK + threadIdx.x;
  if (t >= n || st[t] != OF_TRACK_ALIVE) return;
  const float2 p = xy[t];
  const int ci = trk_near((double)p.y, H) / step, cj = trk_near((double)p.x, W) / step;
  occ[(size_t)ci * ncj + cj] = 1;
}

// the block's count of set flags (every thread calls it; valid in thread 0),
// and each thread's rank among them
__device__ __forceinline__ int trk_block_rank(bool f, int &rank) {
  __shared__ int s_w[TRK_BLOCK / 64];
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < TRK_BLOCK / 64; ++k) {
    before += k < w ? s_w[k] : 0;
    total += s_w[k];
  }
  rank = before + __popcll(m & ((1ull << lane) - 1ull));
  return total;
}

// One thread per seeding cell (row-major): flag = the cell is free, its
// candidate pixel lies in the frame and the smallest eigenvalue of the 3 x 3
// structure tensor around it is >= min_eig (any free cell when min_eig == 0).
// bcnt[block] = the block's accepted cells.
__global__ void __launch_bounds__(TRK_BLOCK)
k_track_flags(const float *__restrict__ G, int H, int W, int P, int step, int nci, int ncj, double min_eig,
              const uint8_t *__restrict__ occ, uint8_t *__restrict__ flags, int *__restrict__ bcnt) {
  OF_NOCONTRACT
  const int cell = blockIdx.x * TRK_BLOCK + threadIdx.x;
  bool f = false;
  if (cell < nci * ncj) {
    const int ci = cell / ncj, cj = cell - ci * ncj;
    const int i = ci * step + step / 2, j = cj * step + step / 2;
    f = i < H && j < W && occ[cell] == 0;
    if (f && min_eig != 0.0) {
      double Jxx = 0.0, Jxy = 0.0, Jyy = 0.0;
      for (int da = -1; da <= 1; ++da)
        for (int db = -1; db <= 1; ++db) {
          const int a = clampi(i + da, 0, H - 1), b = clampi(j + db, 0, W - 1);
          const float *row = G + (size_t)a * P;
          const double gx = 0.5 * ((double)row[min(b + 1, W - 1)] - (double)row[max(b - 1, 0)]);
          const double gy = 0.5 * ((double)G[(size_t)min(a + 1, H - 1) * P + b] -
                                   (double)G[(size_t)max(a - 1, 0) * P + b]);
          Jxx = Jxx + gx * gx;
          Jxy = Jxy + gx * gy;
          Jyy = Jyy + gy * gy;
        }
      const double T = Jxx + Jyy, D = Jxx * Jyy - Jxy * Jxy;
      f = T >= 2.0 * min_eig && (D - min_eig * T) + min_eig * min_eig >= 0.0;
    }
    flags[cell] = f ? 1 : 0;
  }
  int rank;
  const int total = trk_block_rank(f, rank);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

// One block: bcnt[0..nb) -> its exclusive prefix sum in place, *total = the sum
__global__ void __launch_bounds__(TRK_BLOCK) k_track_scan(int *__restrict__ bcnt, int nb, int *__restrict__ total) {
  __shared__ int s_w[TRK_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nb; base += TRK_BLOCK) {
    const int k = base + threadIdx.x;
    const int v = k < nb ? bcnt[k] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int q = 0; q < TRK_BLOCK / 64; ++q) {
      before += q < w ? s_w[q] : 0;
      sum += s_w[q];
    }
    if (k < nb) bcnt[k] = carry + before + incl - v;
    carry += sum;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

// One thread per cell, the blocks of k_track_flags: accepted cell number r in
// row-major order (boff[block] + its rank in the block) becomes new track r
// while r < room; the rest are dropped.  st_new / start_new may be nullptr.
__global__ void __launch_bounds__(TRK_BLOCK)
k_track_scatter(const uint8_t *__restrict__ flags, const int *__restrict__ boff, int step, int ncells, int ncj,
                int room, int frame, float2 *__restrict__ xy_new, uint8_t *__restrict__ st_new,
                int32_t *__restrict__ start_new) {
  const int cell = blockIdx.x * TRK_BLOCK + threadIdx.x;
  const bool f = cell < ncells && flags[cell] != 0;
  int rank;
  trk_block_rank(f, rank);
  const int r = boff[blockIdx.x] + rank;
  if (!f || r >= room) return;
  const int ci = cell / ncj, cj = cell - ci * ncj;
  xy_new[r] = make_float2((float)(cj * step + step / 2), (float)(ci * step + step / 2));
  if (st_new) st_new[r] = OF_TRACK_ALIVE;
  if (start_new) start_new[r] = frame;
}
