// kernels_fuse.hip — motion-compensated temporal denoising: chaining two
// flows (k_flow_compose) and fusing a frame with its neighbours warped along
// flows from the frame to each of them (k_fuse), every neighbour weighted per
// pixel by how well its warped patch matches the frame's (k_fuse_weights gives
// those weights on their own).  Frames are dense
// H x W x C interleaved fp32, flows pitched float2, states dense H x W bytes
// in of_fb_consistency's encoding.  All arithmetic in fp64 from the fp32
// inputs with no contraction, in the order include/optflow.h states
// (of_flow_compose, of_fuse_frames), so a numpy float64 restatement gives the
// same bits.  H * W < 2^31 (checked on the host).  Expects kernels_sample.hip
// (in_frame, bil_tap, bil_at, bil2) and kernels_track.hip (trk_near) before it.
#include "kernels.h"

// out = f followed by g: the pixel's f, plus g sampled where f lands.  sf / sg
// / so may be nullptr (all 0 / not wanted).
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_flow_compose(const float2 *__restrict__ f, const float2 *__restrict__ g, int H, int W, int P,
               const uint8_t *__restrict__ sf, const uint8_t *__restrict__ sg, float2 *__restrict__ out,
               uint8_t *__restrict__ so) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const float2 a = f[(size_t)i * P + j];
    const size_t o = (size_t)i * W + j;
    const double u = a.x, v = a.y;
    const double r = (double)i + v, q = (double)j + u;
    if (!(__builtin_isfinite(a.x) && __builtin_isfinite(a.y) && in_frame(r, q, H, W))) {
      out[(size_t)i * P + j] = a;
      if (so) so[o] = 2;
      continue;
    }
    double gu, gv;
    bil2(g, W, P, bil_tap(r, q, H, W), gu, gv);
    out[(size_t)i * P + j] = make_float2((float)(u + gu), (float)(v + gv));
    if (so) {
      const uint8_t s0 = sf ? sf[o] : (uint8_t)0;
      const uint8_t s1 = sg ? sg[(size_t)trk_near(r, H) * W + trk_near(q, W)] : (uint8_t)0;
      so[o] = s0 > s1 ? s0 : s1;
    }
  }
}

#define FUSE_MAX_N 8   // neighbours per call
#define FUSE_MAX_C 4   // channels
#define FUSE_MAX_R 3   // half-size of the comparison window
#define FUSE_TW 32     // tile: 32 x 8 pixels, one thread each (four waves)
#define FUSE_TH 8
#define FUSE_LDS ((FUSE_TW + 2 * FUSE_MAX_R) * (FUSE_TH + 2 * FUSE_MAX_R))

struct FuseArgs {
  const float *neigh[FUSE_MAX_N];    // H x W x C dense
  const float2 *flow[FUSE_MAX_N];    // pitched, centre -> neighbour k
  const uint8_t *state[FUSE_MAX_N];  // H x W dense or nullptr (all 0)
};

// Neighbour N at pixel (i, j) of the frame I: visible = the flow is finite,
// lands inside the frame and its state is 0; then wk[c] = the warped sample
// (one set of taps for all channels) and D = the squared difference to I
// summed over the channels.
__device__ __forceinline__ bool fuse_sample(const float *__restrict__ I, const float *__restrict__ N,
                                            const float2 *__restrict__ F, const uint8_t *__restrict__ S, int i, int j,
                                            int H, int W, int P, int C, double (&wk)[FUSE_MAX_C], double &D) {
  OF_NOCONTRACT
  const float2 g = F[(size_t)i * P + j];
  const size_t o = (size_t)i * W + j;
  const double r = (double)i + (double)g.y, q = (double)j + (double)g.x;
  if (!(__builtin_isfinite(g.x) && __builtin_isfinite(g.y) && in_frame(r, q, H, W))) return false;
  if (S && S[o] != 0) return false;
  const BilTap b = bil_tap(r, q, H, W);
  double d = 0.0;
#pragma unroll
  for (int c = 0; c < FUSE_MAX_C; ++c) {
    wk[c] = 0.0;
    if (c < C) {
      wk[c] = bil_at(N, C, c, b);
      const double dd = (double)I[o * C + c] - wk[c];
      d = d + dd * dd;
    }
  }
  D = d;
  return true;
}

// The thread's place in its 32 x 8 tile (gx = tiles across; the grid is 1-D in
// the XCD-aware order) and the geometry of the tile's LDS region for a window
// of half-size r.
struct FuseTile {
  int i0, j0, ly, lx, i, j, tid;
  bool own;
  int LW, n_top, n_ring;  // LDS row length; halo ring: rows above and below, then the sides
  size_t o;
};
__device__ __forceinline__ FuseTile fuse_tile(int H, int W, int r, int gx) {
  FuseTile t;
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  t.i0 = tyi * FUSE_TH;
  t.j0 = txi * FUSE_TW;
  t.tid = threadIdx.x;
  t.ly = t.tid / FUSE_TW;
  t.lx = t.tid - t.ly * FUSE_TW;
  t.i = t.i0 + t.ly;
  t.j = t.j0 + t.lx;
  t.own = t.i < H && t.j < W;
  t.LW = FUSE_TW + 2 * r;
  t.n_top = 2 * r * t.LW;
  t.n_ring = t.n_top + 2 * r * FUSE_TH;
  t.o = (size_t)t.i * W + t.j;
  return t;
}

// vis_k and w_k of one neighbour at the thread's pixel, the whole block
// together: the block writes D and the visibility of its tile plus an r-wide
// halo to LDS -- every thread its own pixel, keeping the warped sample wk,
// then the threads share the halo ring -- and after a barrier each visible
// pixel sums its window from LDS in row-major order, so the result does not
// depend on the tile geometry.  Ends in a barrier: the next neighbour
// overwrites the LDS planes.  w is written only where the pixel is visible.
__device__ __forceinline__ bool fuse_weight(const float *__restrict__ I, const float *__restrict__ N,
                                            const float2 *__restrict__ F, const uint8_t *__restrict__ S,
                                            const FuseTile &t, int H, int W, int P, int C, int r, double two_s2,
                                            double h2, double *s_D, uint8_t *s_v, double (&wk)[FUSE_MAX_C], double &w) {
  OF_NOCONTRACT
  double D = 0.0;
  const bool vis = t.own && fuse_sample(I, N, F, S, t.i, t.j, H, W, P, C, wk, D);
  const int LW = t.LW, lo = (t.ly + r) * LW + t.lx + r;
  s_D[lo] = vis ? D : 0.0;
  s_v[lo] = vis ? 1 : 0;
  for (int h = t.tid; h < t.n_ring; h += FUSE_TW * FUSE_TH) {
    int a, b;  // position in the LDS region
    if (h < t.n_top) {
      a = h / LW;
      b = h - a * LW;
      a = a < r ? a : a + FUSE_TH;
    } else {
      const int q = h - t.n_top;
      a = q / (2 * r);
      b = q - a * (2 * r);
      a += r;
      b = b < r ? b : b + FUSE_TW;
    }
    const int y = t.i0 - r + a, x = t.j0 - r + b;
    double hw[FUSE_MAX_C], hD = 0.0;
    const bool hv = y >= 0 && y < H && x >= 0 && x < W && fuse_sample(I, N, F, S, y, x, H, W, P, C, hw, hD);
    s_D[a * LW + b] = hv ? hD : 0.0;
    s_v[a * LW + b] = hv ? 1 : 0;
  }
  __syncthreads();
  if (vis) {
    double Ssum = 0.0;
    int m = 0;
    for (int a = 0; a <= 2 * r; ++a)
      for (int b = 0; b <= 2 * r; ++b) {
        const int p = (t.ly + a) * LW + t.lx + b;
        if (s_v[p]) {
          Ssum = Ssum + s_D[p];
          ++m;
        }
      }
    const double d = Ssum / (double)(m * C);
    const double e0 = d - two_s2;
    const double e = e0 > 0.0 ? e0 : 0.0;
    const double z = e / h2;
    const double x = z < 1.0 ? z : 1.0;
    w = (1.0 - x) * (1.0 - x);
  }
  __syncthreads();
  return vis;
}

// One thread per pixel of a 32 x 8 tile, the loop over the n neighbours inside
// (the pixel's frame value, acc and wsum stay in registers); fuse_weight gives
// every neighbour's weight.
__global__ void __launch_bounds__(FUSE_TW *FUSE_TH)
k_fuse(const float *__restrict__ I, FuseArgs A, int n, int H, int W, int P, int C, int r, double two_s2, double h2,
       int gx, float *__restrict__ out, float *__restrict__ out_w) {
  OF_NOCONTRACT
  __shared__ double s_D[FUSE_LDS];
  __shared__ uint8_t s_v[FUSE_LDS];
  const FuseTile t = fuse_tile(H, W, r, gx);
  double ctr[FUSE_MAX_C], acc[FUSE_MAX_C], wsum = 1.0;
#pragma unroll
  for (int c = 0; c < FUSE_MAX_C; ++c) {
    ctr[c] = t.own && c < C ? (double)I[t.o * C + c] : 0.0;
    acc[c] = ctr[c];
  }
  for (int k = 0; k < n; ++k) {
    double wk[FUSE_MAX_C] = {0.0, 0.0, 0.0, 0.0}, w = 0.0;
    if (fuse_weight(I, A.neigh[k], A.flow[k], A.state[k], t, H, W, P, C, r, two_s2, h2, s_D, s_v, wk, w)) {
#pragma unroll
      for (int c = 0; c < FUSE_MAX_C; ++c) acc[c] = acc[c] + w * wk[c];
      wsum = wsum + w;
    }
  }
  if (!t.own) return;
#pragma unroll
  for (int c = 0; c < FUSE_MAX_C; ++c)
    if (c < C) out[t.o * C + c] = (float)(acc[c] / wsum);
  if (out_w) out_w[t.o] = (float)wsum;
}

// The neighbour weights on their own (of_fuse_weights): out_w[k] = (float)w_k,
// 0 where the neighbour is not visible; n dense H x W planes.
__global__ void __launch_bounds__(FUSE_TW *FUSE_TH)
k_fuse_weights(const float *__restrict__ I, FuseArgs A, int n, int H, int W, int P, int C, int r, double two_s2,
               double h2, int gx, float *__restrict__ out_w) {
  OF_NOCONTRACT
  __shared__ double s_D[FUSE_LDS];
  __shared__ uint8_t s_v[FUSE_LDS];
  const FuseTile t = fuse_tile(H, W, r, gx);
  const size_t px = (size_t)H * W;
  for (int k = 0; k < n; ++k) {
    double wk[FUSE_MAX_C] = {0.0, 0.0, 0.0, 0.0}, w = 0.0;
    const bool vis = fuse_weight(I, A.neigh[k], A.flow[k], A.state[k], t, H, W, P, C, r, two_s2, h2, s_D, s_v, wk, w);
    if (t.own) out_w[(size_t)k * px + t.o] = vis ? (float)w : 0.0f;
  }
}
