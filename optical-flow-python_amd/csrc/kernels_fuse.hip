// kernels_fuse.hip — motion-compensated temporal denoising: chaining two
// flows (k_flow_compose) and fusing a frame with its neighbours warped along
// flows from the frame to each of them (k_fuse), every neighbour weighted per
// pixel by how well its warped patch matches the frame's.  Frames are dense
// H x W x C interleaved fp32, flows pitched float2, states dense H x W bytes
// in of_fb_consistency's encoding.  All arithmetic in fp64 from the fp32
// inputs with no contraction, in the order include/optflow.h states
// (of_flow_compose, of_fuse_frames), so a numpy float64 restatement gives the
// same bits.  H * W < 2^31 (checked on the host).
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
    trk_bil2(g, W, P, bil_tap(r, q, H, W), gu, gv);
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

// One thread per pixel of a 32 x 8 tile, the loop over the n neighbours inside
// (the pixel's frame value, acc and wsum stay in registers).  Per neighbour the
// block writes D and the visibility of its tile plus an r-wide halo to LDS --
// every thread its own pixel, keeping the warped sample, then the threads
// share the halo ring -- and after a barrier each visible pixel sums its
// window from LDS in row-major order, so the result does not depend on the
// tile geometry.  gx = tiles across; the grid is 1-D in the XCD-aware order.
__global__ void __launch_bounds__(FUSE_TW *FUSE_TH)
k_fuse(const float *__restrict__ I, FuseArgs A, int n, int H, int W, int P, int C, int r, double two_s2, double h2,
       int gx, float *__restrict__ out, float *__restrict__ out_w) {
  OF_NOCONTRACT
  __shared__ double s_D[FUSE_LDS];
  __shared__ uint8_t s_v[FUSE_LDS];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int i0 = tyi * FUSE_TH, j0 = txi * FUSE_TW;
  const int tid = threadIdx.x;
  const int ly = tid / FUSE_TW, lx = tid - ly * FUSE_TW;
  const int i = i0 + ly, j = j0 + lx;
  const bool own = i < H && j < W;
  const int LW = FUSE_TW + 2 * r;                         // LDS row length
  const int n_top = 2 * r * LW, n_ring = n_top + 2 * r * FUSE_TH;  // halo ring: rows above and below, then the sides
  const size_t o = (size_t)i * W + j;
  double ctr[FUSE_MAX_C], acc[FUSE_MAX_C], wsum = 1.0;
#pragma unroll
  for (int c = 0; c < FUSE_MAX_C; ++c) {
    ctr[c] = own && c < C ? (double)I[o * C + c] : 0.0;
    acc[c] = ctr[c];
  }
  for (int k = 0; k < n; ++k) {
    const float *__restrict__ N = A.neigh[k];
    const float2 *__restrict__ F = A.flow[k];
    const uint8_t *__restrict__ S = A.state[k];
    double wk[FUSE_MAX_C] = {0.0, 0.0, 0.0, 0.0}, D = 0.0;
    const bool vis = own && fuse_sample(I, N, F, S, i, j, H, W, P, C, wk, D);
    const int lo = (ly + r) * LW + lx + r;
    s_D[lo] = vis ? D : 0.0;
    s_v[lo] = vis ? 1 : 0;
    for (int h = tid; h < n_ring; h += FUSE_TW * FUSE_TH) {
      int a, b;  // position in the LDS region
      if (h < n_top) {
        a = h / LW;
        b = h - a * LW;
        a = a < r ? a : a + FUSE_TH;
      } else {
        const int q = h - n_top;
        a = q / (2 * r);
        b = q - a * (2 * r);
        a += r;
        b = b < r ? b : b + FUSE_TW;
      }
      const int y = i0 - r + a, x = j0 - r + b;
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
          const int p = (ly + a) * LW + lx + b;
          if (s_v[p]) {
            Ssum = Ssum + s_D[p];
            ++m;
          }
        }
      const double d = Ssum / (double)(m * C);
      const double t = d - two_s2;
      const double e = t > 0.0 ? t : 0.0;
      const double z = e / h2;
      const double x = z < 1.0 ? z : 1.0;
      const double w = (1.0 - x) * (1.0 - x);
#pragma unroll
      for (int c = 0; c < FUSE_MAX_C; ++c) acc[c] = acc[c] + w * wk[c];
      wsum = wsum + w;
    }
    __syncthreads();  // the next neighbour overwrites the LDS planes
  }
  if (!own) return;
#pragma unroll
  for (int c = 0; c < FUSE_MAX_C; ++c)
    if (c < C) out[o * C + c] = (float)(acc[c] / wsum);
  if (out_w) out_w[o] = (float)wsum;
}
