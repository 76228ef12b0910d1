// kernels_inpaint.hip — flow-guided video inpainting: growing a byte mask, or
// the union of two, by a square window into a byte plane and / or the data
// weight of a pair (k_mask_grow), and filling the masked pixels of a frame
// with what the other frames of the clip show there, found by walking along
// the flows of the adjacent pairs (k_inpaint_fill).  Frames are dense
// H x W x C interleaved fp32, flows pitched float2, masks dense H x W bytes.
// All arithmetic in fp64 from the fp32 inputs with no contraction, in the
// order include/optflow.h states (of_inpaint_fill), so a numpy float64
// restatement gives the same bits.  H * W < 2^31 (checked on the host).
// Expects kernels_sample.hip before it (in_frame, bil_tap, bil_at, bil2).
#include "kernels.h"

#define INP_MAX_R 16   // hops per direction
#define INP_MAX_C 4    // channels
#define INP_MAX_G 24   // k_mask_grow's radius
#define INP_TW 32      // k_mask_grow's tile: 32 x 8 pixels, one thread each (four waves)
#define INP_TH 8
#define INP_LW (INP_TW + 2 * INP_MAX_G)
#define INP_LH (INP_TH + 2 * INP_MAX_G)

// out(i, j) = any of (a | b) != 0 within g pixels per axis, positions outside
// the frame counting as 0; b may be nullptr.  out_m: bytes 0 / 1; out_w: the
// data weight of a pair, 0.0f where out is set and 1.0f elsewhere, rows of
// pitch wP; either may be nullptr.  One workgroup per 32 x 8 tile (gx tiles
// across, 1-D grid in the XCD-aware order): the tile and its g-wide halo of
// (a | b) != 0 go to LDS, the window's rows are folded there once for the whole
// tile, then every thread folds its column of row results.
__global__ void __launch_bounds__(INP_TW *INP_TH)
k_mask_grow(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int H, int W, int g, int gx,
            uint8_t *__restrict__ out_m, float *__restrict__ out_w, int wP) {
  __shared__ uint8_t s_m[INP_LH * INP_LW];
  __shared__ uint8_t s_h[INP_LH * INP_TW];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int i0 = tyi * INP_TH, j0 = txi * INP_TW;
  const int tid = threadIdx.x;
  const int LW = INP_TW + 2 * g, LH = INP_TH + 2 * g;
  for (int e = tid; e < LH * LW; e += INP_TW * INP_TH) {
    const int la = e / LW, lb = e - la * LW;
    const int y = i0 - g + la, x = j0 - g + lb;
    uint8_t m = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t o = (size_t)y * W + x;
      m = (a[o] != 0 || (b && b[o] != 0)) ? 1 : 0;
    }
    s_m[e] = m;
  }
  __syncthreads();
  for (int e = tid; e < LH * INP_TW; e += INP_TW * INP_TH) {
    const int la = e / INP_TW, lx = e - la * INP_TW;
    uint8_t m = 0;
    for (int k = 0; k <= 2 * g; ++k) m |= s_m[la * LW + lx + k];
    s_h[e] = m;
  }
  __syncthreads();
  const int ly = tid / INP_TW, lx = tid - ly * INP_TW;
  const int i = i0 + ly, j = j0 + lx;
  if (i >= H || j >= W) return;
  uint8_t m = 0;
  for (int k = 0; k <= 2 * g; ++k) m |= s_h[(ly + k) * INP_TW + lx];
  if (out_m) out_m[(size_t)i * W + j] = m;
  if (out_w) out_w[(size_t)i * wP + j] = m ? 0.0f : 1.0f;
}

// The hops of the two walks of a fill, [0]: forward (flows fw_t, fw_t+1, ...
// and frames t+1, t+2, ...), [1]: backward (bw_t-1, bw_t-2, ... and t-1, t-2,
// ...); hop d at index d - 1.
struct InpaintArgs {
  const float2 *flow[2][INP_MAX_R];   // pitched, the flow of the hop
  const uint8_t *mask[2][INP_MAX_R];  // H x W dense, the grown mask of the hop's target
  const float *frame[2][INP_MAX_R];   // H x W x C dense, the target
  int n[2];                           // hops that exist, <= INP_MAX_R
};

// One thread per pixel, a wave per row segment of 64.  A pixel outside the
// grown mask D is copied.  A pixel inside walks forward and backward; the hop
// loop runs per wave, every lane at the same hop d, finished lanes masked, and
// the wave leaves it when no lane is live, so the hop's table entries are
// scalar loads from the kernel arguments.  CT = the channel count, or 0 for
// the generic path (C <= INP_MAX_C at run time).  status: H x W bytes or
// nullptr; hops: 2 x H x W bytes (forward, backward) or nullptr.
template <int CT>
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_inpaint_fill(const float *__restrict__ I, const uint8_t *__restrict__ D, InpaintArgs A, int H, int W, int P, int Cr,
               float *__restrict__ out, uint8_t *__restrict__ status, uint8_t *__restrict__ hops) {
  OF_NOCONTRACT
  constexpr int CM = CT ? CT : INP_MAX_C;
  const int C = CT ? CT : Cr;
  const size_t px = (size_t)H * W;
  OF_FOR_PIXELS_XCD(H, W) {
    const bool own = j < W;
    const size_t o = own ? (size_t)i * W + j : 0;
    const bool hole = own && D[o] != 0;
    double col[2][CM];
    int hit[2] = {0, 0};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
#pragma unroll
      for (int c = 0; c < CM; ++c) col[dir][c] = 0.0;
      double r = (double)i, q = (double)j;
      bool live = hole;
      for (int d = 0; d < A.n[dir]; ++d) {
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;
        if (live) {
          double u, v;
          bil2(A.flow[dir][d], W, P, bil_tap(r, q, H, W), u, v);
          live = __builtin_isfinite(u) && __builtin_isfinite(v);
          if (live) {
            r = r + v;
            q = q + u;
            live = in_frame(r, q, H, W);
          }
          if (live) {
            const BilTap b = bil_tap(r, q, H, W);
            const uint8_t *__restrict__ M = A.mask[dir][d];
            if ((M[b.o00] | M[b.o01] | M[b.o10] | M[b.o11]) == 0) {
              const float *__restrict__ N = A.frame[dir][d];
#pragma unroll
              for (int c = 0; c < CM; ++c)
                if (c < C) col[dir][c] = bil_at(N, C, c, b);
              hit[dir] = d + 1;
              live = false;
            }
          }
        }
      }
    }
    if (!own) continue;
    const int df = hit[0], db = hit[1];
    const bool filled = df != 0 || db != 0;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        float v = I[o * C + c];
        if (df != 0 && db != 0) v = (float)(((double)db * col[0][c] + (double)df * col[1][c]) / (double)(df + db));
        else if (df != 0) v = (float)col[0][c];
        else if (db != 0) v = (float)col[1][c];
        out[o * C + c] = v;
      }
    if (status) status[o] = !hole ? OF_INPAINT_KEPT : (filled ? OF_INPAINT_FILLED : OF_INPAINT_UNFILLED);
    if (hops) {
      hops[o] = (uint8_t)df;
      hops[px + o] = (uint8_t)db;
    }
  }
}
