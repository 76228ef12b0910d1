// kernels_mask.hip — mask propagation: a binary mask carried from the previous
// frame to the current one along the backward flow (k_mask_carry), the pixels
// the flow cannot decide voted by their decided neighbours under a colour
// guide (k_mask_vote), and the mode filter that cleans the labels
// (k_mask_mode).  The guide is dense H x W x C interleaved fp32, the flow
// pitched float2, masks, states, labels and status dense H x W bytes, the
// carried plane A dense H x W fp32.  All arithmetic in fp64 from the fp32 or
// byte inputs with no contraction, in the order include/optflow.h states
// (of_mask_advance), so a numpy float64 restatement gives the same bits.
// H * W < 2^31 (checked on the host).  Expects kernels_sample.hip before it
// (in_frame, bil_tap).
#include "kernels.h"

#define MSK_MAX_R 12  // the vote's radius
#define MSK_MAX_C 4   // channels of the guide
#define MSK_MAX_S 2   // the mode filter's radius
#define MSK_TW 32     // the tile of k_mask_vote and k_mask_mode: 32 x 8 pixels, one thread each (four waves)
#define MSK_TH 8
#define MSK_LW (MSK_TW + 2 * MSK_MAX_R)
#define MSK_LH (MSK_TH + 2 * MSK_MAX_R)
#define MSK_UNDECIDED (-1.0f)  // A of a pixel the flow does not decide

// A(i, j) = (float)bil(M != 0, i + v, j + u) with (u, v) = B(i, j) where u and
// v are finite, the point lies inside the frame and S(i, j) == 0 (S may be
// nullptr: all 0); MSK_UNDECIDED elsewhere.  One thread per pixel.
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_mask_carry(const uint8_t *__restrict__ M, const float2 *__restrict__ B, const uint8_t *__restrict__ S, int H, int W,
             int P, float *__restrict__ A) {
  OF_NOCONTRACT
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j;
    const float2 f = B[(size_t)i * P + j];
    float a = MSK_UNDECIDED;
    if (__builtin_isfinite(f.x) && __builtin_isfinite(f.y) && (!S || S[o] == 0)) {
      const double r = (double)i + (double)f.y, q = (double)j + (double)f.x;
      if (in_frame(r, q, H, W)) {
        const BilTap b = bil_tap(r, q, H, W);
        const double m00 = M[b.o00] ? 1.0 : 0.0, m01 = M[b.o01] ? 1.0 : 0.0;
        const double m10 = M[b.o10] ? 1.0 : 0.0, m11 = M[b.o11] ? 1.0 : 0.0;
        a = (float)((1.0 - b.fr) * ((1.0 - b.fc) * m00 + b.fc * m01) + b.fr * ((1.0 - b.fc) * m10 + b.fc * m11));
      }
    }
    A[o] = a;
  }
}

// The label and status of every pixel from the carried plane A.  A decided
// pixel (A >= 0) takes A >= 0.5f, OF_MASK_CARRIED.  An undecided one runs the
// (2R + 1)^2 window row by row over its decided in-frame neighbours n:
//   D = (sum over c of (G_c(p) - G_c(n))^2) / C;  z = D / rr;  w = z < 1 ? (1 - z)^2 : 0
//   num += w * A(n); den += w; cnt += 1; ones += A(n) >= 0.5f
// and takes num >= 0.5 den where den > 0, else 2 ones >= cnt where cnt > 0
// (both OF_MASK_VOTED), else 0, OF_MASK_UNKNOWN.  rr = range * range.  One
// workgroup per 32 x 8 tile (gx tiles across, 1-D grid in the XCD-aware
// order).  A workgroup without an undecided pixel, decided once for the block
// through an LDS word, writes its labels and leaves before it loads anything
// else; otherwise the tile and its R-wide halo of A and G go to LDS (positions
// outside the frame as undecided, so the window skips them) and every
// undecided thread runs its window there.  CT = the channel count, or 0 for
// the generic path (C <= MSK_MAX_C at run time); the LDS rows of G hold C
// floats per pixel either way.  status: H x W bytes or nullptr.
template <int CT>
__global__ void __launch_bounds__(MSK_TW *MSK_TH)
k_mask_vote(const float *__restrict__ A, const float *__restrict__ G, int H, int W, int Cr, int R, double rr, int gx,
            uint8_t *__restrict__ label, uint8_t *__restrict__ status) {
  OF_NOCONTRACT
  constexpr int CM = CT ? CT : MSK_MAX_C;
  const int C = CT ? CT : Cr;
  __shared__ float s_a[MSK_LH * MSK_LW];
  __shared__ float s_g[MSK_LH * MSK_LW * MSK_MAX_C];
  __shared__ int s_any;
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int i0 = tyi * MSK_TH, j0 = txi * MSK_TW;
  const int tid = threadIdx.x;
  const int ly = tid / MSK_TW, lx = tid - ly * MSK_TW;
  const int i = i0 + ly, j = j0 + lx;
  const bool own = i < H && j < W;
  const size_t o = own ? (size_t)i * W + j : 0;
  const float a = own ? A[o] : 0.0f;
  const bool undecided = own && a < 0.0f;
  if (tid == 0) s_any = 0;
  __syncthreads();
  if (undecided) s_any = 1;
  __syncthreads();
  if (!s_any) {
    if (own) {
      label[o] = a >= 0.5f ? 1 : 0;
      if (status) status[o] = OF_MASK_CARRIED;
    }
    return;
  }
  const int LW = MSK_TW + 2 * R, LH = MSK_TH + 2 * R;
  for (int e = tid; e < LH * LW; e += MSK_TW * MSK_TH) {
    const int la = e / LW, lb = e - la * LW;
    const int y = i0 - R + la, x = j0 - R + lb;
    float an = MSK_UNDECIDED;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t on = (size_t)y * W + x;
      an = A[on];
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) s_g[e * C + c] = G[on * C + c];
    }
    s_a[e] = an;
  }
  __syncthreads();
  if (!own) return;
  uint8_t lab = a >= 0.5f ? 1 : 0, st = OF_MASK_CARRIED;
  if (undecided) {
    const int ec = (ly + R) * LW + lx + R;
    double gp[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) gp[c] = c < C ? (double)s_g[ec * C + c] : 0.0;
    const double dC = (double)C;
    double num = 0.0, den = 0.0;
    int cnt = 0, ones = 0;
    for (int di = 0; di <= 2 * R; ++di)
      for (int dj = 0; dj <= 2 * R; ++dj) {
        const int en = (ly + di) * LW + lx + dj;
        const float an = s_a[en];
        if (!(an >= 0.0f)) continue;
        double D = 0.0;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) {
            const double d = gp[c] - (double)s_g[en * C + c];
            D = D + d * d;
          }
        const double z = (D / dC) / rr;
        const double w = z < 1.0 ? (1.0 - z) * (1.0 - z) : 0.0;
        num = num + w * (double)an;
        den = den + w;
        cnt += 1;
        ones += an >= 0.5f ? 1 : 0;
      }
    if (den > 0.0) {
      lab = num >= 0.5 * den ? 1 : 0;
      st = OF_MASK_VOTED;
    } else if (cnt > 0) {
      lab = 2 * ones >= cnt ? 1 : 0;
      st = OF_MASK_VOTED;
    } else {
      lab = 0;
      st = OF_MASK_UNKNOWN;
    }
  }
  label[o] = lab;
  if (status) status[o] = st;
}

// out(i, j) = the majority of the labels (0 / 1) in the in-frame part of the
// (2s + 1)^2 window, the pixel's own label on a tie; s = 1..MSK_MAX_S.  One
// workgroup per 32 x 8 tile as in k_mask_vote, the tile and its s-wide halo of
// labels in LDS, positions outside the frame as 2.
__global__ void __launch_bounds__(MSK_TW *MSK_TH)
k_mask_mode(const uint8_t *__restrict__ label, int H, int W, int s, int gx, uint8_t *__restrict__ out) {
  __shared__ uint8_t t[(MSK_TH + 2 * MSK_MAX_S) * (MSK_TW + 2 * MSK_MAX_S)];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int i0 = tyi * MSK_TH, j0 = txi * MSK_TW;
  const int tid = threadIdx.x;
  const int LW = MSK_TW + 2 * s, LH = MSK_TH + 2 * s;
  for (int e = tid; e < LH * LW; e += MSK_TW * MSK_TH) {
    const int la = e / LW, lb = e - la * LW;
    const int y = i0 - s + la, x = j0 - s + lb;
    t[e] = y >= 0 && y < H && x >= 0 && x < W ? label[(size_t)y * W + x] : (uint8_t)2;
  }
  __syncthreads();
  const int ly = tid / MSK_TW, lx = tid - ly * MSK_TW;
  const int i = i0 + ly, j = j0 + lx;
  if (i >= H || j >= W) return;
  int k = 0, n = 0;
  for (int di = 0; di <= 2 * s; ++di)
    for (int dj = 0; dj <= 2 * s; ++dj) {
      const int v = t[(ly + di) * LW + lx + dj];
      k += v == 1 ? 1 : 0;
      n += v != 2 ? 1 : 0;
    }
  const int self = t[(ly + s) * LW + lx + s];
  out[(size_t)i * W + j] = (uint8_t)(2 * k > n ? 1 : (2 * k < n ? 0 : self));
}
