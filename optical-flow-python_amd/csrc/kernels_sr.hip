// kernels_sr.hip — multi-frame super-resolution along the flow: a frame and
// its neighbours resampled onto a grid s times finer, every neighbour's taps
// placed where its flow says they belong (k_super_resolve), and one
// back-projection step against the frame (k_sr_back).  Frames are dense
// H x W x C interleaved fp32, flows pitched float2, the neighbour weights n
// dense H x W fp32 planes (k_fuse_weights, kernels_fuse.hip, whose FuseArgs
// and limits on n and C hold here too).  All arithmetic in fp64 from the
// fp32 inputs with no contraction, in the order include/optflow.h states
// (of_super_resolve), so a numpy float64 restatement gives the same bits.
// s*s*H*W < 2^31 (checked on the host).  Expects kernels_sample.hip before
// it (in_frame).
#include "kernels.h"

#define SR_MIN_S 2   // factors
#define SR_MAX_S 4
#define SR_TW 32     // output tile: 32 x 8 pixels, one thread each (four waves)
#define SR_TH 8
// The low-resolution footprint of a tile of n output pixels along one axis:
// ic = Y/s takes at most ceil((n-1)/s) + 1 values, n/2 at s = 2 (a tile starts
// on a multiple of n, which is even) and fewer beyond; the centre's taps, the
// flow's bilinear taps and the weight reach from ic-1 to ic+1: n/2 + 2 entries
// at most, one more kept.
#define SR_FH (SR_TH / SR_MIN_S + 3)
#define SR_FW (SR_TW / SR_MIN_S + 3)
#define SR_FP (SR_FH * SR_FW)

// The 3 x 3 taps of one frame around (zr, zq), row-major: positions outside
// the frame and taps at x >= 1 skipped, the others added to acc and S with
// weight K*R.  `at(a, b, c)` reads channel c of the frame at (a, b).
template <int CM, typename At>
__device__ __forceinline__ void sr_taps(double zr, double zq, double R, double rho2, int H, int W, int C, At at,
                                        double (&acc)[CM], double &S) {
  OF_NOCONTRACT
  const int a0 = (int)floor(zr + 0.5), b0 = (int)floor(zq + 0.5);
#pragma unroll
  for (int ta = -1; ta <= 1; ++ta) {
    const int a = a0 + ta;
    if (a < 0 || a >= H) continue;
    const double dy = (double)a - zr;
#pragma unroll
    for (int tb = -1; tb <= 1; ++tb) {
      const int b = b0 + tb;
      if (b < 0 || b >= W) continue;
      const double dx = (double)b - zq;
      const double x = (dy * dy + dx * dx) / rho2;
      if (!(x < 1.0)) continue;
      const double K = (1.0 - x) * (1.0 - x);
      const double w = K * R;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) acc[c] = acc[c] + w * at(a, b, c);
      S = S + w;
    }
  }
}

// One workgroup per 32 x 8 output tile (gx tiles across, 1-D grid in the
// XCD-aware order), one thread per output pixel.  What does not depend on the
// flow is staged in LDS once: the tile's low-resolution footprint of the
// centre frame, of every neighbour's flow and of every neighbour's weight
// (entries outside the frame are never read: the taps skip them and bil
// clamps).  The neighbours' own taps are gathers from global memory.  CT = the
// channel count, or 0 for the generic path (C <= FUSE_MAX_C at run time).  A:
// the neighbours as k_fuse_weights took them (the states are in Wk already);
// Wk: n dense H x W planes, or nullptr for n = 0.  No atomics.
template <int CT>
__global__ void __launch_bounds__(SR_TW *SR_TH)
k_super_resolve(const float *__restrict__ I, FuseArgs A, const float *__restrict__ Wk, int n, int H, int W, int P,
                int Cr, int s, double rho2, int gx, float *__restrict__ out, float *__restrict__ out_s) {
  OF_NOCONTRACT
  constexpr int CM = CT ? CT : FUSE_MAX_C;
  const int C = CT ? CT : Cr;
  __shared__ float s_c[SR_FP * CM];
  __shared__ float2 s_f[FUSE_MAX_N * SR_FP];
  __shared__ float s_w[FUSE_MAX_N * SR_FP];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int Y0 = tyi * SR_TH, X0 = txi * SR_TW;
  const int tid = threadIdx.x;
  const int a_lo = Y0 / s - 1, b_lo = X0 / s - 1;
  const int fh = (Y0 + SR_TH - 1) / s + 1 - a_lo + 1, fw = (X0 + SR_TW - 1) / s + 1 - b_lo + 1;  // <= SR_FH, SR_FW
  const size_t px = (size_t)H * W;
  for (int e = tid; e < fh * fw; e += SR_TW * SR_TH) {
    const int la = e / fw, lb = e - la * fw;
    const int a = a_lo + la, b = b_lo + lb;
    const bool in = a >= 0 && a < H && b >= 0 && b < W;
    const size_t o = in ? (size_t)a * W + b : 0;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) s_c[e * CM + c] = in ? I[o * C + c] : 0.0f;
    for (int k = 0; k < n; ++k) {
      s_f[k * SR_FP + e] = in ? A.flow[k][(size_t)a * P + b] : make_float2(0.0f, 0.0f);
      s_w[k * SR_FP + e] = in ? Wk[(size_t)k * px + o] : 0.0f;
    }
  }
  __syncthreads();
  const int ly = tid / SR_TW, lx = tid - ly * SR_TW;
  const int Y = Y0 + ly, X = X0 + lx;
  const int sH = s * H, sW = s * W;
  if (Y >= sH || X >= sW) return;
  const double ds = (double)s, half = 0.5 * (double)(s - 1);
  const double r = ((double)Y - half) / ds, q = ((double)X - half) / ds;
  const int ic = Y / s, jc = X / s;
  double acc[CM], S = 0.0;
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.0;
  // the centre frame, from LDS
  sr_taps<CM>(r, q, 1.0, rho2, H, W, C,
              [&](int a, int b, int c) { return (double)s_c[((a - a_lo) * fw + (b - b_lo)) * CM + c]; }, acc, S);
  // bil's taps at (r, q), the same for every neighbour's flow
  const double qc = fmin(fmax(q, 0.0), (double)(W - 1)), rc = fmin(fmax(r, 0.0), (double)(H - 1));
  const double qf = floor(qc), rf = floor(rc);
  const int j0 = (int)qf, i0 = (int)rf;
  const int j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1);
  const double fc = qc - qf, fr = rc - rf;
  const int e00 = (i0 - a_lo) * fw + (j0 - b_lo), e01 = (i0 - a_lo) * fw + (j1 - b_lo);
  const int e10 = (i1 - a_lo) * fw + (j0 - b_lo), e11 = (i1 - a_lo) * fw + (j1 - b_lo);
  const int ec = (ic - a_lo) * fw + (jc - b_lo);
  for (int k = 0; k < n; ++k) {
    const double R = (double)s_w[k * SR_FP + ec];
    if (R == 0.0) continue;
    const float2 *f = s_f + k * SR_FP;
    const float2 f00 = f[e00], f01 = f[e01], f10 = f[e10], f11 = f[e11];
    const double u = (1.0 - fr) * ((1.0 - fc) * (double)f00.x + fc * (double)f01.x) +
                     fr * ((1.0 - fc) * (double)f10.x + fc * (double)f11.x);
    const double v = (1.0 - fr) * ((1.0 - fc) * (double)f00.y + fc * (double)f01.y) +
                     fr * ((1.0 - fc) * (double)f10.y + fc * (double)f11.y);
    const double zr = r + v, zq = q + u;
    if (!in_frame(zr, zq, H, W)) continue;  // a NaN compares false: skipped too
    const float *__restrict__ N = A.neigh[k];
    sr_taps<CM>(zr, zq, R, rho2, H, W, C, [&](int a, int b, int c) { return (double)N[((size_t)a * W + b) * C + c]; },
                acc, S);
  }
  const size_t o = (size_t)Y * sW + X;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) out[o * C + c] = (float)(acc[c] / S);
  if (out_s) out_s[o] = (float)S;
}

// One back-projection step: out += back * (I - L) of the low-resolution pixel
// the output pixel lies in, L = the box reduction of out (dense H x W x C).
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_sr_back(const float *__restrict__ I, const float *__restrict__ L, int sH, int sW, int W, int C, int s, double back,
          float *__restrict__ out) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(sH, sW) {
    if (j >= sW) continue;
    const size_t lo = (size_t)(i / s) * W + j / s, o = (size_t)i * sW + j;
    for (int c = 0; c < C; ++c) {
      const double e = (double)I[lo * C + c] - (double)L[lo * C + c];
      out[o * C + c] = (float)((double)out[o * C + c] + back * e);
    }
  }
}
