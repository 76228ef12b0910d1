// kernels_upsample.hip — reduced-resolution flow: the box reduction of a frame
// (k_reduce_frame) and the edge-aware upsampling of a low-resolution flow
// guided by the full-resolution frame (k_flow_upsample).  Frames are dense
// H x W x C interleaved fp32, flows pitched float2.  All arithmetic in fp64
// from the fp32 inputs with no contraction, in the order include/optflow.h
// states (of_reduce_frame, of_flow_upsample), so a numpy float64 restatement
// gives the same bits.  H * W < 2^31 (checked on the host).
#include "kernels.h"

#define UP_MAX_C 4   // channels
#define UP_MIN_S 2   // scales
#define UP_MAX_S 4
#define UP_TW 64     // output tile: 64 x 8 pixels, 256 threads, two rows each
#define UP_TH 8
// The low-resolution footprint of a tile of n output pixels along one axis:
// a0 = floor((i - 0.5*(s-1))/s) takes at most ceil(n/s) + 1 values (the
// half-pixel phase splits one low pixel between two tiles for even s), and the
// taps reach from a0-1 to a0+2: ceil(n/s) + 4 entries, most at s = 2.
#define UP_FH (UP_TH / UP_MIN_S + 4)
#define UP_FW (UP_TW / UP_MIN_S + 4)

// One thread per low-resolution pixel, all its channels: the s x s block (cut
// at the frame's edge) summed row-major from +0.0.  Along a row consecutive
// threads read consecutive runs of s*C floats.
__global__ void __launch_bounds__(OF_BX *OF_BY)
k_reduce_frame(const float *__restrict__ im, int H, int W, int C, int s, int hs, int ws, float *__restrict__ out) {
  OF_NOCONTRACT
  OF_FOR_PIXELS(hs, ws) {
    if (j >= ws) continue;
    const int i1 = min(i * s + s, H), j1 = min(j * s + s, W);
    double S[UP_MAX_C] = {0.0, 0.0, 0.0, 0.0};
    for (int y = i * s; y < i1; ++y)
      for (int x = j * s; x < j1; ++x) {
        const float *p = im + ((size_t)y * W + x) * C;
#pragma unroll
        for (int c = 0; c < UP_MAX_C; ++c)
          if (c < C) S[c] = S[c] + (double)p[c];
      }
    const double m = (double)((i1 - i * s) * (j1 - j * s));
    float *o = out + ((size_t)i * ws + j) * C;
#pragma unroll
    for (int c = 0; c < UP_MAX_C; ++c)
      if (c < C) o[c] = (float)(S[c] / m);
  }
}

// floor(n/d) for d > 0
__device__ __forceinline__ int up_floor_div(int n, int d) {
  const int q = n / d;
  return (n % d != 0 && n < 0) ? q - 1 : q;
}
// a0 of output index i: floor((i - 0.5*(s-1))/s), in integers (the double
// quotient of the kernel body is an exact multiple of 1/(2s) away from every
// integer it does not hit, so both floors agree)
__device__ __forceinline__ int up_a0(int i, int s) { return up_floor_div(2 * i - (s - 1), 2 * s); }

// One workgroup per 64 x 8 output tile (gx tiles across, 1-D grid in the
// XCD-aware order).  The tile's low-resolution footprint -- the low guide's C
// floats and the low flow of at most UP_FH x UP_FW low pixels -- is staged in
// LDS once; an entry outside the low frame gets a NaN flow, which the taps
// skip as they skip a flow that is not finite.  Every thread then handles the
// pixels (ly, lx) and (ly + 4, lx) of the tile: G is read once, coalesced, and
// the 16 taps read LDS only.  CT = the channel count, or 0 for the generic
// path (C <= UP_MAX_C at run time).  ch2 = C*h2.  No atomics, no scratch.
template <int CT>
__global__ void __launch_bounds__(256)
k_flow_upsample(const float2 *__restrict__ f, int Pl, const float *__restrict__ L, const float *__restrict__ G, int H,
                int W, int hs, int ws, int Cr, int s, double ch2, int gx, float2 *__restrict__ out, int P,
                uint8_t *__restrict__ info) {
  OF_NOCONTRACT
  constexpr int CM = CT ? CT : UP_MAX_C;
  const int C = CT ? CT : Cr;
  __shared__ float2 s_f[UP_FH * UP_FW];
  __shared__ float s_L[UP_FH * UP_FW * CM];
  const int tile = of_xcd_tile(blockIdx.x, gridDim.x);
  const int tyi = tile / gx, txi = tile - tyi * gx;
  const int i0 = tyi * UP_TH, j0 = txi * UP_TW;
  const int tid = threadIdx.x;
  const int a_lo = up_a0(i0, s) - 1, b_lo = up_a0(j0, s) - 1;
  const int fh = up_a0(i0 + UP_TH - 1, s) + 2 - a_lo + 1, fw = up_a0(j0 + UP_TW - 1, s) + 2 - b_lo + 1;
  const float nanf_ = __builtin_nanf("");
  for (int e = tid; e < fh * fw; e += 256) {
    const int la = e / fw, lb = e - la * fw;
    const int a = a_lo + la, b = b_lo + lb;
    const bool in = a >= 0 && a < hs && b >= 0 && b < ws;
    s_f[e] = in ? f[(size_t)a * Pl + b] : make_float2(nanf_, nanf_);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) s_L[e * CM + c] = in ? L[((size_t)a * ws + b) * C + c] : 0.0f;
  }
  __syncthreads();
  const int lx = tid & (UP_TW - 1), ly = tid >> 6;
  const int j = j0 + lx;
  if (j >= W) return;
  const double ds = (double)s, half = 0.5 * (double)(s - 1);
  const double q = ((double)j - half) / ds;
  const int b0 = (int)floor(q);
  double wb[4];
#pragma unroll
  for (int tb = 0; tb < 4; ++tb) {
    const double t = 1.0 - fabs((double)(b0 - 1 + tb) - q) / 2.0;
    wb[tb] = t > 0.0 ? t : 0.0;
  }
#pragma unroll
  for (int hr = 0; hr < 2; ++hr) {
    const int i = i0 + ly + hr * (UP_TH / 2);
    if (i >= H) continue;
    const size_t o = (size_t)i * W + j;
    double g[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) g[c] = c < C ? (double)G[o * C + c] : 0.0;
    const double r = ((double)i - half) / ds;
    const int a0 = (int)floor(r);
    double U = 0.0, V = 0.0, Sw = 0.0, Us = 0.0, Vs = 0.0, Ss = 0.0;
#pragma unroll
    for (int ta = 0; ta < 4; ++ta) {
      const int a = a0 - 1 + ta;
      const double t = 1.0 - fabs((double)a - r) / 2.0;
      const double wa = t > 0.0 ? t : 0.0;
      const int row = (a - a_lo) * fw + (b0 - 1 - b_lo);
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) {
        const int e = row + tb;
        const float2 fl = s_f[e];
        if (!(__builtin_isfinite(fl.x) && __builtin_isfinite(fl.y))) continue;
        const double fx = fl.x, fy = fl.y;
        const double wsp = wa * wb[tb];
        double D = 0.0;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) {
            const double d = g[c] - (double)s_L[e * CM + c];
            D = D + d * d;
          }
        const double z = D / ch2;
        const double x = z < 1.0 ? z : 1.0;
        const double wr = (1.0 - x) * (1.0 - x);
        const double w = wsp * wr;
        U = U + w * fx;
        V = V + w * fy;
        Sw = Sw + w;
        Us = Us + wsp * fx;
        Vs = Vs + wsp * fy;
        Ss = Ss + wsp;
      }
    }
    float2 res;
    uint8_t inf;
    if (Sw > 0.0) {
      res = make_float2((float)(ds * (U / Sw)), (float)(ds * (V / Sw)));
      inf = 0;
    } else if (Ss > 0.0) {
      res = make_float2((float)(ds * (Us / Ss)), (float)(ds * (Vs / Ss)));
      inf = 1;
    } else {
      res = make_float2(nanf_, nanf_);
      inf = 2;
    }
    out[(size_t)i * P + j] = res;
    if (info) info[o] = inf;
  }
}
