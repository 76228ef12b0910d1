// kernels_warp.hip — warping frame 2 by the flow and the data term's
// derivatives (partial_deriv, derivatives.py:148-296): the interpolation
// bases (hermite, bspline3), one pixel's (It, Ix, Iy) of every channel for the
// three interpolations (warp_pixel) and the kernel that stores them as planes
// (k_partial_deriv).  fp32, no contraction.  Expects nothing before it but
// kernels.h.  kernels_assemble.hip, next, calls warp_pixel with RegOut from
// its fused warp + assembly.  See DESIGN.md for the roofline.
#include "kernels.h"

// cubic Hermite basis (tensor-product form of derivatives.py:7-24's
// 16x16 bicubic coefficient matrix)
__device__ __forceinline__ void hermite(float t, float h[4], float dh[4]) {
  OF_NOCONTRACT
  float t2 = t * t, t3 = t2 * t;
  h[0] = 2.0f * t3 - 3.0f * t2 + 1.0f;
  h[1] = -2.0f * t3 + 3.0f * t2;
  h[2] = t3 - 2.0f * t2 + t;
  h[3] = t3 - t2;
  dh[0] = 6.0f * t2 - 6.0f * t;
  dh[1] = -6.0f * t2 + 6.0f * t;
  dh[2] = 3.0f * t2 - 4.0f * t + 1.0f;
  dh[3] = 3.0f * t2 - 2.0f * t;
}

__device__ __forceinline__ float bspline3(float t) {
  OF_NOCONTRACT
  t = fabsf(t);
  if (t < 1.0f) return 2.0f / 3.0f - t * t + 0.5f * t * t * t;
  if (t < 2.0f) {
    float s = 2.0f - t;
    return s * s * s * (1.0f / 6.0f);
  }
  return 0.0f;
}

// partial_deriv (derivatives.py:148-296) for one pixel and all channels.
// (x2, y2) are the 1-based warped coordinates.  Each channel's (It, Ix, Iy)
// goes to out(c, it, ix, iy): PlaneOut stores it straight to the planes (no
// per-channel register arrays: a runtime-indexed array would live in
// scratch); RegOut<NC> keeps it in registers for the fused warp + assembly
// (NC > 0: the channel loop is unrolled, so the array index is static).
struct PlaneOut {
  float *It, *Ix, *Iy;
  size_t ps, k;
  __device__ __forceinline__ void operator()(int c, float it, float ix, float iy) const {
    It[c * ps + k] = it;
    Ix[c * ps + k] = ix;
    Iy[c * ps + k] = iy;
  }
};
template <int NC>
struct RegOut {
  float it[NC], ix[NC], iy[NC];
  __device__ __forceinline__ void operator()(int c, float a, float b, float e) {
    it[c] = a;
    ix[c] = b;
    iy[c] = e;
  }
};
template <int INTERP, int NC, typename Out>
__device__ __forceinline__ void warp_pixel(const DerivArgs &d, int H, int W, int P, size_t ps, int i, int j, float x2,
                                           float y2, Out &out) {
  OF_NOCONTRACT
  const size_t k = (size_t)i * P + j;
  const int nc = NC > 0 ? NC : d.nc;
  if (INTERP == OF_INTERP_BICUBIC) {
    float fx = floorf(x2), fy = floorf(y2);
    bool oob = (fx < 1.0f) || (fx + 1.0f > (float)W) || (fy < 1.0f) || (fy + 1.0f > (float)H) || !(x2 == x2) ||
               !(y2 == y2);
    int fx0 = (int)fminf(fmaxf(fx, 1.0f), (float)W) - 1, cx0 = (int)fminf(fmaxf(fx + 1.0f, 1.0f), (float)W) - 1;
    int fy0 = (int)fminf(fmaxf(fy, 1.0f), (float)H) - 1, cy0 = (int)fminf(fmaxf(fy + 1.0f, 1.0f), (float)H) - 1;
    float ax = oob ? 0.0f : x2 - fx, ay = oob ? 0.0f : y2 - fy;
    float hx[4], dhx[4], hy[4], dhy[4];
    hermite(ax, hx, dhx);
    hermite(ay, hy, dhy);
    const size_t cs[4] = {(size_t)fy0 * P + fx0, (size_t)fy0 * P + cx0, (size_t)cy0 * P + fx0, (size_t)cy0 * P + cx0};
#pragma unroll
    for (int c = 0; c < nc; ++c) {
      const size_t o = c * ps;
      float v = 0.0f, vx = 0.0f, vy = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xi = q & 1, yi = q >> 1;
        const float z = d.I2[o + cs[q]], dx = d.A[o + cs[q]], dy = d.B[o + cs[q]], dxy = d.Cc[o + cs[q]];
        const float gx = hx[xi], gy = hy[yi], sx = hx[2 + xi], sy = hy[2 + yi];
        v += gx * gy * z + sx * gy * dx + gx * sy * dy + sx * sy * dxy;
        vx += dhx[xi] * gy * z + dhx[2 + xi] * gy * dx + dhx[xi] * sy * dy + dhx[2 + xi] * sy * dxy;
        vy += gx * dhy[yi] * z + sx * dhy[yi] * dx + gx * dhy[2 + yi] * dy + sx * dhy[2 + yi] * dxy;
      }
      if (oob) out(c, 0.0f, 0.0f, 0.0f);
      else
        out(c, v - d.I1[o + k], d.blend * vx + (1.0f - d.blend) * d.I1x[o + k],
            d.blend * vy + (1.0f - d.blend) * d.I1y[o + k]);
    }
  } else {
    const bool outside = (x2 > (float)W) || (x2 < 1.0f) || (y2 > (float)H) || (y2 < 1.0f) || !(x2 == x2) || !(y2 == y2);
    if (outside) {
#pragma unroll
      for (int c = 0; c < nc; ++c) out(c, 0.0f, 0.0f, 0.0f);
      return;
    }
    const float r = y2 - 1.0f, q = x2 - 1.0f;
    if (INTERP == OF_INTERP_CUBIC) {
      const int i0 = (int)floorf(r), j0 = (int)floorf(q);
      float wr[4], wc[4];
      int rr[4], cc[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        wr[a] = bspline3(r - (float)(i0 + a - 1));
        wc[a] = bspline3(q - (float)(j0 + a - 1));
        rr[a] = ext_mirror(i0 + a - 1, H);
        cc[a] = ext_mirror(j0 + a - 1, W);
      }
#pragma unroll
      for (int c = 0; c < nc; ++c) {
        const size_t o = c * ps;
        float v = 0.0f, vx = 0.0f, vy = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float tv = 0.0f, tx = 0.0f, ty = 0.0f;
          const size_t rb = o + (size_t)rr[a] * P;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            tv += wc[b] * d.Cc[rb + cc[b]];
            tx += wc[b] * d.A[rb + cc[b]];
            ty += wc[b] * d.B[rb + cc[b]];
          }
          v += wr[a] * tv;
          vx += wr[a] * tx;
          vy += wr[a] * ty;
        }
        out(c, v - d.I1[o + k], d.blend * vx + (1.0f - d.blend) * d.I1x[o + k],
            d.blend * vy + (1.0f - d.blend) * d.I1y[o + k]);
      }
    } else {  // bi-linear
      int i0 = (int)floorf(r), j0 = (int)floorf(q);
      float fr = r - i0, fc = q - j0;
      int i1 = min(i0 + 1, H - 1), j1 = min(j0 + 1, W - 1);
#pragma unroll
      for (int c = 0; c < nc; ++c) {
        const size_t o = c * ps;
        auto bil = [&](const float *p) {
          const float *r0 = p + o + (size_t)i0 * P, *r1 = p + o + (size_t)i1 * P;
          return (1.0f - fr) * ((1.0f - fc) * r0[j0] + fc * r0[j1]) + fr * ((1.0f - fc) * r1[j0] + fc * r1[j1]);
        };
        out(c, bil(d.I2) - d.I1[o + k], d.blend * bil(d.A) + (1.0f - d.blend) * d.I1x[o + k],
            d.blend * bil(d.B) + (1.0f - d.blend) * d.I1y[o + k]);
      }
    }
  }
}


// launch bounds = the grid2 block (64 x 4): without them the compiler
// assumes 1024-thread blocks, caps VGPRs at 128 and spills to scratch
template <int INTERP>
__global__ __launch_bounds__(OF_BX *OF_BY) void k_partial_deriv(DerivArgs d, const float2 *__restrict__ uv, int H,
                                                                int W, int P, size_t ps, float *__restrict__ It,
                                                                float *__restrict__ Ix, float *__restrict__ Iy) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    float2 f = uv[k];
    PlaneOut out{It, Ix, Iy, ps, k};
    warp_pixel<INTERP, 0>(d, H, W, P, ps, i, j, (float)(j + 1) + f.x, (float)(i + 1) + f.y, out);
  }
}
template __global__ void k_partial_deriv<0>(DerivArgs, const float2 *, int, int, int, size_t, float *, float *, float *);
template __global__ void k_partial_deriv<1>(DerivArgs, const float2 *, int, int, int, size_t, float *, float *, float *);
template __global__ void k_partial_deriv<2>(DerivArgs, const float2 *, int, int, int, size_t, float *, float *, float *);
