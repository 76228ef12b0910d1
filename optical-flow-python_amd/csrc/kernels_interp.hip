// kernels_interp.hip — image warping (k_warp_image) and occlusion-aware frame
// interpolation (Baker et al. 2011 sec. 3.3.2) from the two flows of a pair
// and their forward-backward states: splat, resolve, fill, render
// (k_interp_*).  Frames are dense H x W x C interleaved fp32, flows pitched
// float2, keys / states / hole marks / info dense H x W.  All arithmetic in
// fp64 from the fp32 inputs with no contraction, in the order
// include/optflow.h states (of_interp_frames), so a numpy float64 restatement
// gives the same bits.  Expects kernels_sample.hip before it (in_frame,
// bil_tap, bil_at); nothing here is used by a later kernel file.
#include "kernels.h"

// out(i, j, c) = im_c sampled at (i + v, j + u); valid = the sample point is
// inside the frame; a non-finite flow gives valid 0 and out 0
__global__ void k_warp_image(const float *__restrict__ im, int C, const float2 *__restrict__ uv, int H, int W, int P,
                             float *__restrict__ out, uint8_t *__restrict__ valid) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const float2 g = uv[(size_t)i * P + j];
    const size_t o = (size_t)i * W + j;
    const bool fin = __builtin_isfinite(g.x) && __builtin_isfinite(g.y);
    const double r = (double)i + (double)g.y, q = (double)j + (double)g.x;
    if (valid) valid[o] = fin && in_frame(r, q, H, W) ? 1 : 0;
    if (!fin) {
      for (int ch = 0; ch < C; ++ch) out[o * C + ch] = 0.0f;
      continue;
    }
    const BilTap b = bil_tap(r, q, H, W);
    for (int ch = 0; ch < C; ++ch) out[o * C + ch] = (float)bil_at(im, C, ch, b);
  }
}

// Splat: source pixel (i, j) of frame f (blockIdx.z; 0: the forward flow of
// frame 1, 1: the backward flow of frame 2) moves to its position at time t
// and offers its motion to the up to four pixels around it.  An offer's cost
// is the photoconsistency of that motion at the target; the smallest
// (cost, frame, source) key wins by a 64-bit atomicMin, whatever the order of
// arrival.  key: H x W, preset to all ones.
__device__ __forceinline__ void interp_splat_px(const float *__restrict__ I1, const float *__restrict__ I2, int C,
                                                const float2 *__restrict__ flow, int f, int i, int j, int H, int W,
                                                int P, double t, double omt,
                                                unsigned long long *__restrict__ key) {
  OF_NOCONTRACT
  const float2 g = flow[(size_t)i * P + j];
  if (!(__builtin_isfinite(g.x) && __builtin_isfinite(g.y))) return;
  const double u = g.x, v = g.y;
  const double a = f ? (double)-g.x : u, b = f ? (double)-g.y : v, tau = f ? omt : t;
  const double q = (double)j + tau * u, r = (double)i + tau * v;
  const double jf = floor(q), i_f = floor(r);
  const double ta = t * a, tb = t * b, oa = omt * a, ob = omt * b;
  const unsigned long long src = ((unsigned long long)f << 31) | (unsigned long long)((size_t)i * W + j);
#pragma unroll
  for (int di = 0; di < 2; ++di)
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      const double tid = i_f + (double)di, tjd = jf + (double)dj;
      if (!in_frame(tid, tjd, H, W)) continue;                 // in double: the flow may be huge
      if ((dj == 1 && q == jf) || (di == 1 && r == i_f)) continue;  // zero bilinear weight
      const BilTap b1 = bil_tap(tid - tb, tjd - ta, H, W), b2 = bil_tap(tid + ob, tjd + oa, H, W);
      double cost = 0.0;
      for (int ch = 0; ch < C; ++ch) cost = cost + fabs(bil_at(I1, C, ch, b1) - bil_at(I2, C, ch, b2));
      const unsigned long long k = ((unsigned long long)__float_as_uint((float)cost) << 32) | src;
      atomicMin(&key[(size_t)(int)tid * W + (int)tjd], k);
    }
}
__global__ void k_interp_splat(const float *__restrict__ I1, const float *__restrict__ I2, int C,
                               const float2 *__restrict__ fw, const float2 *__restrict__ bw, int H, int W, int P,
                               double t, double omt, unsigned long long *__restrict__ key) {
  const int f = blockIdx.z;
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    interp_splat_px(I1, I2, C, f ? bw : fw, f, i, j, H, W, P, t, omt, key);
  }
}

// hole marks: 0 the motion was splatted, 1 filled from neighbours, 2 unknown
#define OF_HOLE 2
// adds the wave's sum of n to *cnt (every lane of the wave calls it)
__device__ __forceinline__ void wave_count(unsigned n, unsigned *cnt) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt, n);
}

// the winner's motion at time t per target (the backward flow negated), or a
// hole where nothing arrived; *cnt += holes
__global__ void k_interp_resolve(const unsigned long long *__restrict__ key, const float2 *__restrict__ fw,
                                 const float2 *__restrict__ bw, int H, int W, int P, float2 *__restrict__ ut,
                                 uint8_t *__restrict__ hole, unsigned *__restrict__ cnt) {
  unsigned n = 0;
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j;
    const unsigned long long k = key[o];
    if (k == ~0ull) {
      hole[o] = OF_HOLE;
      ++n;
      continue;
    }
    const unsigned s = (unsigned)k & 0x7fffffffu;
    const size_t so = (size_t)(s / (unsigned)W) * P + s % (unsigned)W;
    float2 m;
    if (k & 0x80000000ull) {
      const float2 g = bw[so];
      m = make_float2(-g.x, -g.y);
    } else {
      m = fw[so];
    }
    ut[(size_t)i * P + j] = m;
    hole[o] = 0;
  }
  wave_count(n, cnt);
}

// one Jacobi pass of the hole filling: a hole with known pixels among its 8
// neighbours in `hole0` takes their mean (fp64 sum in row-major order, divided
// by the count, rounded to fp32); everything else is copied.  *cnt += holes left
__global__ void k_interp_fill(const float2 *__restrict__ ut0, const uint8_t *__restrict__ hole0,
                              float2 *__restrict__ ut1, uint8_t *__restrict__ hole1, int H, int W, int P,
                              unsigned *__restrict__ cnt) {
  OF_NOCONTRACT
  unsigned n = 0;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j, k = (size_t)i * P + j;
    const uint8_t h = hole0[o];
    if (h != OF_HOLE) {
      ut1[k] = ut0[k];
      hole1[o] = h;
      continue;
    }
    double su = 0.0, sv = 0.0;
    int m = 0;
    for (int di = -1; di <= 1; ++di)
      for (int dj = -1; dj <= 1; ++dj) {
        const int y = i + di, x = j + dj;
        if (y < 0 || y >= H || x < 0 || x >= W || hole0[(size_t)y * W + x] == OF_HOLE) continue;
        const float2 g = ut0[(size_t)y * P + x];
        su = su + (double)g.x;
        sv = sv + (double)g.y;
        ++m;
      }
    if (m) {
      ut1[k] = make_float2((float)(su / (double)m), (float)(sv / (double)m));
      hole1[o] = 1;
    } else {
      hole1[o] = OF_HOLE;
      ++n;
    }
  }
  wave_count(n, cnt);
}

// the frame at time t: both frames sampled along the motion ut of the pixel,
// a sample dropped where the other frame's forward-backward state says its
// point is not visible there.  info: 0 blend, 1 frame 1 only, 2 frame 2 only,
// 3 neither trusted (blend), | 4 the motion was filled.  A pixel whose motion
// is still unknown (no finite flow reached any pixel) is the blend at zero
// motion with info 3.
__global__ void k_interp_render(const float *__restrict__ I1, const float *__restrict__ I2, int C,
                                const float2 *__restrict__ ut, const uint8_t *__restrict__ hole,
                                const uint8_t *__restrict__ sf, const uint8_t *__restrict__ sb, int H, int W, int P,
                                double t, double omt, float *__restrict__ out, uint8_t *__restrict__ info) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j;
    const uint8_t h = hole[o];
    const float2 g = ut[(size_t)i * P + j];
    const double a = g.x, b = g.y;
    const double r1 = (double)i - t * b, q1 = (double)j - t * a;
    const double r2 = (double)i + omt * b, q2 = (double)j + omt * a;
    const bool in1 = in_frame(r1, q1, H, W), in2 = in_frame(r2, q2, H, W);
    auto near = [](double x, int n) { return (int)fmin(fmax(floor(x + 0.5), 0.0), (double)(n - 1)); };
    const bool o1 = in1 && sf[(size_t)near(r1, H) * W + near(q1, W)] == 1;
    const bool o2 = in2 && sb[(size_t)near(r2, H) * W + near(q2, W)] == 1;
    const bool w1 = in1 && !o2 && h != OF_HOLE, w2 = in2 && !o1 && h != OF_HOLE;
    const BilTap b1 = bil_tap(r1, q1, H, W), b2 = bil_tap(r2, q2, H, W);
    for (int ch = 0; ch < C; ++ch) {
      const double s1 = bil_at(I1, C, ch, b1), s2 = bil_at(I2, C, ch, b2);
      out[o * C + ch] = (float)(w1 == w2 ? omt * s1 + t * s2 : (w1 ? s1 : s2));
    }
    info[o] = (uint8_t)((w1 && w2 ? 0 : (w1 ? 1 : (w2 ? 2 : 3))) | (h == 1 ? 4 : 0));
  }
}
