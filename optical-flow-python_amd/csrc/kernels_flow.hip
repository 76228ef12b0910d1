// kernels_flow.hip — what a warping iteration does to the flow field around
// its solve: the update with clip and the occlusion map (k_update_occ,
// k_add_update), the duv bookkeeping (k_axpy_diff, k_sub2, k_lo_blend), the
// forward-backward check of two flows (k_fb_check) and the plain S x S
// medians (k_median1, k_median2).  Expects nothing before it but kernels.h
// and nothing here is used by a later kernel file.  Warp and derivatives are
// in kernels_warp.hip, the assembly in kernels_assemble.hip, the weighted
// median in kernels_wmf.hip.
#include "kernels.h"

// IRLS update: uv1 = uv + clip(x) (classic_nl.py:250-262); with occ != nullptr
// also detect_occlusion(uv1, images) (occlusion.py:6-56), where uv1 at the
// left / upper neighbour is recomputed in-register.
__device__ __forceinline__ float2 upd(const float2 *uv, const float2 *x, size_t k, int clip) {
  float2 a = uv[k], b = x[k];
  if (clip) { b.x = fminf(fmaxf(b.x, -1.0f), 1.0f); b.y = fminf(fmaxf(b.y, -1.0f), 1.0f); }
  return make_float2(a.x + b.x, a.y + b.y);
}

__global__ void k_update_occ(const float2 *__restrict__ uv, const float2 *__restrict__ x, int clip,
                             float2 *__restrict__ uv1, const float *__restrict__ I1, const float *__restrict__ I2,
                             int nc, float *__restrict__ occ, int H, int W, int P, size_t ps) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    const float2 c = upd(uv, x, k, clip);
    uv1[k] = c;
    if (!occ) continue;
    float dudx = j > 0 ? c.x - upd(uv, x, k - 1, clip).x : 0.0f;
    float dvdy = i > 0 ? c.y - upd(uv, x, k - P, clip).y : 0.0f;
    float div = dudx + dvdy;
    float odiv = expf(-div * div * (1.0f / (2.0f * 0.3f * 0.3f)));
    // bilinear warp of frame 2, 0-based, coordinates clamped ('nearest')
    float r = fminf(fmaxf((float)i + c.y, 0.0f), (float)(H - 1));
    float q = fminf(fmaxf((float)j + c.x, 0.0f), (float)(W - 1));
    int i0 = (int)floorf(r), j0 = (int)floorf(q);
    float fr = r - i0, fc = q - j0;
    int i1 = min(i0 + 1, H - 1), j1 = min(j0 + 1, W - 1);
    float it = 0.0f;
    for (int ch = 0; ch < nc; ++ch) {
      const float *b = I2 + ch * ps;
      const float *r0 = b + (size_t)i0 * P, *r1 = b + (size_t)i1 * P;
      float w = (1.0f - fr) * ((1.0f - fc) * r0[j0] + fc * r0[j1]) + fr * ((1.0f - fc) * r1[j0] + fc * r1[j1]);
      it += fabsf(w - I1[ch * ps + k]);
    }
    if (nc > 1) it /= (float)nc;
    occ[k] = odiv * expf(-it * it * (1.0f / (2.0f * 20.0f * 20.0f)));
  }
}

// in-place uv += x (HS, hs.py:130-134), optional clip
__global__ void k_add_update(float2 *__restrict__ uv, const float2 *__restrict__ x, int clip, int H, int W, int P) {
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    uv[k] = upd(uv, x, k, clip);
  }
}

// uv = uv + (b - a): the duv bookkeeping of classic_nl.py:271-275 / ba.py:404-407
__global__ void k_axpy_diff(float2 *__restrict__ uv, const float2 *__restrict__ a, const float2 *__restrict__ b, int H,
                            int W, int P) {
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    float2 u = uv[k], x = a[k], y = b[k];
    uv[k] = make_float2(u.x + (y.x - x.x), u.y + (y.y - x.y));
  }
}

// out = b - a
__global__ void k_sub2(const float2 *__restrict__ a, const float2 *__restrict__ b, float2 *__restrict__ out, int H,
                       int W, int P) {
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    float2 x = a[k], y = b[k];
    out[k] = make_float2(y.x - x.x, y.y - x.y);
  }
}

// uv_tilde = u + lam * (un - u) (denoise_LO, denoising.py:28-29)
__global__ void k_lo_blend(const float2 *__restrict__ u, const float2 *__restrict__ un, float lam,
                           float2 *__restrict__ out, int H, int W, int P) {
  OF_FOR_PIXELS(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    float2 a = u[k], b = un[k];
    out[k] = make_float2(a.x + lam * (b.x - a.x), a.y + lam * (b.y - a.y));
  }
}

// ---------------------------------------------------------------------------
// Forward-backward consistency (Sundaram et al. 2010): follow A at (i, j),
// sample B bilinearly there and test |A + B|^2 against
// alpha1 (|A|^2 + |B|^2) + alpha2.  state 0 consistent, 1 inconsistent /
// occluded, 2 the target leaves the frame (err = +inf).  fp64 from the fp32
// flows with no contraction, in the order include/optflow.h states, so a
// numpy float64 restatement gives the same bits.  The comparisons are written
// so that NaN / Inf targets count as outside.  st / er are dense H x W.
__device__ __forceinline__ void fb_check_px(const float2 *__restrict__ A, const float2 *__restrict__ B, int i, int j,
                                            int H, int W, int P, double alpha1, double alpha2,
                                            uint8_t *__restrict__ st, float *__restrict__ er) {
  OF_NOCONTRACT
  const float2 a = A[(size_t)i * P + j];
  const size_t o = (size_t)i * W + j;
  const double u = a.x, v = a.y;
  const double q = (double)j + u, r = (double)i + v;
  const bool inside = q >= 0.0 && q <= (double)(W - 1) && r >= 0.0 && r <= (double)(H - 1);
  if (!inside) {
    st[o] = 2;
    if (er) er[o] = __builtin_inff();
    return;
  }
  const double qf = floor(q), rf = floor(r);
  const int j0 = (int)qf, i0 = (int)rf;
  const double fc = q - qf, fr = r - rf;
  const int j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1);
  const float2 b00 = B[(size_t)i0 * P + j0], b01 = B[(size_t)i0 * P + j1];
  const float2 b10 = B[(size_t)i1 * P + j0], b11 = B[(size_t)i1 * P + j1];
  const double bu = (1.0 - fr) * ((1.0 - fc) * (double)b00.x + fc * (double)b01.x) +
                    fr * ((1.0 - fc) * (double)b10.x + fc * (double)b11.x);
  const double bv = (1.0 - fr) * ((1.0 - fc) * (double)b00.y + fc * (double)b01.y) +
                    fr * ((1.0 - fc) * (double)b10.y + fc * (double)b11.y);
  const double du = u + bu, dv = v + bv;
  const double err = du * du + dv * dv;
  const double thr = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2;
  st[o] = err > thr ? 1 : 0;
  if (er) er[o] = (float)err;
}

// one thread per pixel; with st_bw != nullptr the same launch also writes the
// backward mask (the roles of fw and bw exchanged)
__global__ void k_fb_check(const float2 *__restrict__ fw, const float2 *__restrict__ bw, int H, int W, int P,
                           double alpha1, double alpha2, uint8_t *__restrict__ st_fw, float *__restrict__ er_fw,
                           uint8_t *__restrict__ st_bw, float *__restrict__ er_bw) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    fb_check_px(fw, bw, i, j, H, W, P, alpha1, alpha2, st_fw, er_fw);
    if (st_bw) fb_check_px(bw, fw, i, j, H, W, P, alpha1, alpha2, st_bw, er_bw);
  }
}

// ---------------------------------------------------------------------------
// scipy.ndimage.median_filter(size=S, mode='reflect'): rank selection with
// index tie-break (the element of rank S*S/2), branch-free.
template <int S>
__device__ __forceinline__ float median_window(const float *a) {
  constexpr int N = S * S;
  float m = a[0];
#pragma unroll
  for (int t = 0; t < N; ++t) {
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < N; ++u) cnt += (a[u] < a[t]) || (a[u] == a[t] && u < t);
    m = cnt == N / 2 ? a[t] : m;
  }
  return m;
}

template <int S>
__global__ __launch_bounds__(OF_BX *OF_BY) void k_median2(const float2 *__restrict__ in, float2 *__restrict__ out, int H, int W, int P) {
  constexpr int h = S / 2;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    float au[S * S], av[S * S];
    int t = 0;
#pragma unroll
    for (int a = -h; a <= h; ++a) {
      const float2 *row = in + (size_t)ext_reflect(i + a, H) * P;
#pragma unroll
      for (int b = -h; b <= h; ++b, ++t) {
        float2 v = row[ext_reflect(j + b, W)];
        au[t] = v.x;
        av[t] = v.y;
      }
    }
    out[(size_t)i * P + j] = make_float2(median_window<S>(au), median_window<S>(av));
  }
}

template <int S>
__global__ __launch_bounds__(OF_BX *OF_BY) void k_median1(const float *__restrict__ in, float *__restrict__ out, int H, int W, int P, size_t ps) {
  constexpr int h = S / 2;
  in += blockIdx.z * ps;
  out += blockIdx.z * ps;
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    float a[S * S];
    int t = 0;
#pragma unroll
    for (int y = -h; y <= h; ++y) {
      const float *row = in + (size_t)ext_reflect(i + y, H) * P;
#pragma unroll
      for (int x = -h; x <= h; ++x, ++t) a[t] = row[ext_reflect(j + x, W)];
    }
    out[(size_t)i * P + j] = median_window<S>(a);
  }
}
template __global__ void k_median2<3>(const float2 *, float2 *, int, int, int);
template __global__ void k_median2<5>(const float2 *, float2 *, int, int, int);
template __global__ void k_median2<7>(const float2 *, float2 *, int, int, int);
template __global__ void k_median1<3>(const float *, float *, int, int, int, size_t);
template __global__ void k_median1<5>(const float *, float *, int, int, int, size_t);
template __global__ void k_median1<7>(const float *, float *, int, int, int, size_t);
