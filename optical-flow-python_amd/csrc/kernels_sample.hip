// kernels_sample.hip — the clamped bilinear sample in fp64 that everything
// after the flow stage shares: the taps of a point (BilTap, bil_tap), a
// channel of a dense interleaved frame (bil_at) or both components of a
// pitched flow (bil2) at those taps, and the in-frame test (in_frame).  No
// contraction, one fixed order of operations, so a numpy float64 restatement
// gives the same bits.  Device functions only, no kernel; expects nothing
// before it but kernels.h.  Used by kernels_interp.hip, kernels_track.hip,
// kernels_fuse.hip, kernels_noise.hip, kernels_sr.hip, kernels_inpaint.hip,
// kernels_mask.hip and kernels_motion.hip, all included after this file.
#include "kernels.h"

// the four taps and two fractions of the clamped bilinear sample at (r, q),
// both finite; offsets in pixels of a dense H x W plane
struct BilTap {
  size_t o00, o01, o10, o11;
  double fc, fr;
};
__device__ __forceinline__ BilTap bil_tap(double r, double q, int H, int W) {
  OF_NOCONTRACT
  const double qc = fmin(fmax(q, 0.0), (double)(W - 1)), rc = fmin(fmax(r, 0.0), (double)(H - 1));
  const double qf = floor(qc), rf = floor(rc);
  const int j0 = (int)qf, i0 = (int)rf;
  const int j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1);
  BilTap b;
  b.fc = qc - qf;
  b.fr = rc - rf;
  b.o00 = (size_t)i0 * W + j0;
  b.o01 = (size_t)i0 * W + j1;
  b.o10 = (size_t)i1 * W + j0;
  b.o11 = (size_t)i1 * W + j1;
  return b;
}
// channel ch of an interleaved C-channel frame at the taps
__device__ __forceinline__ double bil_at(const float *__restrict__ A, int C, int ch, const BilTap &b) {
  OF_NOCONTRACT
  const double a00 = A[b.o00 * C + ch], a01 = A[b.o01 * C + ch], a10 = A[b.o10 * C + ch], a11 = A[b.o11 * C + ch];
  return (1.0 - b.fr) * ((1.0 - b.fc) * a00 + b.fc * a01) + b.fr * ((1.0 - b.fc) * a10 + b.fc * a11);
}
// offset o of a dense H x W plane (bil_tap's) in the plane pitched to P
__device__ __forceinline__ size_t bil_pitched(size_t o, int W, int P) {
  return o + (size_t)((unsigned)o / (unsigned)W) * (size_t)(P - W);
}
// both components of a pitched flow at the taps
__device__ __forceinline__ void bil2(const float2 *__restrict__ A, int W, int P, const BilTap &b, double &u,
                                     double &v) {
  OF_NOCONTRACT
  const float2 a00 = A[bil_pitched(b.o00, W, P)], a01 = A[bil_pitched(b.o01, W, P)];
  const float2 a10 = A[bil_pitched(b.o10, W, P)], a11 = A[bil_pitched(b.o11, W, P)];
  u = (1.0 - b.fr) * ((1.0 - b.fc) * (double)a00.x + b.fc * (double)a01.x) +
      b.fr * ((1.0 - b.fc) * (double)a10.x + b.fc * (double)a11.x);
  v = (1.0 - b.fr) * ((1.0 - b.fc) * (double)a00.y + b.fc * (double)a01.y) +
      b.fr * ((1.0 - b.fc) * (double)a10.y + b.fc * (double)a11.y);
}
__device__ __forceinline__ bool in_frame(double r, double q, int H, int W) {
  return q >= 0.0 && q <= (double)(W - 1) && r >= 0.0 && r <= (double)(H - 1);
}
