// kernels_motion.hip — global (camera) motion from a dense flow and the
// affine warp that removes it: the thirteen weighted sums of one pass of the
// robust parametric fit per 8 x 64 tile (k_motion_part), their reduction by
// the group tree (k_motion_group, k_motion_final), the closed-form solve and
// the cutoff update in one lane (k_motion_final), and sampling a frame
// through a 2 x 3 matrix (k_warp_affine).  Flows are pitched float2, weights
// dense H x W fp32, states dense H x W bytes in of_fb_consistency's encoding,
// frames dense H x W x C interleaved fp32.  All arithmetic in fp64 from the
// fp32 inputs with no contraction, in the order include/optflow.h states
// (of_fit_motion, of_warp_affine), so a numpy float64 restatement gives the
// same bits.  Every sum runs in one fixed order (rows of a tile ascending,
// the halving tree over its 64 columns, the same tree over groups of 64 tiles)
// whatever the launch geometry: no atomics, nothing that depends on the order
// of arrival.  H * W < 2^31 (checked on the host).
// The arithmetic of a fit pass is stated once, here: the reset of a state
// (mot_reset), the tile mapping (MOT_TILE), the usable-sample test
// (mot_usable) and the closed-form solve (mot_solve) are what
// kernels_layers.hip, included after this file, uses as well.  Expects
// kernels_sample.hip before it (in_frame, bil_tap, bil_at: k_warp_affine).
#include "kernels.h"

#define MOT_NS 13     // sums per pass: Sw Sx Sy Sxx Sxy Syy Su Sxu Syu Sv Sxv Syv Sr
#define MOT_TH 8      // tile: 8 rows x 64 columns, one wave
#define MOT_TW 64
#define MOT_WAVES 4   // tiles (waves) per block

// the passes of a fit: least squares, a Tukey-weighted pass, and the last one,
// which weighs like a Tukey pass, writes the inlier plane and does not solve
#define MOT_PASS_FIRST 0
#define MOT_PASS_ROBUST 1
#define MOT_PASS_LAST 2

// a fit's state between its launches (device memory; read back once at the end)
struct MotionState {
  double th[6];
  double c2;             // squared cutoff of the next Tukey pass
  double sums[MOT_NS];   // of the pass reduced last
  int32_t passes;        // solving passes run
  int32_t degenerate;    // 1: a pass lost rank and solved the translation; 2: no support, the fit stopped
  int32_t stop;
  int32_t pad_;
};

// the normalised coordinates of a frame: x = (j - cx)/s, y = (i - cy)/s
struct MotionFrame {
  double s, cx, cy;
};

// the halving tree over the 64 lanes: s[l] = s[l] + s[l + d] for l < d,
// d = 32 .. 1; lane 0 ends with the sum (lanes >= d hold values nobody reads)
__device__ __forceinline__ double mot_tree(double v) {
  OF_NOCONTRACT
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
  return v;
}

// a fit's state before its first pass: nothing solved, the cutoff c2; stop 1
// leaves the fit stopped, so that passes queued behind it do nothing
__device__ __forceinline__ void mot_reset(MotionState *__restrict__ ms, double c2, int stop) {
  for (int k = 0; k < 6; ++k) ms->th[k] = 0.0;
  for (int k = 0; k < MOT_NS; ++k) ms->sums[k] = 0.0;
  ms->c2 = c2;
  ms->passes = 0;
  ms->degenerate = 0;
  ms->stop = stop;
  ms->pad_ = 0;
}

__global__ void k_motion_init(MotionState *__restrict__ ms, double c2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  mot_reset(ms, c2, 0);
}

// The tile mapping of every kernel that walks a plane in the fit's order: wave
// w of block b has tile b * MOT_WAVES + w (row-major over ntx tiles across),
// lane l its column j, rows i0 .. i0 + 7
#define MOT_TILE(ntx)                                                 \
  const int lane = threadIdx.x & 63;                                  \
  const int tile = blockIdx.x * MOT_WAVES + (threadIdx.x >> 6);       \
  const int ty = tile / (ntx), tx = tile - ty * (ntx);                \
  const int j = tx * MOT_TW + lane, i0 = ty * MOT_TH

// a sample the fit may use, whatever its weight: a finite flow and state 0
__device__ __forceinline__ bool mot_usable(float2 g, uint8_t state) {
  return __builtin_isfinite(g.x) && __builtin_isfinite(g.y) && state == 0;
}

// One wave per tile (tile = blockIdx.x * MOT_WAVES + wave, row-major over
// ntx tiles across), lane l its column: the eight rows' loads first (each
// coalesced along the 64 columns), then 13 fp64 accumulators per lane over
// the rows ascending, the tree across the lanes, and lane 0 writes the tile's
// record: rec[k * stride + tile].  Positions outside the frame add nothing
// (the accumulators start at +0.0 and never become -0.0, so that is adding
// +0.0).  A stopped fit skips its remaining solving passes.
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_motion_part(const float2 *__restrict__ uv, int H, int W, int P, const float *__restrict__ wgt,
              const uint8_t *__restrict__ st, const MotionState *__restrict__ ms, int pass, MotionFrame fr, int ntx,
              int nt, int stride, double *__restrict__ rec, float *__restrict__ inl) {
  OF_NOCONTRACT
  MOT_TILE(ntx);
  if (tile >= nt) return;  // the whole wave
  if (pass != MOT_PASS_LAST && ms->stop) return;
  const bool jin = j < W;
  const double th0 = ms->th[0], th1 = ms->th[1], th2 = ms->th[2], th3 = ms->th[3], th4 = ms->th[4], th5 = ms->th[5];
  const double c2 = ms->c2;
  float2 g[MOT_TH];
  float w32[MOT_TH];
  uint8_t s8[MOT_TH];
#pragma unroll
  for (int r = 0; r < MOT_TH; ++r) {
    const int i = i0 + r;
    const bool in = jin && i < H;
    const size_t o = (size_t)i * W + j;
    g[r] = in ? uv[(size_t)i * P + j] : make_float2(0.0f, 0.0f);
    w32[r] = in && wgt ? wgt[o] : 1.0f;
    s8[r] = in && st ? st[o] : (uint8_t)0;
  }
  const double x = ((double)j - fr.cx) / fr.s;
  double a[MOT_NS];
#pragma unroll
  for (int k = 0; k < MOT_NS; ++k) a[k] = 0.0;
#pragma unroll
  for (int r = 0; r < MOT_TH; ++r) {
    const int i = i0 + r;
    if (!(jin && i < H)) continue;
    const bool ok = mot_usable(g[r], s8[r]);
    const double w0 = ok ? (double)w32[r] : 0.0;
    const double u = ok ? (double)g[r].x : 0.0, v = ok ? (double)g[r].y : 0.0;
    const double y = ((double)i - fr.cy) / fr.s;
    const double uh = th0 + th1 * x + th2 * y, vh = th3 + th4 * x + th5 * y;
    const double ru = u - uh, rv = v - vh;
    const double r2 = ru * ru + rv * rv;
    double w = w0;
    if (pass != MOT_PASS_FIRST) {
      const double z = r2 / c2;
      const double t = z < 1.0 ? z : 1.0;
      w = w0 * ((1.0 - t) * (1.0 - t));
    }
    if (inl) inl[(size_t)i * W + j] = (float)w;
    const double wx = w * x, wy = w * y;
    a[0] = a[0] + w;
    a[1] = a[1] + wx;
    a[2] = a[2] + wy;
    a[3] = a[3] + wx * x;
    a[4] = a[4] + wx * y;
    a[5] = a[5] + wy * y;
    a[6] = a[6] + w * u;
    a[7] = a[7] + wx * u;
    a[8] = a[8] + wy * u;
    a[9] = a[9] + w * v;
    a[10] = a[10] + wx * v;
    a[11] = a[11] + wy * v;
    a[12] = a[12] + w * r2;
  }
#pragma unroll
  for (int k = 0; k < MOT_NS; ++k) {
    const double s = mot_tree(a[k]);
    if (lane == 0) rec[(size_t)k * stride + tile] = s;
  }
}

// One level of the group tree: n values per sum (src[k * sstride + .]) become
// ceil(n / 64), one wave per group of 64, the last group padded with zeros.
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_motion_group(const double *__restrict__ src, int n, int sstride, double *__restrict__ dst, int dstride,
               const MotionState *__restrict__ ms, int pass) {
  const int lane = threadIdx.x & 63;
  const int grp = blockIdx.x * MOT_WAVES + (threadIdx.x >> 6);
  if (grp >= (n + 63) / 64) return;  // the whole wave
  if (pass != MOT_PASS_LAST && ms->stop) return;
  const int idx = grp * 64 + lane;
#pragma unroll
  for (int k = 0; k < MOT_NS; ++k) {
    const double s = mot_tree(idx < n ? src[(size_t)k * sstride + idx] : 0.0);
    if (lane == 0) dst[(size_t)k * dstride + grp] = s;
  }
}

// The solve of one pass in the closed forms of include/optflow.h, operation
// for operation: th from the 13 sums (Sw > 0); true when the model lost rank
// and the translation was solved.  The one statement of it: the fit
// (k_motion_final) and the layers' hypotheses (k_layers_cells) both call it.
__device__ __forceinline__ bool mot_solve(const double *S, int model, double *th) {
  OF_NOCONTRACT
  const double Sw = S[0], Sx = S[1], Sy = S[2], Sxx = S[3], Sxy = S[4], Syy = S[5];
  const double Su = S[6], Sxu = S[7], Syu = S[8], Sv = S[9], Sxv = S[10], Syv = S[11];
  th[0] = Su / Sw;  // the translation model
  th[3] = Sv / Sw;
  th[1] = th[2] = th[4] = th[5] = 0.0;
  if (model == OF_MOTION_SIMILARITY) {
    const double q = Sxx + Syy;
    const double D = q - (Sx * Sx + Sy * Sy) / Sw;
    if (!(D > 1e-9 * Sw)) return true;
    const double ca = ((Sxu + Syv) - (Sx * Su + Sy * Sv) / Sw) / D;
    const double cb = ((Sxv - Syu) - (Sx * Sv - Sy * Su) / Sw) / D;
    th[0] = (Su - ca * Sx + cb * Sy) / Sw;
    th[3] = (Sv - cb * Sx - ca * Sy) / Sw;
    th[1] = ca;
    th[5] = ca;
    th[4] = cb;
    th[2] = -cb;
  } else if (model == OF_MOTION_AFFINE) {
    const double m = Sx / Sw, nn = Sy / Sw;
    const double A = Sxx - m * Sx, B = Sxy - m * Sy, Cc = Syy - nn * Sy;
    const double l = B / A;
    const double E = Cc - l * B;
    if (!(A > 1e-9 * Sw) || !(E > 1e-9 * Sw)) return true;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const double Sf = f ? Sv : Su, Sxf = f ? Sxv : Sxu, Syf = f ? Syv : Syu;
      const double gx = Sxf - m * Sf, gy = Syf - nn * Sf;
      const double p2 = (gy - l * gx) / E;
      const double p1 = (gx - B * p2) / A;
      const double p0 = (Sf - Sx * p1 - Sy * p2) / Sw;
      th[3 * f] = p0;
      th[3 * f + 1] = p1;
      th[3 * f + 2] = p2;
    }
  }
  return false;
}

// The last level (n <= 64 values per sum, one wave), then in lane 0 the solve
// of the pass and the cutoff update: th and c2 stay in device memory for the
// next pass, so a whole fit is a chain of launches with one read-back at its
// end.  The solve is mot_solve.  kappa2 = kappa * kappa and cmin2 = c_min *
// c_min from the host.
__global__ void __launch_bounds__(64)
k_motion_final(const double *__restrict__ src, int n, int sstride, MotionState *__restrict__ ms, int pass, int model,
               double kappa2, double decay, double cmin2) {
  OF_NOCONTRACT
  if (pass != MOT_PASS_LAST && ms->stop) return;
  const int lane = threadIdx.x;
  double S[MOT_NS];
#pragma unroll
  for (int k = 0; k < MOT_NS; ++k) S[k] = mot_tree(lane < n ? src[(size_t)k * sstride + lane] : 0.0);
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < MOT_NS; ++k) ms->sums[k] = S[k];
  if (pass == MOT_PASS_LAST) return;
  const double Sw = S[0], Sr = S[12];
  ms->passes += 1;
  if (!(Sw > 0.0)) {
    ms->stop = 1;
    ms->degenerate |= 2;
    return;
  }
  double th[6];
  const bool lost = mot_solve(S, model, th);
  if (lost) ms->degenerate |= 1;
#pragma unroll
  for (int k = 0; k < 6; ++k) ms->th[k] = th[k];
  const double c = pass == MOT_PASS_FIRST ? kappa2 * (Sr / Sw) : ms->c2 * decay;
  ms->c2 = c > cmin2 ? c : cmin2;
}

// out(i, j, c) = im_c sampled where the matrix A sends the output pixel:
// q = (A0 j + A1 i) + A2, r = (A3 j + A4 i) + A5; a point that is not finite
// or lies outside the frame gives out 0 and valid 0
struct AffineMat {
  double a[6];
};
__global__ void k_warp_affine(const float *__restrict__ im, int C, AffineMat A, int H, int W, float *__restrict__ out,
                              uint8_t *__restrict__ valid) {
  OF_NOCONTRACT
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t o = (size_t)i * W + j;
    const double q = (A.a[0] * (double)j + A.a[1] * (double)i) + A.a[2];
    const double r = (A.a[3] * (double)j + A.a[4] * (double)i) + A.a[5];
    const bool ok = __builtin_isfinite(q) && __builtin_isfinite(r) && in_frame(r, q, H, W);
    if (valid) valid[o] = ok ? 1 : 0;
    if (!ok) {
      for (int ch = 0; ch < C; ++ch) out[o * C + ch] = 0.0f;
      continue;
    }
    const BilTap b = bil_tap(r, q, H, W);
    for (int ch = 0; ch < C; ++ch) out[o * C + ch] = (float)bil_at(im, C, ch, b);
  }
}
