// kernels_noise.hip — noise-level estimation: per-pixel keys (a squared
// residual as fp32) of the motion-compensated pair estimator and of the
// single-frame 2 x 2 detail estimator, and an exact radix selection of the
// lower median of each channel's keys.  Frames are dense H x W x C interleaved
// fp32, the flow pitched float2, the state dense H x W bytes in
// of_fb_consistency's encoding.  All arithmetic in fp64 from the fp32 inputs
// with no contraction, in the order include/optflow.h states
// (of_estimate_noise_pair, of_estimate_noise), so a numpy float64 restatement
// gives the same bits.  H * W < 2^31 (checked on the host).  Expects
// kernels_sample.hip before it (in_frame, bil_tap, bil_at).
//
// Keys are non-negative floats (+Inf included), so their bit patterns order
// as unsigned integers; a slot without a usable sample holds NOISE_NOKEY, all
// ones, above every key.  The rank looked for is below the number of usable
// samples, so the selection never reaches those slots.  Three passes of 11 /
// 11 / 10 bits, most significant first: a counting kernel (per-workgroup LDS
// bins merged into the global bins with integer atomics: the counts do not
// depend on the order of arrival) and k_noise_pick, one workgroup, which finds
// the bin that holds the rank and leaves the prefix and the remaining rank on
// the device for the next pass.  The first count rides on the key kernels.
#include "kernels.h"

#define NOISE_BLOCK 256      // every kernel here: 1-D blocks of four waves
#define NOISE_MAX_C 4        // channels
#define NOISE_BINS 2048      // 11 bits, the widest pass
#define NOISE_NOKEY 0xffffffffu

// the selection's words on the device; the host reads it back once per call
struct NoiseSel {
  uint32_t n;                    // usable samples (the same for every channel)
  uint32_t prefix[NOISE_MAX_C];  // the bits of the rank's key decided so far, right-aligned
  uint32_t rank[NOISE_MAX_C];    // the rank among the keys that share the prefix
  uint32_t pad_[7];
  uint32_t bins[NOISE_MAX_C * NOISE_BINS];  // all 0 between passes (k_noise_pick clears what it read)
};

// ---- the first pass's counts, shared by both key kernels --------------------
__device__ __forceinline__ void noise_bins_clear(uint32_t *s_bins, int n) {
  for (int b = threadIdx.x; b < n; b += NOISE_BLOCK) s_bins[b] = 0;
  __syncthreads();
}
// the workgroup's counts into the global bins, the empty ones skipped
__device__ __forceinline__ void noise_bins_merge(const uint32_t *s_bins, int n, uint32_t *bins) {
  __syncthreads();
  for (int b = threadIdx.x; b < n; b += NOISE_BLOCK) {
    const uint32_t v = s_bins[b];
    if (v) atomicAdd(&bins[b], v);
  }
}

// A sample's keys (NOISE_NOKEY where it is not usable) into slot p of every
// channel's N, and the usable ones into the workgroup's counts
__device__ __forceinline__ void noise_put(bool ok, const double (&v)[NOISE_MAX_C], int C, uint32_t *__restrict__ keys,
                                          unsigned N, unsigned p, uint32_t *s_bins, uint32_t *s_n) {
  if (ok) atomicAdd(s_n, 1u);
#pragma unroll
  for (int c = 0; c < NOISE_MAX_C; ++c)
    if (c < C) {
      const uint32_t k = ok ? __float_as_uint((float)v[c]) : NOISE_NOKEY;
      keys[(size_t)c * N + p] = k;
      if (ok) atomicAdd(&s_bins[c * NOISE_BINS + (k >> 21)], 1u);
    }
}

// Pair estimator: one thread per pixel p = i * W + j (grid-stride), keys[c * N
// + p] for N = H * W.  A pixel is usable when its flow is finite and lands
// inside the frame, its state is 0 and no value involved (its own and the four
// taps', every channel) is non-finite.
__global__ void __launch_bounds__(NOISE_BLOCK)
k_noise_keys_pair(const float *__restrict__ im1, const float *__restrict__ im2, const float2 *__restrict__ F,
                  const uint8_t *__restrict__ S, int H, int W, int P, int C, uint32_t *__restrict__ keys,
                  NoiseSel *__restrict__ sel) {
  OF_NOCONTRACT
  __shared__ uint32_t s_bins[NOISE_MAX_C * NOISE_BINS];
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0;
  noise_bins_clear(s_bins, C * NOISE_BINS);
  const unsigned N = (unsigned)H * (unsigned)W;  // < 2^31, and the grid's stride is far below 2^31: p cannot wrap
  for (unsigned p = blockIdx.x * NOISE_BLOCK + threadIdx.x; p < N; p += gridDim.x * NOISE_BLOCK) {
    const int i = (int)(p / (unsigned)W), j = (int)(p - (unsigned)i * (unsigned)W);
    const float2 g = F[(size_t)i * P + j];
    const double r = (double)i + (double)g.y, q = (double)j + (double)g.x;
    bool ok = __builtin_isfinite(g.x) && __builtin_isfinite(g.y) && in_frame(r, q, H, W) && !(S && S[p] != 0);
    double e[NOISE_MAX_C] = {0.0, 0.0, 0.0, 0.0}, gain = 1.0;
    if (ok) {
      const BilTap b = bil_tap(r, q, H, W);
#pragma unroll
      for (int c = 0; c < NOISE_MAX_C; ++c)
        if (c < C) {
          const float a = im1[(size_t)p * C + c];
          ok = ok && __builtin_isfinite(a) && __builtin_isfinite(im2[b.o00 * C + c]) &&
               __builtin_isfinite(im2[b.o01 * C + c]) && __builtin_isfinite(im2[b.o10 * C + c]) &&
               __builtin_isfinite(im2[b.o11 * C + c]);
          e[c] = (double)a - bil_at(im2, C, c, b);
        }
      const double w00 = (1.0 - b.fr) * (1.0 - b.fc), w01 = (1.0 - b.fr) * b.fc;
      const double w10 = b.fr * (1.0 - b.fc), w11 = b.fr * b.fc;
      gain = 1.0 + (((w00 * w00 + w01 * w01) + w10 * w10) + w11 * w11);
    }
#pragma unroll
    for (int c = 0; c < NOISE_MAX_C; ++c) e[c] = e[c] * e[c] / gain;
    noise_put(ok, e, C, keys, N, p, s_bins, &s_n);
  }
  noise_bins_merge(s_bins, C * NOISE_BINS, sel->bins);
  if (threadIdx.x == 0 && s_n) atomicAdd(&sel->n, s_n);
}

// Single-frame estimator: one thread per 2 x 2 block p = bi * Wb + bj of the
// Hb x Wb = (H / 2) x (W / 2) blocks, keys[c * N + p] for N = Hb * Wb.  A
// block is usable when none of its values, in any channel, is non-finite.
__global__ void __launch_bounds__(NOISE_BLOCK)
k_noise_keys_single(const float *__restrict__ im, int H, int W, int C, uint32_t *__restrict__ keys,
                    NoiseSel *__restrict__ sel) {
  OF_NOCONTRACT
  __shared__ uint32_t s_bins[NOISE_MAX_C * NOISE_BINS];
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0;
  noise_bins_clear(s_bins, C * NOISE_BINS);
  const int Hb = H / 2, Wb = W / 2;
  const unsigned N = (unsigned)Hb * (unsigned)Wb;
  for (unsigned p = blockIdx.x * NOISE_BLOCK + threadIdx.x; p < N; p += gridDim.x * NOISE_BLOCK) {
    const int bi = (int)(p / (unsigned)Wb), bj = (int)(p - (unsigned)bi * (unsigned)Wb);
    const size_t o = (size_t)(2 * bi) * W + 2 * bj;
    bool ok = true;
    double d[NOISE_MAX_C] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NOISE_MAX_C; ++c)
      if (c < C) {
        const float a = im[o * C + c], b = im[(o + 1) * C + c];
        const float e = im[(o + W) * C + c], f = im[(o + W + 1) * C + c];
        ok = ok && __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(e) && __builtin_isfinite(f);
        d[c] = (((double)a - (double)b) - ((double)e - (double)f)) / 2.0;
      }
#pragma unroll
    for (int c = 0; c < NOISE_MAX_C; ++c) d[c] = d[c] * d[c];
    noise_put(ok, d, C, keys, N, p, s_bins, &s_n);
  }
  noise_bins_merge(s_bins, C * NOISE_BINS, sel->bins);
  if (threadIdx.x == 0 && s_n) atomicAdd(&sel->n, s_n);
}

// A later pass's counts: channel blockIdx.y; a key counts when its bits above
// `shift + bits` equal the channel's prefix, in the bin of its next `bits`.
__global__ void __launch_bounds__(NOISE_BLOCK)
k_noise_count(const uint32_t *__restrict__ keys, unsigned N, int shift, int bits, NoiseSel *__restrict__ sel) {
  __shared__ uint32_t s_bins[NOISE_BINS];
  const int c = blockIdx.y, nb = 1 << bits;
  noise_bins_clear(s_bins, nb);
  const uint32_t prefix = sel->prefix[c];
  const uint32_t *__restrict__ K = keys + (size_t)c * N;
  for (unsigned p = blockIdx.x * NOISE_BLOCK + threadIdx.x; p < N; p += gridDim.x * NOISE_BLOCK) {
    const uint32_t k = K[p];
    if ((k >> (shift + bits)) == prefix) atomicAdd(&s_bins[(k >> shift) & (uint32_t)(nb - 1)], 1u);
  }
  noise_bins_merge(s_bins, nb, sel->bins + c * NOISE_BINS);
}

// One workgroup: for every channel the bin b of the pass's 2^BITS bins that
// holds the rank (the first pass starts from rank (n - 1) / 2), then prefix =
// prefix << BITS | b and rank -= the counts below b; the bins go back to 0.
// Every thread owns 2^BITS / 256 consecutive bins.  n = 0: nothing to find.
template <int BITS>
__global__ void __launch_bounds__(NOISE_BLOCK)
k_noise_pick(NoiseSel *__restrict__ sel, int C, int first) {
  __shared__ uint32_t s_sum[NOISE_BLOCK];
  constexpr int PER = (1 << BITS) / NOISE_BLOCK;
  const int tid = threadIdx.x;
  const uint32_t n = sel->n;
  for (int c = 0; c < C; ++c) {
    uint32_t *bins = sel->bins + c * NOISE_BINS;
    const uint32_t rank = first ? (n > 0 ? (n - 1) / 2 : 0u) : sel->rank[c];
    const uint32_t prefix = first ? 0u : sel->prefix[c];
    uint32_t own[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      own[k] = bins[tid * PER + k];
      bins[tid * PER + k] = 0;
      sum += own[k];
    }
    s_sum[tid] = sum;
    __syncthreads();  // every thread has read the channel's rank and prefix
    uint32_t below = 0;
    for (int t = 0; t < tid; ++t) below += s_sum[t];
    if (n > 0 && rank >= below && rank < below + sum) {  // one thread: the counts sum to more than the rank
      int b = 0;
#pragma unroll
      for (int k = 0; k < PER - 1; ++k)
        if (rank >= below + own[k]) {
          below += own[k];
          b = k + 1;
        } else {
          break;
        }
      sel->prefix[c] = (prefix << BITS) | (uint32_t)(tid * PER + b);
      sel->rank[c] = rank - below;
    }
    __syncthreads();
  }
}
