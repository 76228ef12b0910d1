// kernels_wmf.hip — the occlusion-weighted, colour-guided weighted median of
// a flow field (k_wmf): the design, the sample weight, the register bitonic
// sort of both lists' keys and the kernel, one instance per guide channels,
// keys per lane and window.  Expects nothing before it but kernels.h and
// nothing here is used by a later kernel file; host_image.hip sizes its LDS.
// tools/micro/wmf_phases.hip builds this file alone with WMF_PHASE_TIMING.
// DESIGN.md, "Weighted median", tells what was measured and rejected.
#include "kernels.h"

// Occlusion-weighted, colour-guided weighted median
// (denoise_color_weighted_medfilt2, weighted_median.py:24-112).  One wave per 8x8 tile:
//  1. the (8+2h)^2 region is loaded straight into registers, NPER keys per
//     lane (element e = lane*NPER + r), and guide+occ records go to LDS;
//  2. u and v keys (the value widened to fp64 with the region position in
//     its low mantissa bits, wmf_key) are bitonic-sorted in registers; each sample's sorted index e gives it a
//     chunk id e / CH (WMF_NC chunks of CH consecutive sorted samples per list);
//  3. every lane visits its own 15x15 window once (no out-of-window work):
//     weight w is added to the lane's chunk sums of the u and v lists
//     (ds_add_f64 into lane-private LDS slots, program order ->
//     deterministic); the window total is the sum of the chunk sums;
//  4. the chunk holding the half-weight crossing is found from the chunk
//     prefix sums; only that chunk's CH sorted samples are walked (per-lane
//     addresses) to the first one whose cumulative weight reaches total/2.
// LDS per wave at h = 7: 8 KB chunk sums + 8.4 KB records + 2 KB sorted
// positions + 1 KB chunk ids = 19.3 KB -> 8 waves per CU.
// Weight = max(2^(-|dlab|^2 * log2e/(2 sigma^2)) * occ, 1e-10) (v_exp_f32);
// result = the first sorted value with cumsum >= total/2
// (weighted_median.py:5-21, :67-112): the cumulative sum at a sorted sample
// is (chunk prefix) + (in-window weights before it in the chunk), the same
// sums the reference forms, summed in another order.
#define WMF_T 8
#ifdef WMF_PHASE_TIMING  // tools/micro/wmf_phases.hip: per-wave phase timestamps
extern __device__ unsigned long long g_wmf_t[];
#define WMF_STAMP(i) \
  if (threadIdx.x == 0) g_wmf_t[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = clock64()
#else
#define WMF_STAMP(i)
#endif
#define WMF_NC 8
// (measured round 6 and removed: 16 chunks for the large regions, 0.888 vs
// 0.691 ms per 1080p launch at 5 instead of 8 waves per CU; a register
// accumulator per row for the middle sample's chunk, 0.828 vs 0.692 ms --
// DESIGN.md "Round 6 in brief" item 4)
// The chunk sums are fp64: 100 % exact on every fixture.  (Measured round 3
// and removed: fp32 sums, half the chunk-sum LDS -- native ds_add_f32, no CAS
// loop, and yet 4.93 vs 0.83 ms per 1080p launch, 99.996 % exact at h = 12;
// profiles/r3ac_wmf_f32sum.log.  The fp32 LDS add is far slower than
// ds_add_f64 here.)
template <int GC>
struct WmfRec;
template <>
struct WmfRec<3> {
  using T = float4;
  __device__ static T make(float a, float b, float c, float o) { return make_float4(a, b, c, o); }
};
template <>
struct WmfRec<1> {
  using T = float2;
  __device__ static T make(float a, float, float, float o) { return make_float2(a, o); }
};

typedef float wmf_v2f __attribute__((ext_vector_type(2)));

// weight of region sample s for a pixel of guide colour (c01, c2):
// max(2^(nk |dlab|^2) occ, 1e-10), channels 0-1 in packed fp32.  Called from
// the window pass and the chunk walk: both must round identically, so no
// contraction beyond the explicit fma.
__device__ __forceinline__ float wmf_w(const float4 &s, wmf_v2f c01, float c2, float nk) {
#pragma clang fp contract(off)
  const wmf_v2f e = wmf_v2f{s.x, s.y} - c01, q = e * e;
  const float e2 = s.z - c2;
  return fmaxf(__builtin_amdgcn_exp2f(__builtin_fmaf(e2, e2, q.x + q.y) * nk) * s.w, 1e-10f);
}
__device__ __forceinline__ float wmf_w(const float2 &s, wmf_v2f c01, float, float nk) {
#pragma clang fp contract(off)
  const float e = s.x - c01.x;
  return fmaxf(__builtin_amdgcn_exp2f(e * e * nk) * s.y, 1e-10f);
}

// v from lane ^ lj: DPP for lj = 1, 2 (quad_perm), 4 (row_half_mirror then
// quad_perm) and 8 (row_ror:8), a ds_bpermute otherwise (16 and 32 use
// swap_rows64 below) (lj is a constant once the sort loops are unrolled)
__device__ __forceinline__ uint64_t xor_lane64(uint64_t v, int lj) {
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  int a, b;
  if (lj == 1) {
    a = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xf, 0xf, false);
    b = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xf, 0xf, false);
  } else if (lj == 2) {
    a = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xf, 0xf, false);
    b = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xf, 0xf, false);
  } else if (lj == 8) {
    a = __builtin_amdgcn_mov_dpp(lo, 0x128, 0xf, 0xf, false);
    b = __builtin_amdgcn_mov_dpp(hi, 0x128, 0xf, 0xf, false);
  } else if (lj == 4) {  // row_half_mirror (l ^ 7), then quad_perm [3,2,1,0] (l ^ 3)
    a = __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(lo, 0x141, 0xf, 0xf, false), 0x1B, 0xf, 0xf, false);
    b = __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(hi, 0x141, 0xf, 0xf, false), 0x1B, 0xf, 0xf, false);
  } else {
    return __shfl_xor(v, lj);
  }
  return ((uint64_t)(uint32_t)b << 32) | (uint32_t)a;
}

// v_permlane16_swap / v_permlane32_swap (gfx950) of two 64-bit registers: the upper
// row of each 32-lane row pair (lj = 16) / the upper 32 lanes (lj = 32) of x
// trade places with the lower row / half of y, i.e. afterwards lower lanes
// hold (x own, x of lane + lj) and upper lanes (y of lane - lj, y own)
__device__ __forceinline__ void swap_rows64(uint64_t &x, uint64_t &y, int lj) {
  const unsigned xl = (unsigned)x, xh = (unsigned)(x >> 32), yl = (unsigned)y, yh = (unsigned)(y >> 32);
  unsigned a0, a1, b0, b1;
  if (lj == 16) {
    const auto l = __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
    a0 = l[0]; b0 = l[1]; a1 = h[0]; b1 = h[1];
  } else {
    const auto l = __builtin_amdgcn_permlane32_swap(xl, yl, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(xh, yh, false, false);
    a0 = l[0]; b0 = l[1]; a1 = h[0]; b1 = h[1];
  }
  x = ((uint64_t)a1 << 32) | a0;
  y = ((uint64_t)b1 << 32) | b0;
}

// Sort keys: the flow value widened to fp64 (exact), the region position
// (ry << 8 | rx) in the 29 mantissa bits the widening leaves zero.  As
// doubles they order by value, ties by position (reversed for negative
// values: any fixed tie order gives the same weighted median), -0 before +0
// like the old integer key; +-inf and NaN map to +-2^1000 / 2^1001 (above
// every finite fp32) so no key is a NaN, padding to 2^1002.  The position is
// the key's low 16 bits either way.
__device__ __forceinline__ uint64_t wmf_key(float v, unsigned pos) {
  // selects, not branches: the region load issues every read before the
  // first key is formed
  const double d = (double)v;
  const double e = v > 0.f ? 0x1p1000 : -0x1p1000;
  const double f = __builtin_isnan(v) ? 0x1p1001 : (__builtin_isinf(v) ? e : d);
  return __builtin_bit_cast(uint64_t, f) | (uint64_t)pos;
}
// padding keys: above every value; position (RW, 0), one row below the
// region -- out of every lane's window (dy = RW - py > 2 hsz), yet its
// record address (RW * RP) is inside the LDS allocation, so the chunk walk
// reads it without a select
#define WMF_PAD_KEY(RW) (__builtin_bit_cast(uint64_t, 0x1p1002) | ((uint64_t)(RW) << 8))
__device__ __forceinline__ double wmf_d(uint64_t k) { return __builtin_bit_cast(double, k); }
// v_min_f64 / v_max_f64 without the canonicalising v_max_f64 x, x that the
// builtins add in IEEE mode (keys are never NaN, and fp64 denormals -- the
// keys of +-0 -- are preserved: float_denorm_mode_16_64 = 3)
__device__ __forceinline__ uint64_t wmf_min(uint64_t a, uint64_t b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(wmf_d(a)), "v"(wmf_d(b)));
  return __builtin_bit_cast(uint64_t, r);
}
__device__ __forceinline__ uint64_t wmf_max(uint64_t a, uint64_t b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(wmf_d(a)), "v"(wmf_d(b)));
  return __builtin_bit_cast(uint64_t, r);
}

// (min, max) of a pair from one asm statement: a select between two outputs
// of one statement cannot be turned into a branch around either
__device__ __forceinline__ void wmf_minmax(uint64_t a, uint64_t b, uint64_t &mn, uint64_t &mx) {
  double r0, r1;
  asm("v_min_f64 %0, %2, %3\n\tv_max_f64 %1, %2, %3" : "=&v"(r0), "=&v"(r1) : "v"(wmf_d(a)), "v"(wmf_d(b)));
  mn = __builtin_bit_cast(uint64_t, r0);
  mx = __builtin_bit_cast(uint64_t, r1);
}
// min(a, -b) in one v_min_f64 (source negate modifier)
__device__ __forceinline__ uint64_t wmf_min_neg(uint64_t a, uint64_t b) {
  double r;
  asm("v_min_f64 %0, %1, -%2" : "=v"(r) : "v"(wmf_d(a)), "v"(wmf_d(b)));
  return __builtin_bit_cast(uint64_t, r);
}

template <int NPER>
struct Bitonic {
  static constexpr int N = NPER * 64;
  // lane bits of the sign in stage (kk, jj): (lane * NPER) & kk, xor lj for a
  // DPP cross-lane stage; and the bit of r (kk < NPER)
  static constexpr int lane_sel(int kk, int jj) {
    return ((kk >= NPER ? kk / NPER : 0) ^ (jj >= NPER && jj / NPER < 16 ? jj / NPER : 0)) & 63;
  }
  static constexpr bool r_bit(int r, int kk) { return kk < NPER && (r & kk) != 0; }

  // one stage (kk, jj) after stage (pkk, pjj) (pkk = 0: none), then the next
  template <int KK, int JJ, int PKK, int PJJ>
  __device__ __forceinline__ static void stage(uint64_t (&ka)[NPER], uint64_t (&kb)[NPER], int lane) {
    constexpr int ls = lane_sel(KK, JJ) ^ (PKK ? lane_sel(PKK, PJJ) : 0);
    const unsigned lflip = ls ? (unsigned)(__builtin_popcount(lane & ls) & 1) << 31 : 0u;
#pragma unroll
    for (int r = 0; r < NPER; ++r) {
      const bool rf = r_bit(r, KK) != (PKK ? r_bit(r, PKK) : false);
      if (ls || rf) {
        const uint64_t m = (uint64_t)(lflip ^ (rf ? 0x80000000u : 0u)) << 32;
        ka[r] ^= m;
        kb[r] ^= m;
      }
    }
    if constexpr (JJ >= NPER) {
      constexpr int lj = JJ / NPER;
      if constexpr (lj == 16 || lj == 32) {
        // the two lists' key r in one exchange: swap_rows64(a, b) leaves the
        // lower rows / half holding list a's pair (own, partner) and the upper
        // ones list b's pair; each lane forms (min, max) of its pair, and the
        // same exchange of (min, max) hands every lane its own result -- list
        // a: lower min, upper max; list b likewise -- in 3 instructions per
        // key.  (Measured round 6 and removed: each list's key swapped with
        // itself, 2 copies + 2 swaps + min + max + 2 selects per key; sort
        // VALU 2275 vs 2031 per wave, 0.674 vs 0.667 ms per 1080p launch --
        // DESIGN.md "Round 6 in brief" item 4)
#pragma unroll
        for (int r = 0; r < NPER; ++r) {
          uint64_t x = ka[r], y = kb[r], mn, mx;
          swap_rows64(x, y, lj);
          wmf_minmax(x, y, mn, mx);
          swap_rows64(mn, mx, lj);
          ka[r] = mn;
          kb[r] = mx;
        }
      } else {
        // every partner first, then the minima: the DPP moves of a key are
        // not right behind the v_xor that wrote it (VALU -> DPP hazard nops)
        uint64_t pa[NPER], pb[NPER];
#pragma unroll
        for (int r = 0; r < NPER; ++r) {
          pa[r] = xor_lane64(ka[r], lj);
          pb[r] = xor_lane64(kb[r], lj);
        }
#pragma unroll
        for (int r = 0; r < NPER; ++r) {
          ka[r] = wmf_min_neg(ka[r], pa[r]);
          kb[r] = wmf_min_neg(kb[r], pb[r]);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < NPER; ++r) {
        const int rp = r ^ JJ;
        if (rp > r) {
          const uint64_t a0 = ka[r], a1 = ka[rp], b0 = kb[r], b1 = kb[rp];
          ka[r] = wmf_min(a0, a1);
          ka[rp] = wmf_max(a0, a1);
          kb[r] = wmf_min(b0, b1);
          kb[rp] = wmf_max(b0, b1);
        }
      }
    }
    if constexpr (JJ > 1) {
      stage<KK, JJ / 2, KK, JJ>(ka, kb, lane);
    } else if constexpr (KK < N) {
      stage<2 * KK, KK, KK, JJ>(ka, kb, lane);
    } else {
      // back to plain keys (the last merge's blocks are all ascending and
      // its last stage is in-lane: nothing left to flip unless NPER == 1)
      constexpr int le = lane_sel(KK, JJ);
      if constexpr (le != 0) {
        const uint64_t m = (uint64_t)((unsigned)(__builtin_popcount(lane & le) & 1) << 31) << 32;
#pragma unroll
        for (int r = 0; r < NPER; ++r) {
          ka[r] ^= m;
          kb[r] ^= m;
        }
      }
    }
  }
};

// Bitonic sort of the 64*NPER keys of two lists at once (element e = lane *
// NPER + r).  Merge kk sorts blocks of kk elements ascending where e & kk is
// 0 and descending elsewhere; the keys of descending blocks carry a flipped
// sign bit during that merge (min of negated keys = max), so every
// compare-exchange is ascending.  A pair inside a lane is one v_min_f64 + one
// v_max_f64.  A pair across lanes at lane distance lj < 16 (DPP partner):
// during that stage the upper lane of each pair (lane & lj) holds its keys
// negated as well, so both lanes compute min(own, -partner) -- the lower lane
// gets min(x_L, x_U), the upper -max(x_L, x_U) -- one v_min_f64 with a
// negated source and no per-lane select (was v_cmp + an SALU xor of the
// compare mask with the lane's direction + two v_cndmask, the compare mask
// one SGPR pair every key waited on).  The sign changes between stages are
// one v_xor of the high dword per key with a lane-only mask (Bitonic::stage:
// every stage a template instance, so every mask and partner distance is a
// compile-time constant).  At lj = 16 / 32 the two lists' keys share one
// v_permlane{16,32}_swap exchange (swap_rows64; see the stage).
template <int NPER>
__device__ __forceinline__ void bitonic_regs2(uint64_t (&ka)[NPER], uint64_t (&kb)[NPER], int lane) {
  Bitonic<NPER>::template stage<2, 1, 0, 0>(ka, kb, lane);
}

// HS > 0: area_hsz fixed at compile time (window loop fully unrolled,
// immediate LDS offsets); HS == 0: runtime hsz.  RP = LDS row pitch of the
// region records (RP % 16 == 8: the 8 rows of a tile fall on disjoint banks).
// LDS (not VGPRs) bounds the occupancy at 2 waves per SIMD: let the
// scheduler use the registers to keep LDS reads in flight
template <int GC, int NPER, int HS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_wmf(const float2 *__restrict__ uv, const float *__restrict__ guide,
                                             const float *__restrict__ occ, float2 *out, int H, int W,
                                             int P, size_t ps, int hsz_rt, float nk, int RW_rt, int RP_rt,
                                             const float2 *base) {
  using T = typename WmfRec<GC>::T;
  constexpr int N = NPER * 64, NC = WMF_NC, CH = N / NC;
  const int hsz = HS > 0 ? HS : hsz_rt;
  // region width and record pitch: compile-time with HS (no runtime divides)
  constexpr int RWc = WMF_T + 2 * HS, RPc = RWc + ((8 - RWc) % 16 + 16) % 16;
  const int RW = HS > 0 ? RWc : RW_rt, RP = HS > 0 ? RPc : RP_rt;
  // whole-sample reflect with one fold reaches every region sample when the
  // plane has >= WMF_T + hsz rows / columns (all pyramid levels of the
  // registry); otherwise the general modulo form
  const bool fold1 = H >= WMF_T + hsz && W >= WMF_T + hsz;
  auto mir = [&](int i, int n) { return fold1 ? (i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i)) : ext_mirror(i, n); };
  const int nreg = RW * RW;
  // LDS: chunk sums [2][WMF_NC][64] f64 (u chunks, then v chunks; a chunk's
  // 64 lane slots are contiguous, so a scatter-add never conflicts) | records
  // [RW][RP] | sorted positions (ry << 8 | rx) of the u and v lists [2][N] u16 |
  // chunk ids [2][RW][RP] u8 (the u list's plane, then the v list's.
  // Measured rounds 2 and 4 and removed: the two ids of a sample side by
  // side, one u16 read per window sample instead of two u8, 0.821 vs 0.777 ms
  // per 1080p launch; profiles/r4h_wmf_cid_ab.log)
  extern __shared__ double csum[];
  T *smp = reinterpret_cast<T *>(csum + 2 * NC * 64);
  uint16_t *ku = reinterpret_cast<uint16_t *>(smp + RW * RP), *kv = ku + N;
  uint8_t *cid = reinterpret_cast<uint8_t *>(kv + N);
  // blocks b, b + 8, b + 16 ... run on one XCD (one L2), so each XCD gets a
  // contiguous run of row-major tiles; the 22x22 regions of horizontally
  // adjacent tiles (8 apart) then overlap inside one L2 instead of eight
  // (the same time per launch as the plain order, HBM traffic 315 -> 89 MB;
  // DESIGN.md, "Weighted median")
  const int nt = gridDim.x * gridDim.y, lin = blockIdx.x + blockIdx.y * gridDim.x;
  const int xcd = lin & 7, tile = xcd * (nt >> 3) + min(xcd, nt & 7) + (lin >> 3);
  const int tby = tile / gridDim.x, tbx = tile - tby * gridDim.x;
  const int ty0 = tby * WMF_T, tx0 = tbx * WMF_T;
  const int lane = threadIdx.x;
  WMF_STAMP(0);
  // region load: every lane's NPER samples' offsets first (padding lanes,
  // s >= nreg, re-read the last sample and rewrite its record with the same
  // bytes), then all uv / guide / occ reads, then keys and records -- no
  // branch between the reads, so they are all in flight at once (was one
  // round trip per sample and read kind: 15.5 K of 102 K cycles per wave)
  uint64_t a[NPER], b[NPER];
  unsigned goff[NPER], rpos[NPER];
  auto region_offsets = [&](auto mirf) {
#pragma unroll
    for (int r = 0; r < NPER; ++r) {
      const int s = min(lane * NPER + r, nreg - 1);
      const int ry = s / RW, rx = s - ry * RW;
      goff[r] = (unsigned)(mirf(ty0 - hsz + ry, H) * P + mirf(tx0 - hsz + rx, W));
      rpos[r] = ((unsigned)ry << 8) | (unsigned)rx;
    }
  };
  if (fold1)
    region_offsets([](int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); });
  else
    region_offsets([](int i, int n) { return ext_mirror(i, n); });
  float2 rv[NPER];
  float rg[NPER][3], ro[NPER];
#pragma unroll
  for (int r = 0; r < NPER; ++r) rv[r] = uv[goff[r]];
#pragma unroll
  for (int r = 0; r < NPER; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rg[r][c] = c < GC ? guide[c * ps + goff[r]] : 0.f;
    ro[r] = occ[goff[r]];
  }
#pragma unroll
  for (int r = 0; r < NPER; ++r) {
    // padding keys by a mask, not a select: a per-lane select lets the
    // compiler sink the last sample's read into a branch behind the others
    const uint64_t pm = 0ull - (uint64_t)(lane * NPER + r >= nreg);
    const uint64_t ka = wmf_key(rv[r].x, rpos[r]), kb = wmf_key(rv[r].y, rpos[r]);
    a[r] = ka ^ ((ka ^ WMF_PAD_KEY(RW)) & pm);
    b[r] = kb ^ ((kb ^ WMF_PAD_KEY(RW)) & pm);
    smp[(rpos[r] >> 8) * RP + (rpos[r] & 0xffu)] = WmfRec<GC>::make(rg[r][0], rg[r][1], rg[r][2], ro[r]);
  }
  double *cs = csum + lane;
#pragma unroll
  for (int c = 0; c < 2 * NC; ++c) cs[c * 64] = 0.0;
  WMF_STAMP(1);
  bitonic_regs2<NPER>(a, b, lane);
#pragma unroll
  for (int r = 0; r < NPER; ++r) {
    const int e = lane * NPER + r;
    const unsigned pa = (uint16_t)a[r], pb = (uint16_t)b[r];
    ku[e] = (uint16_t)pa;  // padding keys -> (RW, 0): out of every window
    kv[e] = (uint16_t)pb;
    const int qa = (pa >> 8) * RP + (pa & 0xffu), qb_ = (pb >> 8) * RP + (pb & 0xffu);
    const unsigned padpos = (unsigned)RW << 8;
    if (pa != padpos) cid[qa] = (uint8_t)(e / CH);
    if (pb != padpos) cid[RW * RP + qb_] = (uint8_t)(e / CH);
  }
  __syncthreads();
  WMF_STAMP(2);
  const int py = lane >> 3, px = lane & 7;
  const int gi = ty0 + py, gj = tx0 + px;
  const int qb = py * RP + px;
  float cg[3] = {0.f, 0.f, 0.f};
  {
    const T c0 = smp[qb + hsz * RP + hsz];
    const float *cf = reinterpret_cast<const float *>(&c0);
#pragma unroll
    for (int c = 0; c < GC; ++c) cg[c] = cf[c];
  }
  const wmf_v2f c01 = {cg[0], cg[1]};
  // window pass: the per-chunk weight of both lists.  One window row per
  // step: its records and chunk offsets are read first, so the LDS latency
  // is paid once per row.
  char *csb = reinterpret_cast<char *>(cs);
  auto visit_row = [&](int q0, int n) {
    constexpr int MX = HS > 0 ? 2 * HS + 1 : 5;
    T rec[MX];
    unsigned cu[MX], cv[MX];
#pragma unroll
    for (int dx = 0; dx < MX; ++dx)
      if (dx < n) {
        rec[dx] = smp[q0 + dx];
        cu[dx] = cid[q0 + dx];
        cv[dx] = cid[RW * RP + q0 + dx];
      }
#pragma unroll
    for (int dx = 0; dx < MX; ++dx)
      if (dx < n) {
        const double w = (double)wmf_w(rec[dx], c01, cg[2], nk);
        atomicAdd(reinterpret_cast<double *>(csb + (cu[dx] << 9)), w);  // 512 B: a chunk's 64 lane slots
        atomicAdd(reinterpret_cast<double *>(csb + (cv[dx] << 9)) + NC * 64, w);
      }
  };
  if (HS > 0) {
#pragma unroll
    for (int dy = 0; dy <= 2 * HS; ++dy) visit_row(qb + dy * RP, 2 * HS + 1);
  } else {
    for (int dy = 0; dy <= 2 * hsz; ++dy)
      for (int dx = 0; dx <= 2 * hsz; dx += 5) visit_row(qb + dy * RP + dx, min(5, 2 * hsz + 1 - dx));
  }
  WMF_STAMP(3);
  double su[NC], sv[NC], tot = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    su[c] = cs[c * 64];
    sv[c] = cs[(NC + c) * 64];
    tot += su[c];
  }
  const double half = 0.5 * tot;
  // crossing chunk of each list: first chunk whose running sum reaches half
  double pu = 0.0, pv = 0.0, bu = 0.0, bv = 0.0;
  int chu = -1, chv = -1, lastu = 0, lastv = 0;
  double lbu = 0.0, lbv = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (chu < 0 && su[c] > 0.0) { lastu = c; lbu = pu; }
    if (chv < 0 && sv[c] > 0.0) { lastv = c; lbv = pv; }
    if (chu < 0 && pu + su[c] >= half) { chu = c; bu = pu; }
    if (chv < 0 && pv + sv[c] >= half) { chv = c; bv = pv; }
    pu += su[c];
    pv += sv[c];
  }
  // rounding of the v chunk sums vs the total: fall back to the last chunk
  // with window weight (the walk then ends on its last window sample)
  if (chu < 0) { chu = lastu; bu = lbu; }
  if (chv < 0) { chv = lastv; bv = lbv; }
  WMF_STAMP(4);
  const unsigned span = 2u * hsz;
  // walk results as record indices relative to the lane's window origin qb
  // The median is the first in-window sample whose cumulative sum reaches
  // half; every in-window weight is >= 1e-10 (far above an ulp of a sum
  // <= 225), so the sums strictly increase and that sample is also the LAST
  // in-window sample whose sum BEFORE it is still below half (the walk starts
  // below half: the crossing chunk's prefix, or the fallback's).  With no
  // crossing in the chunk that is its last in-window sample -- the fallback
  // below -- so one compare and one select per sample and list, no "found"
  // state.  (Measured round 6 and removed: the first-reach walk with a found
  // flag and a last-seen index per list, the same sample bitwise; walk VALU
  // 3024 vs 2704 per wave, 0.692 vs 0.668 ms per 1080p launch -- DESIGN.md
  // "Round 6 in brief" item 4)
  unsigned resu = 0, resv = 0;
  // the crossing chunks' sorted positions (ry << 8 | rx), 8 per 16-B read;
  // window offsets straight from the position bytes (dy = ry - py and
  // dx = rx - px as unsigned: out of the window unless both <= span; padding
  // keys have ry = RW)
  const uint4 *wu = reinterpret_cast<const uint4 *>(ku + chu * CH), *wv = reinterpret_cast<const uint4 *>(kv + chv * CH);
  for (int g = 0; g < CH / 8; ++g) {
    const uint4 A = wu[g], B = wv[g];
    const unsigned wa4[4] = {A.x, A.y, A.z, A.w}, wb4[4] = {B.x, B.y, B.z, B.w};
    unsigned qa[8], qv[8];
    bool ina[8], inb[8];
    T ra[8], rb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int sh = 16 * (i & 1);
      const unsigned wa = wa4[i >> 1], wb = wb4[i >> 1];
      const unsigned dya = ((wa >> (sh + 8)) & 0xffu) - (unsigned)py, dxa = ((wa >> sh) & 0xffu) - (unsigned)px;
      const unsigned dyb = ((wb >> (sh + 8)) & 0xffu) - (unsigned)py, dxb = ((wb >> sh) & 0xffu) - (unsigned)px;
      ina[i] = max(dya, dxa) <= span;
      inb[i] = max(dyb, dxb) <= span;
      // qb + qa = ry * RP + rx: inside the region for every real sample, the
      // word after it for a padding key (no select needed for the read)
      qa[i] = dya * (unsigned)RP + dxa;
      qv[i] = dyb * (unsigned)RP + dxb;
      ra[i] = smp[qb + qa[i]];
      rb[i] = smp[qb + qv[i]];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float xa = wmf_w(ra[i], c01, cg[2], nk), xb = wmf_w(rb[i], c01, cg[2], nk);
      resu = (ina[i] && bu < half) ? qa[i] : resu;
      resv = (inb[i] && bv < half) ? qv[i] : resv;
      // select before the widening: one v_cndmask instead of two (the empty
      // asm keeps the compiler from hoisting the conversion above the select)
      float sa = ina[i] ? xa : 0.f, sb = inb[i] ? xb : 0.f;
      asm("" : "+v"(sa), "+v"(sb));
      bu += (double)sa;
      bv += (double)sb;
    }
    // (measured r5v: a wave-level exit once every lane has both medians,
    // `if (!__any(resu == 0xffff || resv == 0xffff)) break;`, is 1.5 % slower
    // per launch, 0.812 vs 0.801 ms, same flow: the walk is short and the
    // vote costs more than the samples it saves)
  }
  WMF_STAMP(5);
  if (gi < H && gj < W) {
    // the selected samples' values, re-read at their (mirrored) positions
    const int dya = (int)(resu / (unsigned)RP), dyb = (int)(resv / (unsigned)RP);
    const int ya = mir(gi - hsz + dya, H), xa = mir(gj - hsz + (int)resu - dya * RP, W);
    const int yb = mir(gi - hsz + dyb, H), xb = mir(gj - hsz + (int)resv - dyb * RP, W);
    float2 med = make_float2(uv[(size_t)ya * P + xa].x, uv[(size_t)yb * P + xb].y);
    if (base) {  // out = base + (med - base): classic_nl.py:271-275 fused (out may alias base)
      const float2 b0 = base[(size_t)gi * P + gj];
      med = make_float2(b0.x + (med.x - b0.x), b0.y + (med.y - b0.y));
    }
    out[(size_t)gi * P + gj] = med;
  }
}

#define OF_WMF(GC, NP, HS)                                                                                       \
  template __global__ void k_wmf<GC, NP, HS>(const float2 *, const float *, const float *, float2 *, int, int, int, \
                                              size_t, int, float, int, int, const float2 *);
OF_WMF(1, 1, 0) OF_WMF(1, 2, 0) OF_WMF(1, 4, 0) OF_WMF(1, 8, 0) OF_WMF(1, 16, 0) OF_WMF(1, 8, 7)
OF_WMF(3, 1, 0) OF_WMF(3, 2, 0) OF_WMF(3, 4, 0) OF_WMF(3, 8, 0) OF_WMF(3, 16, 0) OF_WMF(3, 8, 7)
#undef OF_WMF
