// kernels_cgs.hip — k_cgs, the fed CG's iteration for the 'backslash'
// surrogate: the polynomial preconditioner and the strip / halo geometry
// (first comment), the LDS-ring records and their helpers (CgRec, CgRaw,
// cgr_*), the CGS_* knobs with their measurement notes, and the kernel.
// Expects kernels_solve.hip and kernels_cg.hip before it: PcgArgs, the cg_*
// raw-buffer and packed helpers, cg_inv<true>, cg_prologue, write_partials.
// Invariants as for k_cg: one launch per iteration with the launch-boundary
// reduce, the same grid at every launch of a solve, out-of-image lanes load 0
// and store nowhere.  CGS_ / cgs_ names belong to this kernel alone (the host
// geometry knobs CGS_*_BLOCKS included); the one-workgroup CG is CGW_ / cgw_.
#include "kernels.h"

// ---------------------------------------------------------------------------
// The 'backslash' surrogate iteration (k_cgs below): the fused, q-free CG
// iteration with a degree-CG_DEG (5) polynomial preconditioner in the 2x2
// block-Jacobi splitting A = D - N, B = D^-1 N:
//   M^-1 = (c0 + c1 B + ... + c5 B^5) D^-1,
// the Chebyshev polynomial that minimises max |1 - X p(X)| for the spectrum
// of X = D^-1 A = I - B on [a, 2] (a = 0.04, 0.01 for the robust GNC stages;
// host: cheb_poly; 2 bounds the spectrum because D + N is positive
// semidefinite).  p > 0 there, so M is SPD.  (Round 1 used degree 3: 0.54x
// the iterations of a first-order Neumann preconditioner, 0.27x of block
// Jacobi; degree 5 takes 0.69x the iterations of degree 3.)
//
// z = M^-1 r by Horner, one neighbour exchange per stage:
//   y = D^-1 r,  g4 = c4 y + c5 D^-1 N y,  g3 = c3 y + D^-1 N g4, ...,
//   z = c0 y + D^-1 N g1   (and r.z = c0 r.y + y.N g1).
// The rho recurrence needs q.M^-1 q = sum_i c_i T_i with y_q = D^-1 q,
// v1 = D^-1 N y_q, v2 = D^-1 N v1:  T0 = y_q.q, T1 = y_q.N y_q, T2 = v1.N y_q,
// T3 = v1.N v1, T4 = v2.N v1, T5 = v2.N v2 (each edge counted once, by its
// right / lower pixel).
// Seven stencil stages deep, so a strip carries four halo lanes per side
// towards a neighbouring strip: strip t holds columns [112 t, 112 t + 128)
// (lane l: columns 112 t + 2 l and + 1) and owns lanes 4..59 (PCG_SWP = 112
// output columns).  The halo only recomputes the neighbour's pixels, so the
// side of a strip that has no neighbour needs none: the first strip also
// owns lanes 0..3 and the last strip lanes 60..63, i.e. 120 + 112 (n - 2) +
// 120 columns over n strips (17 at 1920, not 18) and all 128 when one strip
// covers the level.  Those lanes are exact as they stand: wave_from_prev /
// wave_from_next are wave_shr:1 / wave_shl:1 DPP moves with bound_ctrl, so
// lane 0 reads 0 as its left value and left weight (cgr_nsum's L and wl, T5's
// h0) and lane 63 reads 0 as its right value (Rt), which is the operator at
// the image's first and last column; columns >= W load 0 through CG_OOB, are
// stored nowhere and count in no dot product (ok0 / ok1 in soff8, dm0, dm1
// and the mask on p), and the ODD instances zero the pixel at column W.
// Arithmetic is on (u, v)
// pairs of one pixel (packed fp32: v_pk_fma_f32).  Each row's coefficients
// are staged once into an LDS ring of records (per pixel the (u, v) weight
// pairs of the edges right and below and D^-1 as (ia, ic), (ic, id)) that
// every stage reads; D itself is re-formed from D^-1 where a stage needs it.

// CGS_HALO: halo lanes per side of a k_cgs strip (2 px each).  Everything a launch
// stores (r, p, x) and the dots p.q, q.z, r.z, r.r are exact with 4 (z
// reaches 6 px out); only the T terms of q.M^-1 q at the strip's first and
// last output columns reach 9-10 px (T5 uses v2 of the left neighbour), so
// they see the DPP's zero beyond lane 0.  That moves only the rho
// recurrence's beta: 5 halo lanes (108 output columns) give the same 479 CG
// iterations per 1080p pair and the same pairs/s (profiles/r3ae_*), so 4.
#ifndef CGS_HALO
#define CGS_HALO 4
#endif
#define PCG_SWP (128 - 4 * CGS_HALO)
#define CG_ROW_OOB 0x40000000u

struct CgRec {  // one LDS-ring row: pixel e of the lane, (u, v) pairs
  cg_f2 wx[2], wy[2];  // weights of the edges right of / below the pixel
  cg_f2 ma[2], mb[2];  // D^-1 columns: (ia, ic), (ic, id)
};
struct CgRaw {  // staged global loads of one coefficient row (plane order)
  cg_f2 wxu, wyu, wxv, wyv, a, c, d;
};

__device__ __forceinline__ cg_f2 cg_lo(cg_f4 v) { return cg_f2{v.x, v.y}; }
__device__ __forceinline__ cg_f2 cg_hi(cg_f4 v) { return cg_f2{v.z, v.w}; }
__device__ __forceinline__ cg_f4 cg_cat(cg_f2 a, cg_f2 b) { return cg_f4{a.x, a.y, b.x, b.y}; }
__device__ __forceinline__ cg_f2 cg_left2(cg_f2 v) { return cg_f2{wave_from_prev(v.x), wave_from_prev(v.y)}; }
__device__ __forceinline__ cg_f2 cg_right2(cg_f2 v) { return cg_f2{wave_from_next(v.x), wave_from_next(v.y)}; }

// N f of the middle row; wu = vertical weight pairs of the row above
__device__ __forceinline__ cg_f4 cgr_nsum(cg_f4 up, cg_f4 mid, cg_f4 dn, const CgRec &c, const cg_f2 (&wu)[2]) {
  const cg_f2 m0 = cg_lo(mid), m1 = cg_hi(mid);
  const cg_f2 L = cg_left2(m1), Rt = cg_right2(m0), wl = cg_left2(c.wx[1]);
  const cg_f2 s0 = wl * L + c.wx[0] * m1 + wu[0] * cg_lo(up) + c.wy[0] * cg_lo(dn);
  const cg_f2 s1 = c.wx[0] * m0 + c.wx[1] * Rt + wu[1] * cg_hi(up) + c.wy[1] * cg_hi(dn);
  return cg_cat(s0, s1);
}
__device__ __forceinline__ cg_f4 cgr_minv(const CgRec &m, cg_f4 r) {
  const cg_f2 z0 = m.ma[0] * r.x + m.mb[0] * r.y;
  const cg_f2 z1 = m.ma[1] * r.z + m.mb[1] * r.w;
  return cg_cat(z0, z1);
}
// D f with D re-formed from the stored D^-1 (its 2x2 inverse; scalar-Jacobi
// rows, ic = 0, give diag(1/ia, 1/id); all-zero records give D = 0)
__device__ __forceinline__ cg_f4 cgr_diag(const CgRec &m, cg_f4 f) {
  cg_f2 o[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float ia = m.ma[e].x, ic = m.ma[e].y, id = m.mb[e].y;
    const float det = ia * id - ic * ic;
    const float inv = det != 0.f ? __builtin_amdgcn_rcpf(det) : 0.f;
    const cg_f2 da = cg_f2{id, -ic} * inv, db = cg_f2{-ic, ia} * inv;
    const float fu = e ? f.z : f.x, fv = e ? f.w : f.y;
    o[e] = da * fu + db * fv;
  }
  return cg_cat(o[0], o[1]);
}
// D f from the raw coefficient row (wave 0 still holds it): no inverse
__device__ __forceinline__ cg_f4 cgr_diag_raw(const CgRaw &c, cg_f4 f) {
  const cg_f2 u = cg_f2{f.x, f.z}, v = cg_f2{f.y, f.w};
  const cg_f2 du = c.a * u + c.c * v, dv = c.c * u + c.d * v;
  return cg_f4{du.x, dv.x, du.y, dv.y};
}

// ---------------------------------------------------------------------------
// k_cgs: the degree-CG_DEG (5) iteration above with its pipeline stages
// split over the 4 waves of a block, which all work on ONE band:
//   wave 0: loads, coefficient records -> LDS ring, A) r, y of row n-1
//   wave 1: Horner B) g4 (row n-3), g3 (n-4), g2 (n-5), g1 (n-6)
//   wave 2: D) z, p, x of row n-8, E) q, y_q of row n-9
//   wave 3: F) v1 and T1, T2 (row n-11), v2 and T3..T5 (row n-12)
// with one block barrier per row step; rows cross waves through small LDS
// rings (y, g1, y_q; records in a 14-row ring), a wave's own rows stay in
// registers, and so does what a wave has read and needs again at a later
// step: wave 0 its records of rows n-1, n-2 (CGS_W0REG), wave 2 the records
// of rows n-8, n-9 with the vertical weights of row n-10 and the g1 rows
// n-7 .. n-9, wave 3 the records of rows n-11, n-12 with the vertical
// weights of row n-13 and the y_q rows n-10 .. n-12.  Per row step wave 2
// reads one record, one g1 row and one y row from LDS and wave 3 one record
// and one y_q row; wave 1 keeps the records of rows n-3 .. n-6 with the
// vertical weights of row n-7 and reads one record and its five y rows.  The
// vertical weights of the row above a stage's own come out of that row's
// record, never from a read of their own.  (The round-1 form of this iteration, since removed, gave each
// wave its own band and the whole pipeline: its record ring allowed one wave
// per SIMD and 1.6x the rows read.)  Here 74 KB of LDS per block allow 2 blocks per CU (R = 39 at
// 1080p) and a step costs only the heaviest wave's share.  Stage lags follow
// from one barrier per step: a stage reads rows of another wave produced at
// earlier steps; the band is walked for n in [r0 - 8, r1 + 11] (an odd band,
// walked bottom to top, to r1 + 12: stage F's T5 seam edge) so that every
// row a required stage reads was produced.
// Rejected variants of this kernel (record split over waves 0 / 3, the
// round-4 register record rings, raw-D stage E, pair-block splitting, trimmed
// drain loads)
// are recorded with their measurements in DESIGN.md §3; the commits that
// measured them hold their source.
#define CGS_NREC 14
// CGS_W0REG (default 1): wave 0 keeps the records of rows n-1, n-2 it
// formed in registers instead of reading them back from the LDS ring (4
// ds_read_b128 + 2 ds_read_b64 and their wait per row step of the
// pace-setting wave; 184 -> 202 VGPRs, the same 2 waves / SIMD).  Round-5
// A/B, 2 reps, the same flow bitwise (profiles/r5s_cgs_ab.log): isolated
// 200-iteration 1080p solve 3.87 / 3.87 vs 3.96 / 3.92 ms, timed bench 47.95 /
// 47.94 vs 47.94 / 47.87 pairs/s.  Masking the out-of-band rows instead of
// branching over them (one basic block per row step) was 5 % slower as timed.
// Also measured and removed (round 5, profiles/r5u_cgs_w3rec_ab.log): the
// coefficient loads and records moved from wave 0 to wave 3 (one row ahead,
// a 15-row ring): wave 0 101 -> 89 K working cycles per launch but wave 3
// 56 -> 92 K, a 200-iteration 1080p solve 4.19 vs 3.90 ms, 45.0 vs 47.8
// pairs/s, the same flow bitwise.
#ifndef CGS_W0REG
#define CGS_W0REG 1
#endif
// Waves 1 and 3 run at issue priority 1 (0 otherwise), above the
// other lanes' kernels that share their SIMDs in the timed geometry: 45.65 /
// 45.78 / 45.87 vs 45.34 / 45.45 / 45.57 pairs/s, 3 reps each
// (profiles/r4k_prio_ab.log); the same arithmetic

// Load distance in row steps (each step ends at a block barrier, so a load
// issued at step n is waited for at step n + distance): wave 0's coefficient,
// p_old and r_in rows (CGS_PF), wave 2's p_old and x rows (CGS_PF2).  Ring
// sizes are powers of two dividing the 8-step unroll.
#ifndef CGS_PF
#define CGS_PF 2
#endif
// The distance holds only while every row step issues the same memory
// operations: the compiler sizes each s_waitcnt vmcnt for the fewest
// operations any path can have put behind the awaited load.  With wave 2's x
// load and stores under branches it waited with vmcnt(1), i.e. for the p_old
// load of the same step (distance 0, whatever CGS_PF2 said: the round-2
// sweep of 2..4 was flat for that reason).  Unconditional (load_x, so8) the
// wait is vmcnt(5) at distance 1, vmcnt(9) at 2.  Timed bench, 5 alternating
// runs each on one box, the same flow bitwise: conditional 51.01 +- 0.04,
// then CGS_PF2 1 / 2 / 3: 52.55 +- 0.14 / 53.02 +- 0.08 / 52.78 +- 0.04
// pairs/s (profiles/r7_cgs_waits/).
#ifndef CGS_PF2
#define CGS_PF2 2
#endif
#define CGS_POW2(n) ((n) <= 1 ? 1 : (n) <= 2 ? 2 : (n) <= 4 ? 4 : 8)
#define CGS_SGN CGS_POW2(CGS_PF + 2)
#define CGS_RIN CGS_POW2(CGS_PF + 1)
#define CGS_W2N CGS_POW2(CGS_PF2 + 1)
static_assert(CGS_PF >= 1 && CGS_PF + 3 <= 8 && CGS_PF2 >= 1 && CGS_PF2 + 1 <= 8, "k_cgs load distances");

// CGS_PHASE_TIMING (tools/micro builds only): per role, the cycles a wave
// spends working and waiting at the row-step barriers
#ifdef CGS_PHASE_TIMING
__device__ unsigned long long g_cgs_t[4][3];  // [role] {work, wait, waves}
#define CGS_T0 unsigned long long cgs_wait = 0, cgs_t_start = clock64();
#define CGS_BAR_BEGIN const unsigned long long cgs_b0 = clock64();
#define CGS_BAR_END cgs_wait += clock64() - cgs_b0;
#define CGS_T1                                                           \
  if (lane == 0) {                                                       \
    const unsigned long long tot = clock64() - cgs_t_start;              \
    atomicAdd(&g_cgs_t[wid][0], tot - cgs_wait);                         \
    atomicAdd(&g_cgs_t[wid][1], cgs_wait);                               \
    atomicAdd(&g_cgs_t[wid][2], 1ull);                                   \
  }
#else
#define CGS_T0
#define CGS_BAR_BEGIN
#define CGS_BAR_END
#define CGS_T1
#endif

template <int U>
struct CgsStep {  // position of a row step in the 8-step trip (CGS_STEPS)
  static constexpr int value = U;
};

template <bool FIRST, bool ODD>
__global__ __launch_bounds__(256) void k_cgs(PcgArgs g, int k, int R, int nbands) {
  __shared__ double lds[64];
  __shared__ float4 ring[CGS_NREC][4][64];  // [row slot][record quarter][lane]
  __shared__ float4 s_y[8][64], s_g1[4][64], s_yq[4][64];
  const int H = g.H, W = g.W;
  const unsigned rowb4 = (unsigned)g.P * 4u, rowb8 = (unsigned)g.P * 8u;
  const size_t vbytes = (size_t)H * g.P * 8;
  const __amdgpu_buffer_rsrc_t rc = cg_rsrc(g.coef, g.ps * 7 * 4);
  const __amdgpu_buffer_rsrc_t rin = cg_rsrc(FIRST ? g.b : g.r_in, vbytes);
  const __amdgpu_buffer_rsrc_t rpo = cg_rsrc(g.p_old, vbytes);
  const __amdgpu_buffer_rsrc_t rx = cg_rsrc(g.x, vbytes);
  const __amdgpu_buffer_rsrc_t rro = cg_rsrc(g.r_out, vbytes);
  const __amdgpu_buffer_rsrc_t rpn = cg_rsrc(g.p_new, vbytes);
  const unsigned ps4 = (unsigned)(g.ps * 4);
  // XCD-aware tile order: blocks b, b + 8, b + 16 ... share an XCD's L2
  // (MI355X_MICROARCH.md, workgroup dispatch), so give each XCD a contiguous
  // run of row-major tiles; its neighbours' column halos are then read
  // through the same L2 at about the same row step
  const int nt = gridDim.x * gridDim.y, lin = blockIdx.x + blockIdx.y * gridDim.x;
  const int xcd = lin & 7, tile = xcd * (nt >> 3) + min(xcd, nt & 7) + (lin >> 3);
  const int lane = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(threadIdx.y), band = tile / gridDim.x;
  const int tid = lane + wid * 64;
  // pipeline role of this wave (A/B, round 2: pairing the roles of two
  // co-resident blocks differently on the SIMDs, role = wid ^ f(block), was
  // no faster: 51.5-54 vs 52 us per 1080p launch)
  const int role = wid;
  // strip tx spans columns [PCG_SWP tx, PCG_SWP tx + 128): lanes 4..59 are
  // output; the first strip's lanes 0..3 and the last strip's lanes 60..63
  // have no neighbouring strip to recompute for, so they are output too
  const int tx = tile - band * gridDim.x;
  const int jc = tx * PCG_SWP + 2 * lane;
  const bool ok0 = jc < W, ok1 = jc + 1 < W;
  const bool out_lane = (lane >= CGS_HALO || tx == 0) && (lane < 64 - CGS_HALO || tx == (int)gridDim.x - 1);
  const unsigned off4 = ok0 ? (unsigned)jc * 4u : CG_OOB, off8 = ok0 ? (unsigned)jc * 8u : CG_OOB;
  const unsigned soff8 = ok0 && out_lane ? (unsigned)jc * 8u : CG_OOB;
  const bool live = band < nbands;
  // odd bands walk bottom to top, so each band meets its neighbours' halo
  // rows at the same row step (both at the start or both at the end of the
  // walk) and the second read of those rows is served by the XCD's L2.  The
  // walk runs in virtual rows t (orig row H-1-t when flipped); the lower
  // edge of virtual row t is the upper edge of its orig row, i.e. the wy
  // stored at orig row H-2-t.
  const bool flip = band & 1;
  const int rb0 = band * R, rb1 = min(rb0 + R, H);
  const int r0 = flip ? H - rb1 : rb0, r1 = flip ? H - rb0 : rb1;
  const float c0 = g.poly[0], c1 = g.poly[1], c2 = g.poly[2], c3 = g.poly[3], c4 = g.poly[4], c5 = g.poly[5];
  // Row offsets are stepped, not multiplied out per row: virtual row t lies
  // at byte rw8(t) = base8 + t step8 of a vector and rw4(t) of a coefficient
  // plane, in unsigned arithmetic that wraps for the rows of a walk outside
  // the image.  Each role keeps running values that advance by one step per
  // row step (set before the walk; the multiplications below run only there).
  // For the single-plane vectors (range H P 8 bytes) the wrapped offset of a
  // row t < 0 is >= 2^32 - 20 row pitches and that of a row t >= H is >= the
  // range, with or without CG_OOB of an out-of-image column on top, so the
  // descriptor's range check alone returns 0 / drops the access, without
  // memory traffic.  The seven coefficient planes share one descriptor (a row
  // >= H of planes 0..5 is in range), so their offsets keep a validity select.
  const unsigned step4 = flip ? 0u - rowb4 : rowb4, step8 = flip ? 0u - rowb8 : rowb8;
  const unsigned base4 = flip ? (unsigned)(H - 1) * rowb4 : 0u, base8 = flip ? (unsigned)(H - 1) * rowb8 : 0u;
  auto rw4 = [&](int t) { return base4 + (unsigned)t * step4; };
  auto rw8 = [&](int t) { return base8 + (unsigned)t * step8; };
  // wy of virtual row t: the plane row above when flipped (orig row H-2-t)
  const unsigned wadj4 = flip ? rowb4 : 0u, Hw = (unsigned)(flip ? H - 1 : H);
  // row t's coefficients; c4 = rw4(t)
  auto load_raw = [&](int t, unsigned c4, CgRaw &c) {
    const unsigned v = off4 + ((unsigned)t < (unsigned)H ? c4 : CG_ROW_OOB);
    const unsigned vw = off4 + ((unsigned)t < Hw ? c4 - wadj4 : CG_ROW_OOB);
    c.wxu = cg_mask1<ODD>(cg_ld2(rc, v, 0), ok1);
    c.wyu = cg_mask1<ODD>(cg_ld2(rc, vw, ps4), ok1);
    c.wxv = cg_mask1<ODD>(cg_ld2(rc, v, 2 * ps4), ok1);
    c.wyv = cg_mask1<ODD>(cg_ld2(rc, vw, 3 * ps4), ok1);
    c.a = cg_mask1<ODD>(cg_ld2(rc, v, 4 * ps4), ok1);
    c.c = cg_mask1<ODD>(cg_ld2(rc, v, 5 * ps4), ok1);
    c.d = cg_mask1<ODD>(cg_ld2(rc, v, 6 * ps4), ok1);
  };
  // records are keyed by absolute row (rows >= r0 - 7 >= -7)
  auto rslot = [](int t) { return (t + 2 * CGS_NREC) % CGS_NREC; };
  // inside the walk the slot of row n is a running counter (CGS_RS_NEXT) and
  // that of row n - d follows by one subtraction and wrap (rsl): no division
  auto rsl = [](int rs, int d) {
    const int s = rs - d;
    return s < 0 ? s + CGS_NREC : s;
  };
#define CGS_RS_NEXT(rs) rs = (rs) + 1 == CGS_NREC ? 0 : (rs) + 1
  // put_rec / get_rec / get_wy take the slot (get_wy: wave 0 without CGS_W0REG)
  auto put_rec = [&](int slot, const CgRaw &c) {
    CgCoef cc;
    cc.a = c.a;
    cc.c = c.c;
    cc.d = c.d;
    const CgInv mi = cg_inv<true>(cc);
    float4 *q = &ring[slot][0][lane];
    q[0] = make_float4(c.wxu.x, c.wxv.x, c.wyu.x, c.wyv.x);
    q[64] = make_float4(c.wxu.y, c.wxv.y, c.wyu.y, c.wyv.y);
    q[128] = make_float4(mi.ia.x, mi.ic.x, mi.ic.x, mi.id.x);
    q[192] = make_float4(mi.ia.y, mi.ic.y, mi.ic.y, mi.id.y);
    CgRec r;  // the record as get_rec reads it back
    r.wx[0] = cg_f2{c.wxu.x, c.wxv.x};
    r.wy[0] = cg_f2{c.wyu.x, c.wyv.x};
    r.wx[1] = cg_f2{c.wxu.y, c.wxv.y};
    r.wy[1] = cg_f2{c.wyu.y, c.wyv.y};
    r.ma[0] = cg_f2{mi.ia.x, mi.ic.x};
    r.mb[0] = cg_f2{mi.ic.x, mi.id.x};
    r.ma[1] = cg_f2{mi.ia.y, mi.ic.y};
    r.mb[1] = cg_f2{mi.ic.y, mi.id.y};
    return r;
  };
  auto get_rec = [&](int slot) {
    const float4 *q = &ring[slot][0][lane];
    const float4 a = q[0], b = q[64], c = q[128], d = q[192];
    CgRec r;
    r.wx[0] = cg_f2{a.x, a.y};
    r.wy[0] = cg_f2{a.z, a.w};
    r.wx[1] = cg_f2{b.x, b.y};
    r.wy[1] = cg_f2{b.z, b.w};
    r.ma[0] = cg_f2{c.x, c.y};
    r.mb[0] = cg_f2{c.z, c.w};
    r.ma[1] = cg_f2{d.x, d.y};
    r.mb[1] = cg_f2{d.z, d.w};
    return r;
  };
#if !CGS_W0REG
  auto get_wy = [&](int slot, cg_f2 (&wu)[2]) {  // vertical weight pairs only
    const float2 *q = reinterpret_cast<const float2 *>(&ring[slot][0][lane]);
    const float2 a = q[1], b = q[129];
    wu[0] = cg_f2{a.x, a.y};
    wu[1] = cg_f2{b.x, b.y};
  };
#endif
  auto ld4 = [&](float4 (&rg)[4][64], int t) {
    const float4 v = rg[t & 3][lane];
    return cg_f4{v.x, v.y, v.z, v.w};
  };
  auto st4 = [&](float4 (&rg)[4][64], int t, cg_f4 v) { rg[t & 3][lane] = make_float4(v.x, v.y, v.z, v.w); };
  // (c8 = rw8(row): out-of-image rows are refused by the range check, above)
  auto load_po = [&](unsigned c8) {
    return FIRST ? cg_f4{0.f, 0.f, 0.f, 0.f} : cg_mask1<ODD>(cg_ld4(rpo, off8 + c8), ok1);
  };
  auto load_rin = [&](unsigned c8) { return cg_mask1<ODD>(cg_ld4(rin, off8 + c8), ok1); };
  // x_lo = 0 in the launch after a residual replacement (xz, known after
  // the prologue; the preamble's x rows are then dropped)
  bool xz = false;
  // (always issued: outside the band, and after xz, from an out-of-range
  // offset that returns 0 without memory traffic.  A branch around the load
  // makes the count of memory operations behind an earlier load depend on
  // the path, and the wait before that load's use then covers this step's)
  const unsigned nrb = (unsigned)(r1 - r0);  // rows of the band
  auto load_x = [&](int t, unsigned c8) {
    if (FIRST) return cg_f4{0.f, 0.f, 0.f, 0.f};
    return cg_mask1<ODD>(cg_ld4(rx, off8 + (!xz && (unsigned)(t - r0) < nrb ? c8 : CG_ROW_OOB)), ok1);
  };
  const bool dm0 = out_lane && ok0, dm1 = out_lane && ok1;
  // (jc is even, so in the even-width instances dm0 == dm1 and one select per
  // masked sum, dm0 ? a + b : 0, gives the same bits, as does one condition
  // for stage D's mask on p.  Measured and left out: the compiler then
  // branches around the sums; per steady step of <false, false> wave 2 grows
  // 171 -> 178 instructions (v_mov_b32 23 -> 35) and wave 3 121 -> 129, and
  // the timed bench loses 0.5 %: 56.28 +- 0.06 vs 56.59 +- 0.07 pairs/s, 5
  // alternating runs each on one box (profiles/cgs_record_reads/))
  auto mdot = [&](cg_f4 a, cg_f4 b) {
    const cg_f2 p = cg_lo(a) * cg_lo(b), q = cg_hi(a) * cg_hi(b);
    return (dm0 ? p.x + p.y : 0.f) + (dm1 ? q.x + q.y : 0.f);
  };
  const cg_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // (a flipped band walks one step further: stage F's T5 there also takes the
  // edge below its last virtual row, which needs v2 of row r1)
  const int ns = r0 - 8, ne = r1 + 11 + (flip ? 1 : 0);

  // zeroed rings: rows above the band that no required stage reads
  {
    float4 *z = &ring[0][0][0];
    for (int e = tid; e < CGS_NREC * 4 * 64; e += 256) z[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < 8 * 64; e += 256) (&s_y[0][0])[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < 4 * 64; e += 256) {
      (&s_g1[0][0])[e] = make_float4(0.f, 0.f, 0.f, 0.f);
      (&s_yq[0][0])[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // wave 0: raw rows ns-2 .. ns+PF-1, p_old rows ns-2 .. ns+PF-1, r_in rows
  // ns-1 .. ns+PF-2; wave 2: p_old, x of rows ns-8 .. ns-9+PF2 (register
  // rings indexed by (row - ns) mod ring size)
  CgRaw SG[CGS_SGN], SGp[2];
  cg_f4 PO[8], RI[CGS_RIN], PO2[CGS_W2N], XI[CGS_W2N];
  if (live && role == 0) {
    load_raw(ns - 2, rw4(ns - 2), SGp[0]);
    load_raw(ns - 1, rw4(ns - 1), SGp[1]);
#pragma unroll
    for (int m = 0; m < CGS_PF; ++m) load_raw(ns + m, rw4(ns + m), SG[m]);
    SG[CGS_SGN - 1] = SGp[1];  // raw row ns-1: stage A's D at the first step
#pragma unroll
    for (int m = -2; m < CGS_PF; ++m) PO[m & 7] = load_po(rw8(ns + m));
#pragma unroll
    for (int m = -1; m < CGS_PF - 1; ++m) RI[(m + 16) & (CGS_RIN - 1)] = load_rin(rw8(ns + m));
  }
  if (live && role == 2) {
#pragma unroll
    for (int m = -8; m < CGS_PF2 - 8; ++m) {
      PO2[(m + 16) & (CGS_W2N - 1)] = load_po(rw8(ns + m));
      XI[(m + 16) & (CGS_W2N - 1)] = load_x(ns + m, rw8(ns + m));
    }
  }
  float alpha = 0.f, beta = 0.f;
  if (cg_prologue<FIRST>(g, k, lds, &alpha, &beta, &xz)) return;
  if (xz)
#pragma unroll
    for (int m = 0; m < CGS_W2N; ++m) XI[m] = zero4;

  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  CgRec QA[2];  // CGS_W0REG: wave 0's records of rows n - 2, n - 1 (by R2)
  // row o inside the band (stores and dot products only there); so8: the
  // store offset of row o, out of range (the store is dropped) outside the
  // band, so that every row step issues the same memory operations
  auto inband = [&](int o) { return (unsigned)(o - r0) < nrb; };
  // (the empty asm keeps the select: without it the compiler threads the
  // stores back into the two arms of the inband branch below them)
  auto so8 = [&](int o, unsigned c8) {  // c8 = rw8(o)
    unsigned ro = inband(o) ? c8 : CG_ROW_OOB;
    asm("" : "+s"(ro));
    return soff8 + ro;
  };
  if (live) {
    if (role == 0) {
      QA[0] = put_rec(rslot(ns - 2), SGp[0]);  // ring slots of rows ns - 2, ns - 1 at u = 0
      QA[1] = put_rec(rslot(ns - 1), SGp[1]);
    }
    __syncthreads();
    CGS_T0
    // issue priority for the pace-setting roles (loads + stage A, and z / p /
    // q) over the Horner and T waves they share a SIMD with: 52 -> 50 us
    // per 1080p launch (A/B, profiles/r2z_cgs_setprio_ab.log; wave 0
    // alone: 51.3)
    if (role == 0 || role == 2) __builtin_amdgcn_s_setprio(2);
    // the Horner and T waves above other kernels' waves on their SIMD (the
    // timed lanes run a fine solve one block per CU beside other lanes' work)
    else __builtin_amdgcn_s_setprio(1);
    // each wave runs its own role's loop (registers of one role only), one
    // block barrier per row step in every role (same step count).  A trip is
    // eight row steps, each an instance of one generic lambda: u is a
    // compile-time constant where the register rings are indexed, so the
    // rings are split into registers before any loop pass sees them (as an
    // unrolled loop over u they were kept as 32-register tuples, which the
    // register allocator copied whole: up to 80 moves in a row step).  Whole
    // trips run without a test between their steps; only the last, partial
    // trip tests n against ne.  With the test inside every step the compiler
    // merged the early exits into a flag tested at the top of the next step,
    // i.e. a path that reaches a step without the memory operations of the
    // step before, and sized every vmcnt wait for that path (load distance 1
    // instead of CGS_PF / CGS_PF2; see the note above CGS_PF2)
#define CGS_STEPS(...)                                                    \
  {                                                                       \
    auto cgs_step = [&](int n0, auto cgs_u) __attribute__((always_inline)) { \
      constexpr int u = decltype(cgs_u)::value;                           \
      const int n = n0 + u;                                               \
      __VA_ARGS__                                                         \
      CGS_BAR_BEGIN                                                       \
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");              \
      __builtin_amdgcn_s_barrier();                                       \
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");              \
      CGS_BAR_END                                                         \
    };                                                                    \
    int n0 = ns;                                                          \
    for (; n0 + 7 <= ne; n0 += 8) {                                       \
      cgs_step(n0, CgsStep<0>{});                                         \
      cgs_step(n0, CgsStep<1>{});                                         \
      cgs_step(n0, CgsStep<2>{});                                         \
      cgs_step(n0, CgsStep<3>{});                                         \
      cgs_step(n0, CgsStep<4>{});                                         \
      cgs_step(n0, CgsStep<5>{});                                         \
      cgs_step(n0, CgsStep<6>{});                                         \
      cgs_step(n0, CgsStep<7>{});                                         \
    }                                                                     \
    do {                                                                  \
      if (n0 > ne) break;                                                 \
      cgs_step(n0, CgsStep<0>{});                                         \
      if (n0 + 1 > ne) break;                                             \
      cgs_step(n0, CgsStep<1>{});                                         \
      if (n0 + 2 > ne) break;                                             \
      cgs_step(n0, CgsStep<2>{});                                         \
      if (n0 + 3 > ne) break;                                             \
      cgs_step(n0, CgsStep<3>{});                                         \
      if (n0 + 4 > ne) break;                                             \
      cgs_step(n0, CgsStep<4>{});                                         \
      if (n0 + 5 > ne) break;                                             \
      cgs_step(n0, CgsStep<5>{});                                         \
      if (n0 + 6 > ne) break;                                             \
      cgs_step(n0, CgsStep<6>{});                                         \
    } while (0);                                                          \
  }
// register-ring index of row n + d: (u + d) mod ring size
#define R8(d) ((u + (d) + 16) & 7)
#define R4(d) ((u + (d) + 16) & 3)
#define R2(d) ((u + (d) + 16) & 1)
#define RSG(d) ((u + (d) + 16) & (CGS_SGN - 1))
#define RRI(d) ((u + (d) + 16) & (CGS_RIN - 1))
#define RW2(d) ((u + (d) + 16) & (CGS_W2N - 1))
    if (role == 0) {
      // running offsets of rows n + PF (c4, c8), n + PF - 1 (c8p), n - 1 (cs)
      unsigned c4 = rw4(ns + CGS_PF), c8 = rw8(ns + CGS_PF), c8p = rw8(ns + CGS_PF - 1), cs = rw8(ns - 1);
      int rs = rslot(ns);
      CGS_STEPS({
        load_raw(n + CGS_PF, c4, SG[RSG(CGS_PF)]);
        PO[R8(CGS_PF)] = load_po(c8);
        RI[RRI(CGS_PF - 1)] = load_rin(c8p);
        // A) row n-1: r = r_in - alpha A p_old, y = D^-1 r
#if CGS_W0REG
        const cg_f2 wu[2] = {QA[R2(-2)].wy[0], QA[R2(-2)].wy[1]};  // before row n takes the slot
        const CgRec q1 = QA[R2(-1)];
        QA[R2(0)] = put_rec(rs, SG[RSG(0)]);
#else
        put_rec(rs, SG[RSG(0)]);
        const CgRec q1 = get_rec(rsl(rs, 1));
        cg_f2 wu[2];
        get_wy(rsl(rs, 2), wu);
#endif
        cg_f4 r = RI[RRI(-1)];
        if (!FIRST) r -= alpha * (cgr_diag_raw(SG[RSG(-1)], PO[R8(-1)]) - cgr_nsum(PO[R8(-2)], PO[R8(-1)], PO[R8(0)], q1, wu));
        const cg_f4 y = cgr_minv(q1, r);
        s_y[(n - 1) & 7][lane] = make_float4(y.x, y.y, y.z, y.w);
        const int o = n - 1;
        cg_st4(rro, so8(o, cs), r);
        if (inband(o)) {
          acc[4] += (double)mdot(r, r);
          acc[3] += (double)(c0 * mdot(r, y));
        }
        c4 += step4;
        c8p = c8;
        c8 += step8;
        cs += step8;
        CGS_RS_NEXT(rs);
      })
    } else if (role == 1) {
      // Horner, degree 5: g4 = c4 y + c5 B y (row n-3), g3 = c3 y + B g4
      // (n-4), g2 = c2 y + B g3 (n-5), g1 = c1 y + B g2 (n-6) -> LDS
      cg_f4 G4[4] = {zero4, zero4, zero4, zero4}, G3[4] = {zero4, zero4, zero4, zero4};
      cg_f4 G2[4] = {zero4, zero4, zero4, zero4};
      auto yrow = [&](int t) {
        const float4 a = s_y[t & 7][lane];
        return cg_f4{a.x, a.y, a.z, a.w};
      };
      // Carried as in waves 2 and 3: RB the records of rows n-3 (read at this
      // step for g4) .. n-6, by R4; the slot row n-3 takes held row n-7, whose
      // wy is g1's wu (w7) and is taken out first.  Before: 4 records and the
      // wy pair of row n-7 per step (23 LDS instructions per steady step of
      // <false, false>, now 10: one record, five y rows, the g1 write; 128 ->
      // 114 instructions, the same 24 v_mov_b32, 246 -> 226 VGPRs).
      // RB is initialised to 0 at loop entry, which is what reading those
      // records after the first __syncthreads() would return.  Wave 0 stores
      // the record of row r at step r (rows ns-2, ns-1 before the walk), a
      // barrier ahead of this wave's first read of it at step r + 3; the
      // reads this replaces are at steps r + 4 .. r + 7 (r + 7: the wy alone),
      // and the slot is next stored with row r + 14 at step r + 14, so what
      // was read at step r + 3 is what they return.  Rows ns-4 .. ns-7, which
      // RB stands for at step ns, are below ns - 2 and never stored; their
      // zeroed slots are first stored at steps ns + 10 .. ns + 7, after the
      // last reads of those rows at steps ns + 3 .. ns.
      // Timed bench, 5 alternating runs each on one box, the same iterates and
      // flow bitwise (profiles/cgs_wave1_reads/): parent 56.20 +- 0.13, RB
      // 57.01 +- 0.12 pairs/s (second box 56.19 +- 0.07, 56.93 +- 0.04).
      // Also measured and left out, neither clearing 3 sd on either box:
      // + the y rows n-3 .. n-6 carried in a ring YR[8] by R8, one s_y read
      //   per step (6 LDS instructions, 106 instructions, 240 VGPRs): 57.01
      //   +- 0.12 (second box 57.10 +- 0.06, +0.3 %, 2.8 sd);
      // + the slot from the running counter as in the other roles instead of
      //   rslot(): on RB alone 57.06 +- 0.10 (second box only), on RB + YR
      //   57.22 +- 0.32 (57.03 +- 0.12).  The steady step has the same
      //   instruction counts with it: the compiler already steps the slot.
      CgRec RB[4] = {};
#define CGS_Y1(d) yrow(n + (d))
      CGS_STEPS({
        const cg_f2 w7[2] = {RB[R4(-7)].wy[0], RB[R4(-7)].wy[1]};  // before row n-3 takes the slot
        RB[R4(-3)] = get_rec(rslot(n - 3));
        // the wu of a stage is the wy of the next stage's record
        const CgRec q3 = RB[R4(-3)], q4 = RB[R4(-4)], q5 = RB[R4(-5)], q6 = RB[R4(-6)];
        {
          const cg_f4 y0 = CGS_Y1(-3);
          const cg_f4 ny = cgr_nsum(CGS_Y1(-4), y0, CGS_Y1(-2), q3, q4.wy);
          G4[R4(-3)] = c4 * y0 + c5 * cgr_minv(q3, ny);
        }
        {
          const cg_f4 ng = cgr_nsum(G4[R4(-5)], G4[R4(-4)], G4[R4(-3)], q4, q5.wy);
          G3[R4(-4)] = c3 * CGS_Y1(-4) + cgr_minv(q4, ng);
        }
        {
          const cg_f4 ng = cgr_nsum(G3[R4(-6)], G3[R4(-5)], G3[R4(-4)], q5, q6.wy);
          G2[R4(-5)] = c2 * CGS_Y1(-5) + cgr_minv(q5, ng);
        }
        {
          const cg_f4 ng = cgr_nsum(G2[R4(-7)], G2[R4(-6)], G2[R4(-5)], q6, w7);
          st4(s_g1, n - 6, c1 * CGS_Y1(-6) + cgr_minv(q6, ng));
        }
      })
#undef CGS_Y1
    } else if (role == 2) {
      cg_f4 PP[4] = {zero4, zero4, zero4, zero4}, ZZ[2] = {zero4, zero4};
      // What the wave read and needs again: RD the records of rows n-8 (read
      // at this step for stage D) and n-9 (read one step ago, now stage E's;
      // its wy is stage D's wu), by R2; the slot row n-8 takes held row n-10,
      // whose wy is stage E's wu.  G1 the g1 rows n-9 .. n-7 by R4, row n-7
      // read at this step.  Before: 2 records, 2 wy pairs and 3 g1 rows per
      // step (14 LDS instructions per steady step of <false, false>, now 7;
      // 191 -> 171 instructions, the same 23 v_mov_b32).
      // At loop entry they are initialised to 0, which is what reading them
      // after the first __syncthreads() would return: the record of a row
      // r < ns - 2 shares its ring slot with row r + 14, which wave 0 stores
      // at step r + 14, after the last read of row r at step r + 10 (wave
      // 3: r + 13), so every read of rows ns-10 .. ns-9 (wave 3: ns-13 ..
      // ns-12) sees the zeroed slot; a g1 (y_q) row r is stored at step r +
      // 6 (r + 9), which for rows ns-9, ns-8 (ns-12, ns-11) is before the
      // walk, i.e. never, and its slot is next stored at step r + 10 (r +
      // 13), after its last read at step r + 9 (r + 12).
      // Timed bench, 5 alternating runs each on one box, the same flow
      // bitwise (profiles/cgs_record_reads/): parent 54.91 +- 0.09, the wy
      // of a record read in the same step taken from it 55.19 +- 0.07, +
      // wave 2's carried rows 56.04 +- 0.06, + wave 3's 56.59 +- 0.07
      // pairs/s; wave 2 72.3 K -> 58.0 K working cycles per launch.  (The
      // round-4 rings of DESIGN.md §3 were 7 % slower as timed; then wave 0
      // set the step and the rings were copied whole.)
      // Also measured and left out: each wave's one new record read issued
      // at the end of the step before (its row is two barriers old), to be in
      // flight across the barrier: 57.04 +- 0.19 vs 57.06 +- 0.05 pairs/s,
      // the fence before the barrier waits for the read anyway.
      CgRec RD[2] = {};
      cg_f4 G1[4] = {zero4, zero4, zero4, zero4};
      // running offsets of rows n + PF2 - 8 (c8) and n - 8 (cs)
      unsigned c8 = rw8(ns + CGS_PF2 - 8), cs = rw8(ns - 8);
      int rs = rslot(ns);
      CGS_STEPS({
        PO2[RW2(CGS_PF2 - 8)] = load_po(c8);
        XI[RW2(CGS_PF2 - 8)] = load_x(n + CGS_PF2 - 8, c8);
        // D) row n-8: z = c0 y + D^-1 N g1, p = z + beta p_old, x += alpha p_old
        const cg_f2 wuE[2] = {RD[R2(-10)].wy[0], RD[R2(-10)].wy[1]};  // before row n-8 takes the slot
        RD[R2(-8)] = get_rec(rsl(rs, 8));
        G1[R4(-7)] = ld4(s_g1, n - 7);
        {
          const CgRec q4 = RD[R2(-8)];
          const cg_f4 ng = cgr_nsum(G1[R4(-9)], G1[R4(-8)], G1[R4(-7)], q4, RD[R2(-9)].wy);
          const float4 b = s_y[(n - 8) & 7][lane];
          const cg_f4 yr = {b.x, b.y, b.z, b.w};
          const cg_f4 z = c0 * yr + cgr_minv(q4, ng);
          cg_f4 p = FIRST ? z : z + beta * PO2[RW2(-8)];
          const int o = n - 8;
          const bool rv = (unsigned)o < (unsigned)H;
          if (!(rv && ok0)) { p.x = 0.f; p.y = 0.f; }
          if (!(rv && ok1)) { p.z = 0.f; p.w = 0.f; }
          PP[R4(-8)] = p;
          ZZ[R2(-8)] = z;
          const unsigned so = so8(o, cs);
          cg_st4(rpn, so, p);
          cg_st4(rx, so, FIRST ? zero4 : XI[RW2(-8)] + alpha * PO2[RW2(-8)]);
          if (inband(o)) acc[3] += (double)mdot(yr, ng);
        }
        // E) row n-9: q = A p, y_q = D^-1 q
        {
          const CgRec q5 = RD[R2(-9)];
          const cg_f4 pm = PP[R4(-9)];
          const cg_f4 q = cgr_diag(q5, pm) -
                          cgr_nsum(PP[R4(-10)], pm, PP[R4(-8)], q5, wuE);
          const cg_f4 yq = cgr_minv(q5, q);
          st4(s_yq, n - 9, yq);
          const int o = n - 9;
          if (inband(o)) {
            acc[0] += (double)mdot(pm, q);
            acc[1] += (double)mdot(q, ZZ[R2(-9)]);
            acc[2] += (double)(c0 * mdot(q, yq));
          }
        }
        c8 += step8;
        cs += step8;
        CGS_RS_NEXT(rs);
      })
    } else {
      // q.M^-1 q = sum_i c_i T_i with v0 = y_q, v1 = B v0, v2 = B v1:
      // T1 = v0.N v0, T2 = v1.N v0 (row n-11); T3 = v1.N v1, T4 = v2.N v1,
      // T5 = v2.N v2 (row n-12; T5 counts each edge once, by its right /
      // lower pixel)
      cg_f4 V1[4] = {zero4, zero4, zero4, zero4}, V2[2] = {zero4, zero4};
      // carried as in wave 2 (see there for the values at loop entry): RF the
      // records of rows n-11 (read at this step) and n-12, whose wy is the wu
      // of row n-11; the slot row n-11 takes held row n-13, whose wy is wy7.
      // YQ the y_q rows n-12 .. n-10, row n-10 read at this step.  12 -> 5
      // LDS instructions per steady step, 144 -> 121 instructions
      CgRec RF[2] = {};
      cg_f4 YQ[4] = {zero4, zero4, zero4, zero4};
      int rs = rslot(ns);
      const int ve0 = flip ? r0 : r0 + 1;
      const unsigned nve = flip ? nrb + 1u : nrb - 1u;
      CGS_STEPS({
        // row n's record: raw since wave 0 stored it at step n - 1; stage A
        // reads it at step n + 1
        const cg_f2 wy7[2] = {RF[R2(-13)].wy[0], RF[R2(-13)].wy[1]};  // before row n-11 takes the slot
        RF[R2(-11)] = get_rec(rsl(rs, 11));
        YQ[R4(-10)] = ld4(s_yq, n - 10);
        {
          const CgRec q6 = RF[R2(-11)];
          const cg_f4 yq = YQ[R4(-11)];
          const cg_f4 ny = cgr_nsum(YQ[R4(-12)], yq, YQ[R4(-10)], q6, RF[R2(-12)].wy);
          const cg_f4 v1 = cgr_minv(q6, ny);
          V1[R4(-11)] = v1;
          const int o = n - 11;
          if (inband(o)) {
            const cg_f4 t = (c1 * yq + c2 * v1) * ny;
            acc[2] += (double)((dm0 ? t.x + t.y : 0.f) + (dm1 ? t.z + t.w : 0.f));
          }
        }
        {
          const CgRec q7 = RF[R2(-12)];
          const cg_f4 v1 = V1[R4(-12)];
          const cg_f4 nv = cgr_nsum(V1[R4(-13)], v1, V1[R4(-11)], q7, wy7);
          const cg_f4 v2 = cgr_minv(q7, nv);
          const cg_f4 vu = V2[R2(-13)];
          V2[R2(-12)] = v2;
          const int o = n - 12;
          // T5's vertical edge (o - 1, o), once over the level: the walk of
          // an odd band is flipped, so both of its seam edges lie above one of
          // its virtual rows r0 .. r1 (the band below it in the walk is even
          // and cannot take the edge: it has no v2 past its own last row);
          // an even band then takes its inner edges only
          // (flipped: o in [r0, r1]; else o in (r0, r1): one range test, its
          // bounds set before the walk)
          const bool vedge = (unsigned)(o - ve0) < nve;
          if (inband(o)) {
            const cg_f2 w0 = cg_lo(v2), w1 = cg_hi(v2);
            const cg_f2 h0 = cg_left2(q7.wx[1]) * cg_left2(w1);
            const cg_f2 h1 = q7.wx[0] * w0;
            const cg_f4 t = (c3 * v1 + c4 * v2) * nv + (2.0f * c5) * v2 * cg_cat(h0, h1);
            acc[2] += (double)((dm0 ? t.x + t.y : 0.f) + (dm1 ? t.z + t.w : 0.f));
          }
          if (vedge) {
            const cg_f4 t = (2.0f * c5) * v2 * cg_cat(wy7[0] * cg_lo(vu), wy7[1] * cg_hi(vu));
            acc[2] += (double)((dm0 ? t.x + t.y : 0.f) + (dm1 ? t.z + t.w : 0.f));
          }
        }
        CGS_RS_NEXT(rs);
      })
    }
#undef R8
#undef R4
#undef R2
#undef RSG
#undef RRI
#undef RW2
#undef CGS_STEPS
#undef CGS_RS_NEXT
    CGS_T1
  }
  write_partials<5>(acc, g.part_wr, lds);
}
