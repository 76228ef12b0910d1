// kernels_assemble.hip — assembly of the matrix-free flow operator
// (SURVEY.md §8a rows a8-a12): one pixel's row of the 2 x 2-block 5-point
// system, seven coefficient planes and a float2 right-hand side (assemble_px),
// from derivative planes (k_flow_operator) or fused with the warp
// (k_warp_operator), each in one instance per penalty mode (PenMode) and with
// or without the per-pixel data weight, and the fp64 assembly AltBA needs
// (k_flow_operator_f64).  Expects kernels_warp.hip before it (warp_pixel,
// RegOut).  host_flow.hip picks the instance (pen_mode, OF_BY_PM); the
// solver files read the planes.  See DESIGN.md for the roofline.
#include "kernels.h"

// Penalty mode of an assembly kernel: OF_PM_ANY decides everything at run
// time (use_q / use_r, each penalty's kind); otherwise the system is the
// quadratic relaxation only (OF_PM_Q, alpha == 1, every penalty quadratic) or
// the robust one only (OF_PM_R(kind), alpha == 0, every robust penalty of
// that kind).  The arithmetic is the generic form's, term for term.
#define OF_PM_ANY (-1)
#define OF_PM_Q 0
#define OF_PM_R(kind) (1 + (kind))
template <int M>
struct PenMode {
  static constexpr bool any = M == OF_PM_ANY;
  static constexpr int kind = M == OF_PM_ANY ? -1 : M == OF_PM_Q ? OF_PEN_QUADRATIC : M - 1;
  __device__ static bool q(const OpArgs &o) { return any ? o.use_q : M == OF_PM_Q; }
  __device__ static bool r(const OpArgs &o) { return any ? o.use_r : M != OF_PM_Q; }
  __device__ static float pen(const PenF &p, float x) { return pen_k<kind>(p, x); }
};

template <int M = OF_PM_ANY>
__device__ __forceinline__ float2 edge_w(const OpArgs &o, int axis, float du, float dv) {
  OF_NOCONTRACT
  using PM = PenMode<M>;
  float wu = 0.0f, wv = 0.0f;
  if (PM::q(o)) { wu += o.aq_s * PM::pen(o.qsu[axis], du); wv += o.aq_s * PM::pen(o.qsv[axis], dv); }
  if (PM::r(o)) { wu += o.ar_s * PM::pen(o.rsu[axis], du); wv += o.ar_s * PM::pen(o.rsv[axis], dv); }
  return make_float2(wu, wv);
}

__device__ __forceinline__ float2 ld_uvd(const float2 *uv, const float2 *duv, size_t k) {
  float2 a = uv[k];
  if (duv) { float2 b = duv[k]; a.x += b.x; a.y += b.y; }
  return a;
}

// The flow at a pixel and its four neighbours, loaded together at clamped
// indices (a neighbour outside the image reads the pixel itself; its value
// is never used) and pinned in registers right away: loaded under the
// boundary branches, each load was a masked load waited for on its own --
// four more memory round trips per pixel row of the fused warp + assembly,
// after the gather's.
struct UvNbr {
  float2 c, r, d, l, u;
};
__device__ __forceinline__ UvNbr ld_nbr(const float2 *__restrict__ uv, int i, int j, int H, int W, int P) {
  const size_t k = (size_t)i * P + j;
  UvNbr n;
  n.c = uv[k];
  n.r = uv[j < W - 1 ? k + 1 : k];
  n.d = uv[i < H - 1 ? k + P : k];
  n.l = uv[j > 0 ? k - 1 : k];
  n.u = uv[i > 0 ? k - P : k];
  asm volatile("" : "+v"(n.c.x), "+v"(n.c.y), "+v"(n.r.x), "+v"(n.r.y), "+v"(n.d.x), "+v"(n.d.y), "+v"(n.l.x),
               "+v"(n.l.y), "+v"(n.u.x), "+v"(n.u.y));
  return n;
}

// coef planes: 0 wx_u, 1 wy_u, 2 wx_v, 3 wy_v, 4 a_uu, 5 a_uv, 6 a_vv; rhs float2.
// One pixel's row of the system; deriv(ch, It, Ix, Iy) fetches channel ch's
// derivatives (planes, or the fused kernel's registers).  nb: the flow of
// the pixel and its neighbours already in registers (ld_nbr; only without
// duv), else loaded here.  WT: the data term carries the per-pixel weight
// wgt[k] (a plane pitched like an Img plane; include/optflow.h, "Per-pixel
// data-term weights"): psi * wgt[k], one fp32 product, stands in for psi.
template <int NC, int M, bool WT, typename Deriv>
__device__ __forceinline__ void assemble_px(const OpArgs &o, const float2 *__restrict__ uv,
                                            const float2 *__restrict__ duv, int nc_rt, const float2 *__restrict__ uvhat,
                                            int i, int j, int H, int W, int P, size_t ps, float *__restrict__ coef,
                                            float2 *__restrict__ rhs, const float *__restrict__ wgt, const Deriv &deriv,
                                            const UvNbr *nb = nullptr) {
  OF_NOCONTRACT
  using PM = PenMode<M>;
  const int nc = NC > 0 ? NC : nc_rt;
  const size_t k = (size_t)i * P + j;
  const float2 c = nb ? nb->c : ld_uvd(uv, duv, k);
  float2 eR = make_float2(0.f, 0.f), eD = eR, eL = eR, eU = eR;
  if (j < W - 1) { float2 n = nb ? nb->r : ld_uvd(uv, duv, k + 1); eR = edge_w<M>(o, 0, n.x - c.x, n.y - c.y); }
  if (i < H - 1) { float2 n = nb ? nb->d : ld_uvd(uv, duv, k + P); eD = edge_w<M>(o, 1, n.x - c.x, n.y - c.y); }
  if (j > 0) { float2 n = nb ? nb->l : ld_uvd(uv, duv, k - 1); eL = edge_w<M>(o, 0, c.x - n.x, c.y - n.y); }
  if (i > 0) { float2 n = nb ? nb->u : ld_uvd(uv, duv, k - P); eU = edge_w<M>(o, 1, c.x - n.x, c.y - n.y); }
  // data term, channel-averaged (classic_nl.py:330-343)
  float du = 0.f, dv = 0.f;
  if (duv) { du = duv[k].x; dv = duv[k].y; }
  float psq = 0.f, psr = 0.f, ix2 = 0.f, iy2 = 0.f, ixy = 0.f, itx = 0.f, ity = 0.f;
#pragma unroll
  for (int ch = 0; ch < nc; ++ch) {
    float it, gx, gy;
    deriv(ch, it, gx, gy);
    const float itl = it + gx * du + gy * dv;
    if (PM::q(o)) psq += PM::pen(o.qd, itl);
    if (PM::r(o)) psr += PM::pen(o.rd, itl);
    ix2 += gx * gx; iy2 += gy * gy; ixy += gx * gy;
    itx += itl * gx; ity += itl * gy;
  }
  const float inv = 1.0f / (float)nc;
  float psi = ((PM::q(o) ? o.aq_d * psq : 0.f) + (PM::r(o) ? o.ar_d * psr : 0.f)) * inv;
  if (WT) psi = psi * wgt[k];
  ix2 *= inv; iy2 *= inv; ixy *= inv; itx *= inv; ity *= inv;
  // b uses uv (not uv + duv): classic_nl.py:362-367
  const float2 u0 = nb ? nb->c : uv[k];
  float lu = 0.f, lv = 0.f;
  if (j < W - 1) { float2 n = nb ? nb->r : uv[k + 1]; lu += eR.x * (u0.x - n.x); lv += eR.y * (u0.y - n.y); }
  if (i < H - 1) { float2 n = nb ? nb->d : uv[k + P]; lu += eD.x * (u0.x - n.x); lv += eD.y * (u0.y - n.y); }
  if (j > 0) { float2 n = nb ? nb->l : uv[k - 1]; lu += eL.x * (u0.x - n.x); lv += eL.y * (u0.y - n.y); }
  if (i > 0) { float2 n = nb ? nb->u : uv[k - P]; lu += eU.x * (u0.x - n.x); lv += eU.y * (u0.y - n.y); }
  float auu = psi * ix2 + (eL.x + eR.x + eU.x + eD.x);
  float avv = psi * iy2 + (eL.y + eR.y + eU.y + eD.y);
  float bu = -lu - psi * itx, bv = -lv - psi * ity;
  if (uvhat) {  // AltBA coupling (alt_ba.py:236-242)
    const float2 h = uvhat[k];
    const float tu = pen_w(o.rc, u0.x - h.x), tv = pen_w(o.rc, u0.y - h.y);
    auu += o.lambda2 * tu;
    avv += o.lambda2 * tv;
    bu += o.lambda2 * tu * (h.x - u0.x);
    bv += o.lambda2 * tv * (h.y - u0.y);
  }
  coef[k] = eR.x;
  coef[ps + k] = eD.x;
  coef[2 * ps + k] = eR.y;
  coef[3 * ps + k] = eD.y;
  coef[4 * ps + k] = auu;
  coef[5 * ps + k] = psi * ixy;
  coef[6 * ps + k] = avv;
  rhs[k] = make_float2(bu, bv);
}

// WT: the data term is multiplied by the weight plane wgt (assemble_px);
// without it wgt is never read and the host passes nullptr.
template <bool WT, int M>
__global__ __launch_bounds__(OF_BX *OF_BY) void k_flow_operator(OpArgs o, const float2 *__restrict__ uv, const float2 *__restrict__ duv,
                                const float *__restrict__ It, const float *__restrict__ Ix, const float *__restrict__ Iy,
                                int nc, const float2 *__restrict__ uvhat, int H, int W, int P, size_t ps,
                                float *__restrict__ coef, float2 *__restrict__ rhs, const float *__restrict__ wgt) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    assemble_px<0, M, WT>(o, uv, duv, nc, uvhat, i, j, H, W, P, ps, coef, rhs, wgt,
                          [&](int ch, float &it, float &gx, float &gy) {
      const size_t kc = ch * ps + k;
      it = It[kc];
      gx = Ix[kc];
      gy = Iy[kc];
    });
  }
}

// Warp + derivatives + assembly in one pass: the
// per-channel It / Ix / Iy of a pixel stay in registers, so the 24 B/px
// round trip of the three planes (nc = 1) and one launch per warping
// iteration go away.  The same arithmetic as k_partial_deriv +
// k_flow_operator, bitwise: no fma contraction in either (OF_WARP_NOCONTRACT;
// tests/test_gpu_stages.py), with the data weight as well (WT, as above).
template <bool WT, int INTERP, int NC, int M>
__global__ __launch_bounds__(OF_BX *OF_BY) void k_warp_operator(DerivArgs d, OpArgs o, const float2 *__restrict__ uv,
                                                                int H, int W, int P, size_t ps,
                                                                float *__restrict__ coef, float2 *__restrict__ rhs,
                                                                const float *__restrict__ wgt) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    // the pixel's and its neighbours' flow in one round trip, before the
    // gather that needs the pixel's
    const UvNbr nb = ld_nbr(uv, i, j, H, W, P);
    const float2 f = nb.c;
    RegOut<NC> r;
    warp_pixel<INTERP, NC>(d, H, W, P, ps, i, j, (float)(j + 1) + f.x, (float)(i + 1) + f.y, r);
    assemble_px<NC, M, WT>(o, uv, (const float2 *)nullptr, NC, (const float2 *)nullptr, i, j, H, W, P, ps, coef, rhs,
                           wgt, [&](int ch, float &it, float &gx, float &gy) {
                             it = r.it[ch];
                             gx = r.ix[ch];
                             gy = r.iy[ch];
                           }, &nb);
  }
}
#define OF_WOP(WT, I, N, M)                                                                                   \
  template __global__ void k_warp_operator<WT, I, N, M>(DerivArgs, OpArgs, const float2 *, int, int, int, size_t, \
                                                        float *, float2 *, const float *);
#define OF_FOP_WT(WT, M)                                                                                       \
  template __global__ void k_flow_operator<WT, M>(OpArgs, const float2 *, const float2 *, const float *,        \
                                                  const float *, const float *, int, const float2 *, int, int,  \
                                                  int, size_t, float *, float2 *, const float *);
// specialised penalty modes: the registry's quadratic stage and its robust
// stages (generalized Charbonnier: Classic+NL; Charbonnier: Classic-C;
// Lorentzian: BA; Horn-Schunck's constant weights)
#define OF_PM_LIST(X) X(OF_PM_ANY) X(OF_PM_Q) X(OF_PM_R(OF_PEN_GEN_CHARBONNIER)) X(OF_PM_R(OF_PEN_CHARBONNIER)) \
  X(OF_PM_R(OF_PEN_LORENTZIAN)) X(OF_PM_R(OF_PEN_CONST))
#define OF_WOP_WT(WT, M) \
  OF_WOP(WT, 0, 1, M) OF_WOP(WT, 1, 1, M) OF_WOP(WT, 2, 1, M) OF_WOP(WT, 0, 3, M) OF_WOP(WT, 1, 3, M) OF_WOP(WT, 2, 3, M)
#define OF_WOP_M(M) OF_WOP_WT(false, M) OF_WOP_WT(true, M)
#define OF_FOP(M) OF_FOP_WT(false, M) OF_FOP_WT(true, M)
OF_PM_LIST(OF_WOP_M)
OF_PM_LIST(OF_FOP)
#undef OF_WOP_M
#undef OF_WOP_WT
#undef OF_WOP
#undef OF_FOP
#undef OF_FOP_WT

// The same assembly with every intermediate in fp64 (the reference's own
// precision) and one rounding per stored plane: for AltBA (OpArgs::f64),
// whose robust systems are so ill-conditioned that the ~2e-7 relative error
// of the fp32 assembly's diagonal (a sum of four edge weights, a data term
// and the coupling) moved the solve by 5x the float32 floor of the system
// (tools/altba_gpu_probe.py).  Not on the hot path.
// A kernel of its own, not an assemble_px instance: it has no OF_NOCONTRACT and
// all-fp64 arithmetic, so folding it in would change its rounding or put a
// type parameter through the hot path.
__device__ __forceinline__ double2 edge_w_f64(const OpArgs &o, int axis, double du, double dv) {
  double wu = 0.0, wv = 0.0;
  if (o.use_q) { wu += o.aq_s_d * pen_w_f64(o.qsu[axis], du); wv += o.aq_s_d * pen_w_f64(o.qsv[axis], dv); }
  if (o.use_r) { wu += o.ar_s_d * pen_w_f64(o.rsu[axis], du); wv += o.ar_s_d * pen_w_f64(o.rsv[axis], dv); }
  return make_double2(wu, wv);
}
__device__ __forceinline__ double2 ld_uvd_f64(const float2 *uv, const float2 *duv, size_t k) {
  const float2 a = uv[k];
  double2 r = make_double2(a.x, a.y);
  if (duv) { const float2 b = duv[k]; r.x += b.x; r.y += b.y; }
  return r;
}
__global__ __launch_bounds__(OF_BX *OF_BY) void k_flow_operator_f64(OpArgs o, const float2 *__restrict__ uv,
                                const float2 *__restrict__ duv, const float *__restrict__ It,
                                const float *__restrict__ Ix, const float *__restrict__ Iy, int nc,
                                const float2 *__restrict__ uvhat, int H, int W, int P, size_t ps,
                                float *__restrict__ coef, float2 *__restrict__ rhs) {
  OF_FOR_PIXELS_XCD(H, W) {
    if (j >= W) continue;
    const size_t k = (size_t)i * P + j;
    const double2 c = ld_uvd_f64(uv, duv, k);
    double2 eR = make_double2(0.0, 0.0), eD = eR, eL = eR, eU = eR;
    if (j < W - 1) { double2 n = ld_uvd_f64(uv, duv, k + 1); eR = edge_w_f64(o, 0, n.x - c.x, n.y - c.y); }
    if (i < H - 1) { double2 n = ld_uvd_f64(uv, duv, k + P); eD = edge_w_f64(o, 1, n.x - c.x, n.y - c.y); }
    if (j > 0) { double2 n = ld_uvd_f64(uv, duv, k - 1); eL = edge_w_f64(o, 0, c.x - n.x, c.y - n.y); }
    if (i > 0) { double2 n = ld_uvd_f64(uv, duv, k - P); eU = edge_w_f64(o, 1, c.x - n.x, c.y - n.y); }
    double du = 0.0, dv = 0.0;
    if (duv) { du = duv[k].x; dv = duv[k].y; }
    double psq = 0.0, psr = 0.0, ix2 = 0.0, iy2 = 0.0, ixy = 0.0, itx = 0.0, ity = 0.0;
    for (int ch = 0; ch < nc; ++ch) {
      const size_t kc = ch * ps + k;
      const double gx = Ix[kc], gy = Iy[kc], itl = It[kc] + gx * du + gy * dv;
      if (o.use_q) psq += pen_w_f64(o.qd, itl);
      if (o.use_r) psr += pen_w_f64(o.rd, itl);
      ix2 += gx * gx; iy2 += gy * gy; ixy += gx * gy;
      itx += itl * gx; ity += itl * gy;
    }
    const double inv = 1.0 / (double)nc;
    const double psi = ((o.use_q ? o.aq_d_d * psq : 0.0) + (o.use_r ? o.ar_d_d * psr : 0.0)) * inv;
    ix2 *= inv; iy2 *= inv; ixy *= inv; itx *= inv; ity *= inv;
    const float2 u0f = uv[k];
    const double2 u0 = make_double2(u0f.x, u0f.y);
    double lu = 0.0, lv = 0.0;
    if (j < W - 1) { float2 n = uv[k + 1]; lu += eR.x * (u0.x - n.x); lv += eR.y * (u0.y - n.y); }
    if (i < H - 1) { float2 n = uv[k + P]; lu += eD.x * (u0.x - n.x); lv += eD.y * (u0.y - n.y); }
    if (j > 0) { float2 n = uv[k - 1]; lu += eL.x * (u0.x - n.x); lv += eL.y * (u0.y - n.y); }
    if (i > 0) { float2 n = uv[k - P]; lu += eU.x * (u0.x - n.x); lv += eU.y * (u0.y - n.y); }
    double auu = psi * ix2 + (eL.x + eR.x + eU.x + eD.x);
    double avv = psi * iy2 + (eL.y + eR.y + eU.y + eD.y);
    double bu = -lu - psi * itx, bv = -lv - psi * ity;
    if (uvhat) {  // AltBA coupling (alt_ba.py:236-242)
      const float2 h = uvhat[k];
      const double tu = pen_w_f64(o.rc, u0.x - h.x), tv = pen_w_f64(o.rc, u0.y - h.y);
      auu += o.lambda2_d * tu;
      avv += o.lambda2_d * tv;
      bu += o.lambda2_d * tu * (h.x - u0.x);
      bv += o.lambda2_d * tv * (h.y - u0.y);
    }
    coef[k] = (float)eR.x;
    coef[ps + k] = (float)eD.x;
    coef[2 * ps + k] = (float)eR.y;
    coef[3 * ps + k] = (float)eD.y;
    coef[4 * ps + k] = (float)auu;
    coef[5 * ps + k] = (float)(psi * ixy);
    coef[6 * ps + k] = (float)avv;
    rhs[k] = make_float2((float)bu, (float)bv);
  }
}
