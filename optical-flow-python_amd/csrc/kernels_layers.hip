// kernels_layers.hip — layered motion segmentation of a flow field
// (of_segment_motion): the usable-pixel plane (k_layers_usable), one
// hypothesis per cell of the fit's pass-0 tile records (k_layers_cells),
// consensus scoring of every hypothesis on the pixels not yet removed
// (k_layers_score), the choice of a layer's seed (k_layers_pick), the removal of
// a fitted layer's inliers (k_layers_remove, k_layers_commit), the joint label
// assignment with the per-layer state planes of the refits (k_layers_assign)
// and the label mode filter (k_layers_mode).  The passes between them are the
// fit's own kernels (kernels_motion.hip, included before this file), unchanged,
// and what these kernels do as the fit does it, they do with the fit's own
// pieces: its tile mapping (MOT_TILE), usable-sample test (mot_usable), state
// reset (mot_reset) and closed-form solve (mot_solve).
// Same conventions as there: pitched float2 flows, dense H x W planes, fp64
// from the fp32 inputs with no contraction in the order include/optflow.h
// states ("Layered motion segmentation"); every floating-point sum in the
// fit's fixed order.  Counts are integers (ballot and popcount per wave, LDS
// per block, one integer atomic per block and counter), so their order of
// arrival does not matter.  H * W < 2^31 (checked on the host).
#include "kernels.h"

#define LAY_MAXH 256  // hypotheses: at most 16 x 16 cells
#define LAY_MAXK 8    // layers

// a cell's hypothesis; flag 0: none, 1: one, 3: one whose solve lost rank
struct LayerHyp {
  double th[6];
  int32_t flag;
  int32_t pad_;
};

// what a segmentation keeps on the device between its launches
struct LayerCtl {
  int32_t total;             // usable pixels
  int32_t n;                 // layers extracted so far
  int32_t done;              // the extraction has stopped
  int32_t inl;               // inliers of the layer being extracted
  int32_t lost[LAY_MAXK];    // the seed hypothesis of layer l had lost rank
  int32_t pixels[LAY_MAXK];  // of every label in the filtered plane
  int32_t count[LAY_MAXH];   // consensus of every hypothesis
};

// the plane every later step reads: 0 usable and not removed, 1 not usable,
// 2 + l removed by layer l
#define LAY_REM 0
#define LAY_UNUSABLE 1

__device__ __forceinline__ double lay_r2(const double *th, double x, double y, double u, double v) {
  OF_NOCONTRACT
  const double uh = th[0] + th[1] * x + th[2] * y, vh = th[3] + th[4] * x + th[5] * y;
  const double ru = u - uh, rv = v - vh;
  return ru * ru + rv * rv;
}

// the lanes of a wave for which p holds
__device__ __forceinline__ int lay_votes(bool p) { return __popcll(__ballot(p)); }

// state plane and count of the usable pixels: w0 > 0, with w0 the fit's
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_layers_usable(const float2 *__restrict__ uv, int H, int W, int P, const float *__restrict__ wgt,
                const uint8_t *__restrict__ st, int ntx, int nt, uint8_t *__restrict__ cst, LayerCtl *ctl) {
  __shared__ int scnt;
  if (threadIdx.x == 0) scnt = 0;
  __syncthreads();
  MOT_TILE(ntx);
  if (tile < nt) {
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < MOT_TH; ++r) {
      const int i = i0 + r;
      bool use = false;
      if (j < W && i < H) {
        const size_t o = (size_t)i * W + j;
        const float2 g = uv[(size_t)i * P + j];
        const bool ok = mot_usable(g, st ? st[o] : (uint8_t)0);
        use = ok && (wgt ? wgt[o] : 1.0f) > 0.0f;
        cst[o] = use ? LAY_REM : LAY_UNUSABLE;
      }
      cnt += lay_votes(use);
    }
    if (lane == 0 && cnt) atomicAdd(&scnt, cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0 && scnt) atomicAdd(&ctl->total, scnt);
}

// The n values v[(r0 + t / cwid) * ntx + q0 + t % cwid], t = 0 .. n - 1, through
// the group tree in one wave: 64 at a time through the halving tree, the
// results collected 64 at a time for the next level, four levels (n <= 2^24).
// A level that holds one value adds +0.0 to it, which changes no bit (a tile
// value is never -0.0).  The sum is in lane 0.
__device__ __forceinline__ double lay_cell_sum(const double *__restrict__ v, int ntx, int r0, int q0, int cwid, int n,
                                               int lane) {
  double b2 = 0.0, b3 = 0.0, b4 = 0.0;
  const int G1 = (n + 63) / 64;
  for (int g1 = 0; g1 < G1; ++g1) {
    const int t = g1 * 64 + lane;
    double x = 0.0;
    if (t < n) {
      const int rr = t / cwid;
      x = v[(size_t)(r0 + rr) * ntx + q0 + (t - rr * cwid)];
    }
    const double s1 = __shfl(mot_tree(x), 0, 64);
    if (lane == (g1 & 63)) b2 = s1;
    const bool last = g1 == G1 - 1;
    if ((g1 & 63) == 63 || last) {
      const int g2 = g1 >> 6;
      const double s2 = __shfl(mot_tree(b2), 0, 64);
      b2 = 0.0;
      if (lane == (g2 & 63)) b3 = s2;
      if ((g2 & 63) == 63 || last) {
        const double s3 = __shfl(mot_tree(b3), 0, 64);
        b3 = 0.0;
        if (lane == ((g2 >> 6) & 63)) b4 = s3;
      }
    }
  }
  return mot_tree(b4);
}

// One wave per cell (a, b) of the g x g grid over the nty x ntx tile records
// of pass 0 (rec[k * stride + tile]): the cell's tiles in row-major order
// through the group tree, then the solve in lane 0.
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_layers_cells(const double *__restrict__ rec, int stride, int nty, int ntx, int g, int model,
               LayerHyp *__restrict__ hyp) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * MOT_WAVES + (threadIdx.x >> 6);
  if (cell >= g * g) return;  // the whole wave
  const int a = cell / g, b = cell - a * g;
  const int ch = (nty + g - 1) / g, cw = (ntx + g - 1) / g;
  const int r0 = a * ch, r1 = min(r0 + ch, nty), q0 = b * cw, q1 = min(q0 + cw, ntx);
  double S[MOT_NS], th[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int flag = 0;
  if (r0 < r1 && q0 < q1) {  // the cell exists
    const int cwid = q1 - q0;
    for (int k = 0; k < MOT_NS; ++k)
      S[k] = lay_cell_sum(rec + (size_t)k * stride, ntx, r0, q0, cwid, (r1 - r0) * cwid, lane);
    if (lane == 0 && S[0] > 0.0) flag = mot_solve(S, model, th) ? 3 : 1;
  }
  if (lane != 0) return;
  for (int k = 0; k < 6; ++k) hyp[cell].th[k] = th[k];
  hyp[cell].flag = flag;
  hyp[cell].pad_ = 0;
}

// count[h] += #{p not removed : r2_h(p) < c2} for every hypothesis h.  One wave
// per tile, a lane's eight rows of (u, v, not removed) and y in registers across
// the hypothesis loop; the hypotheses in LDS, read at a wave-uniform address.
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_layers_score(const float2 *__restrict__ uv, int H, int W, int P, const uint8_t *__restrict__ cst,
               const LayerHyp *__restrict__ hyp, int nh, double c2, MotionFrame fr, int ntx, int nt, LayerCtl *ctl) {
  OF_NOCONTRACT
  __shared__ double sth[LAY_MAXH * 6];
  __shared__ int sflag[LAY_MAXH];
  __shared__ int scnt[LAY_MAXH];
  if (ctl->done) return;  // the whole grid
  for (int h = threadIdx.x; h < nh; h += MOT_WAVES * 64) {
    sflag[h] = hyp[h].flag;
    scnt[h] = 0;
    for (int k = 0; k < 6; ++k) sth[h * 6 + k] = hyp[h].th[k];
  }
  __syncthreads();
  MOT_TILE(ntx);
  if (tile < nt) {
    double u[MOT_TH], v[MOT_TH], y[MOT_TH];
    unsigned rem = 0;
#pragma unroll
    for (int r = 0; r < MOT_TH; ++r) {
      const int i = i0 + r;
      const bool in = j < W && i < H && cst[(size_t)i * W + j] == LAY_REM;
      const float2 g = in ? uv[(size_t)i * P + j] : make_float2(0.0f, 0.0f);
      u[r] = (double)g.x;
      v[r] = (double)g.y;
      y[r] = ((double)i - fr.cy) / fr.s;
      rem |= (in ? 1u : 0u) << r;
    }
    const double x = ((double)j - fr.cx) / fr.s;
    for (int h = 0; h < nh; ++h) {
      if (!sflag[h]) continue;
      const double *th = sth + h * 6;
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < MOT_TH; ++r) cnt += lay_votes(((rem >> r) & 1u) && lay_r2(th, x, y[r], u[r], v[r]) < c2);
      if (lane == 0 && cnt) atomicAdd(&scnt[h], cnt);
    }
  }
  __syncthreads();
  for (int h = threadIdx.x; h < nh; h += MOT_WAVES * 64)
    if (scnt[h]) atomicAdd(&ctl->count[h], scnt[h]);
}

// One wave: the hypothesis with the largest count, the lowest index on a tie,
// becomes the start of layer l's passes in ms (c2 fixed), unless the
// extraction has stopped or stops here for lack of support; then ms is left
// stopped, so the passes queued behind do nothing.  Clears the counts.
__global__ void __launch_bounds__(64)
k_layers_pick(const LayerHyp *__restrict__ hyp, int nh, int l, double min_support, double c2,
              MotionState *__restrict__ ms, LayerCtl *ctl) {
  const int lane = threadIdx.x;
  int bc = -1, bh = -1;
  for (int h = lane; h < nh; h += 64) {
    const int cnt = ctl->count[h];
    if (hyp[h].flag && cnt > bc) {
      bc = cnt;
      bh = h;
    }
    ctl->count[h] = 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int oc = __shfl_down(bc, d, 64), oh = __shfl_down(bh, d, 64);
    if (oc > bc || (oc == bc && oc >= 0 && oh < bh)) {
      bc = oc;
      bh = oh;
    }
  }
  if (lane != 0) return;
  mot_reset(ms, c2, 1);
  if (ctl->done) return;
  if (bh < 0 || (double)bc < min_support * (double)ctl->total) {
    ctl->done = 1;
    return;
  }
  for (int k = 0; k < 6; ++k) ms->th[k] = hyp[bh].th[k];
  ms->stop = 0;
  ctl->lost[l] = hyp[bh].flag >> 1;
}

// the pixels not yet removed that layer l's fit explains (r2 < c2) are marked
// as removed by it and counted
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_layers_remove(const float2 *__restrict__ uv, int H, int W, int P, uint8_t *__restrict__ cst,
                const MotionState *__restrict__ ms, int l, double c2, MotionFrame fr, int ntx, int nt, LayerCtl *ctl) {
  OF_NOCONTRACT
  __shared__ int scnt;
  if (ctl->done) return;  // the whole grid
  if (threadIdx.x == 0) scnt = 0;
  __syncthreads();
  MOT_TILE(ntx);
  if (tile < nt) {
    double th[6];
    for (int k = 0; k < 6; ++k) th[k] = ms->th[k];
    const double x = ((double)j - fr.cx) / fr.s;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < MOT_TH; ++r) {
      const int i = i0 + r;
      bool inl = false;
      if (j < W && i < H && cst[(size_t)i * W + j] == LAY_REM) {
        const float2 g = uv[(size_t)i * P + j];
        const double y = ((double)i - fr.cy) / fr.s;
        inl = lay_r2(th, x, y, (double)g.x, (double)g.y) < c2;
        if (inl) cst[(size_t)i * W + j] = (uint8_t)(2 + l);
      }
      cnt += lay_votes(inl);
    }
    if (lane == 0 && cnt) atomicAdd(&scnt, cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0 && scnt) atomicAdd(&ctl->inl, scnt);
}

// layer l stays when its inliers reach the support; otherwise it is discarded
// and the extraction stops
__global__ void k_layers_commit(int l, double min_support, LayerCtl *ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!ctl->done) {
    if ((double)ctl->inl < min_support * (double)ctl->total) ctl->done = 1;
    else ctl->n = l + 1;
  }
  ctl->inl = 0;
}

// raw(i, j) = the layer of lay[0 .. n) with the smallest r2 below c2, the
// lowest index on a tie, else OF_LAYER_NONE (also where the flow is not
// finite); state plane l, mask + l * H * W, is 0 where a usable pixel carries
// label l and 1 elsewhere: the `state` of layer l's refit.  Rearms the layers'
// fits (a refit without support stops only itself).
__global__ void __launch_bounds__(MOT_WAVES * 64)
k_layers_assign(const float2 *__restrict__ uv, int H, int W, int P, const uint8_t *__restrict__ cst,
                MotionState *__restrict__ lay, int n, double c2, MotionFrame fr, int ntx, int nt,
                uint8_t *__restrict__ raw, uint8_t *__restrict__ mask) {
  OF_NOCONTRACT
  __shared__ double sth[LAY_MAXK * 6];
  if ((int)threadIdx.x < n * 6) sth[threadIdx.x] = lay[threadIdx.x / 6].th[threadIdx.x % 6];
  if (blockIdx.x == 0 && (int)threadIdx.x < n) lay[threadIdx.x].stop = 0;
  __syncthreads();
  MOT_TILE(ntx);
  if (tile >= nt || j >= W) return;
  const size_t ps = (size_t)H * W;
  const double x = ((double)j - fr.cx) / fr.s;
#pragma unroll
  for (int r = 0; r < MOT_TH; ++r) {
    const int i = i0 + r;
    if (i >= H) break;
    const size_t o = (size_t)i * W + j;
    const float2 g = uv[(size_t)i * P + j];
    const bool fin = __builtin_isfinite(g.x) && __builtin_isfinite(g.y);
    const double u = fin ? (double)g.x : 0.0, v = fin ? (double)g.y : 0.0;
    const double y = ((double)i - fr.cy) / fr.s;
    double best = c2;
    int lab = OF_LAYER_NONE;
    for (int l = 0; l < n; ++l) {
      const double r2 = lay_r2(sth + l * 6, x, y, u, v);
      if (fin && r2 < best) {
        best = r2;
        lab = l;
      }
    }
    raw[o] = (uint8_t)lab;
    const bool use = cst[o] != LAY_UNUSABLE;
    for (int l = 0; l < n; ++l) mask[(size_t)l * ps + o] = use && lab == l ? 0 : 1;
  }
}

// out(i, j) = the value among 0 .. n - 1 and OF_LAYER_NONE that occurs most
// often in the in-frame part of the (2r + 1)^2 window of raw, the smallest on
// a tie; pixels[l] += the pixels that end with label l.  A block filters 8 rows
// x 32 columns (block b: tile row b / nbx, tile column b % nbx) from a copy
// with its halo in LDS; r <= LAY_MAXR.
#define LAY_MAXR 3
#define LAY_FW 32
#define LAY_FH 8
#define LAY_OUTSIDE 254
__global__ void __launch_bounds__(LAY_FW *LAY_FH)
k_layers_mode(const uint8_t *__restrict__ raw, int H, int W, int n, int r, int nbx, uint8_t *__restrict__ out,
              LayerCtl *ctl) {
  __shared__ uint8_t t[(LAY_FH + 2 * LAY_MAXR) * (LAY_FW + 2 * LAY_MAXR)];
  __shared__ int spx[LAY_MAXK];
  const int tid = threadIdx.x, li = tid / LAY_FW, lj = tid - li * LAY_FW;
  const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
  const int tw = LAY_FW + 2 * r, th = LAY_FH + 2 * r;
  if (tid < LAY_MAXK) spx[tid] = 0;
  for (int k = tid; k < tw * th; k += LAY_FW * LAY_FH) {
    const int ki = k / tw;
    const int ii = by * LAY_FH - r + ki, jj = bx * LAY_FW - r + (k - ki * tw);
    t[k] = ii >= 0 && ii < H && jj >= 0 && jj < W ? raw[(size_t)ii * W + jj] : (uint8_t)LAY_OUTSIDE;
  }
  __syncthreads();
  const int i = by * LAY_FH + li, j = bx * LAY_FW + lj;
  int lab = LAY_OUTSIDE;
  if (i < H && j < W) {
    unsigned long long cnt = 0;  // a byte per layer: a window holds at most 49
    int none = 0;
    for (int di = 0; di <= 2 * r; ++di)
      for (int dj = 0; dj <= 2 * r; ++dj) {
        const int v = t[(li + di) * tw + lj + dj];
        if (v < LAY_MAXK) cnt += 1ull << (8 * v);
        else if (v == OF_LAYER_NONE) ++none;
      }
    int best = -1;
    for (int l = 0; l < n; ++l) {
      const int cl = (int)((cnt >> (8 * l)) & 255ull);
      if (cl > best) {
        best = cl;
        lab = l;
      }
    }
    if (none > best) lab = OF_LAYER_NONE;
    out[(size_t)i * W + j] = (uint8_t)lab;
  }
  for (int l = 0; l < n; ++l) {
    const int c = lay_votes(lab == l);
    if ((tid & 63) == 0 && c) atomicAdd(&spx[l], c);
  }
  __syncthreads();
  if (tid < n && spx[tid]) atomicAdd(&ctl->pixels[tid], spx[tid]);
}
