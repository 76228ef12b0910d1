// host_image.hip — host side of the image kernels (kernels_img.hip) and of
// the flow-field helpers: arena images and fields, uploads and downloads,
// correlation taps, pyramids, the ROF texture split, the per-level derivative
// planes and warps, the median filters and the flow resampling.
namespace {

Img new_img(of_ctx *c, int H, int W, int C) {
  Img m;
  m.H = H;
  m.W = W;
  m.C = C;
  m.P = of_pitch(W);
  m.p = (float *)c->arena.alloc(sizeof(float) * m.ps() * (C > 0 ? C : 1));
  return m;
}
F2 new_f2(of_ctx *c, int H, int W) {
  F2 f;
  f.H = H;
  f.W = W;
  f.P = of_pitch(W);
  f.p = (float2 *)c->arena.alloc(sizeof(float2) * (size_t)H * f.P);
  return f;
}
Img view(const Img &m, int c0, int n) {
  Img v = m;
  v.p = m.plane(c0);
  v.C = n;
  return v;
}

// host planar dense (C x H x W) -> device pitched
void upload_img(of_ctx *c, const Img &m, const float *host) {
  HIPCHK(hipMemcpy2DAsync(m.p, sizeof(float) * m.P, host, sizeof(float) * m.W, sizeof(float) * m.W,
                          (size_t)m.H * m.C, hipMemcpyHostToDevice, c->stream));
}
void download_img(of_ctx *c, const Img &m, float *host) {
  HIPCHK(hipMemcpy2DAsync(host, sizeof(float) * m.W, m.p, sizeof(float) * m.P, sizeof(float) * m.W,
                          (size_t)m.H * m.C, hipMemcpyDeviceToHost, c->stream));
}
Img upload_new_img(of_ctx *c, const float *host, int H, int W, int C) {
  Img m = new_img(c, H, W, C);
  upload_img(c, m, host);
  return m;
}
void copy_img(of_ctx *c, const Img &dst, const Img &src) {
  HIPCHK(hipMemcpyAsync(dst.p, src.p, sizeof(float) * src.ps() * src.C, hipMemcpyDeviceToDevice, c->stream));
}
// ---- dense data: n values, no pitch ----
// an arena buffer where `want` says so (an optional output's device side), else nullptr
template <typename T>
T *new_dense(of_ctx *c, size_t n, bool want = true) {
  return want ? (T *)c->arena.alloc(sizeof(T) * n) : nullptr;
}
// the host data's arena copy, on the context's stream; nullptr for nullptr
template <typename T>
T *upload_dense(of_ctx *c, const T *host, size_t n) {
  T *d = new_dense<T>(c, n, host != nullptr);
  if (host) HIPCHK(hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
  return d;
}
// device -> host where the caller gave a host buffer
template <typename T, typename D>
void download_dense(of_ctx *c, T *host, const D *dev, size_t n) {
  static_assert(std::is_same<T, D>::value, "host and device buffers of one type");
  if (host) HIPCHK(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
}
// planar host/dense-device uv <-> pitched float2
void f2_from_dense(of_ctx *c, const F2 &f, const float *dense_dev) {
  Grid2 g = grid2(f.H, f.W);
  launch(c, "planar2_to_f2", k_planar2_to_f2, g.grid, g.block, 0, dense_dev, f.p, f.H, f.W, f.P,
         (size_t)f.H * f.W);
}
void f2_to_dense(of_ctx *c, const F2 &f, float *dense_dev) {
  Grid2 g = grid2(f.H, f.W);
  launch(c, "f2_to_planar2", k_f2_to_planar2, g.grid, g.block, 0, (const float2 *)f.p, dense_dev, f.H, f.W, f.P,
         (size_t)f.H * f.W);
}
F2 upload_f2(of_ctx *c, const float *host, int H, int W) {
  F2 f = new_f2(c, H, W);
  f2_from_dense(c, f, upload_dense(c, host, 2 * (size_t)H * W));
  return f;
}
void download_f2(of_ctx *c, const F2 &f, float *host) {
  float *d = new_dense<float>(c, 2 * (size_t)f.H * f.W);
  f2_to_dense(c, f, d);
  download_dense(c, host, d, 2 * (size_t)f.H * f.W);
}
void fill_f2(of_ctx *c, const F2 &f, float v) {
  Grid2 g = grid2(f.H, f.W);
  launch(c, "fill_f2", k_fill_f2, g.grid, g.block, 0, f.p, f.H, f.W, f.P, make_float2(v, v));
}
// a solve's starting flow: the caller's, or zero
F2 init_flow(of_ctx *c, const float *init_uv, int H, int W) {
  if (init_uv) return upload_f2(c, init_uv, H, W);
  F2 f = new_f2(c, H, W);
  fill_f2(c, f, 0.0f);
  return f;
}
// two dense host frames of n floats each -> the arena
void upload_frames(of_ctx *c, const float *im1, const float *im2, size_t n, float **d1, float **d2) {
  *d1 = upload_dense(c, im1, n);
  *d2 = upload_dense(c, im2, n);
}

// ---- global scale_image over all planes of an image ------------------------
void scale_img(of_ctx *c, const Img &m, float vlow, float vhigh, int mm_slot) {
  uint32_t *mm = c->d_mm + 2 * mm_slot;
  launch(c, "mm_init", k_mm_init, dim3(1), dim3(64), 0, mm, 1);
  Grid2 gm = grid2(m.H, m.W, 256), g = grid2(m.H, m.W);
  launch(c, "minmax", k_minmax, gm.grid, gm.block, 0, (const float *)m.p, m.H, m.W, m.P, m.C, m.ps(), mm);
  launch(c, "scale", k_scale, g.grid, g.block, 0, m.p, m.H, m.W, m.P, m.C, m.ps(), (const uint32_t *)mm, vlow, vhigh);
}

// estimate_flow preprocessing (interface.py:41-64, 91-141): the gray planes of
// two (H, W, C) frames and, with a guide (p != nullptr), the first frame's Lab
// (C == 3) or gray guide, the /255 decision from that frame's own maximum
template <typename T>
void rgb_prep(of_ctx *c, const T *rgb1, const T *rgb2, int H, int W, int C, const Img &gray, const Img &guide) {
  uint32_t *mm = c->d_mm + 2 * 8;
  launch(c, "mm_init", k_mm_init, dim3(1), dim3(64), 0, mm, 1);
  const long n = (long)H * W * 3;
  if (C == 3)
    launch(c, "rgb_max", k_rgb_max<T>, dim3((unsigned)std::min<long>((n + 255) / 256, 256)), dim3(256), 0, rgb1, n, mm);
  Grid2 g = grid2(H, W);
  launch(c, "rgb_prep", k_rgb_prep<T>, g.grid, g.block, 0, rgb1, rgb2, H, W, C, gray.p, gray.P, gray.ps(), guide.p,
         (const uint32_t *)mm);
  if (guide.p && C == 3)
    for (int ch = 0; ch < 3; ++ch) scale_img(c, view(guide, ch, 1), 0.0f, 255.0f, 9 + ch);
}

// ---- correlation taps -------------------------------------------------------
Taps make_taps(const double *k, int kh, int kw) {
  Taps t;
  memset(&t, 0, sizeof(t));
  t.kh = kh;
  t.kw = kw;
  for (int a = 0; a < kh * kw; ++a) t.w[a] = (float)k[a];
  return t;
}
void correlate(of_ctx *c, const Img &in, const Img &out, const Taps &t) {
  Grid2 g = grid2(in.H, in.W);
  const bool fold1 = in.H > t.kh / 2 && in.W > t.kw / 2;  // one reflection reaches every tap
  auto go = [&](auto k) {
    launch(c, "correlate", k, gz(g, in.C), g.block, 0, (const float *)in.p, out.p, in.H, in.W, in.P, in.ps(), t);
  };
  if (fold1 && t.kh == 5 && t.kw == 5) go(k_correlate_k<5, 5>);
  else if (fold1 && t.kh == 1 && t.kw == 5) go(k_correlate_k<1, 5>);
  else if (fold1 && t.kh == 5 && t.kw == 1) go(k_correlate_k<5, 1>);
  else if (fold1 && t.kh == 3 && t.kw == 3) go(k_correlate_k<3, 3>);
  else if (fold1 && t.kh == 1 && t.kw == 3) go(k_correlate_k<1, 3>);
  else if (fold1 && t.kh == 3 && t.kw == 1) go(k_correlate_k<3, 1>);
  else go(k_correlate);
}

// fspecial('gaussian') (image_processing.py:29-49)
std::vector<double> gaussian(int size, double sigma) {
  std::vector<double> k(size * size);
  double m = (size - 1) / 2.0, mx = 0, s = 0;
  for (int a = 0; a < size; ++a)
    for (int b = 0; b < size; ++b) {
      double y = a - m, x = b - m;
      k[a * size + b] = std::exp(-(x * x + y * y) / (2 * sigma * sigma));
      mx = std::max(mx, k[a * size + b]);
    }
  for (auto &v : k) {
    if (v < 2.220446049250313e-16 * mx) v = 0;
    s += v;
  }
  if (s != 0)
    for (auto &v : k) v /= s;
  return k;
}

void resize_dims(int H, int W, double ratio, int *nH, int *nW) {
  int a = (int)std::floor(H * ratio + 0.5), b = (int)std::floor(W * ratio + 0.5);
  *nH = a < 1 ? 1 : a;
  *nW = b < 1 ? 1 : b;
}

// one compute_image_pyramid step (pyramid.py:58-67)
// a separable kh x kw kernel ky (x) kx as a row pass then a column pass
// (10 taps per pixel instead of 25 for 5 x 5; same sums, another rounding order)
void correlate_sep(of_ctx *c, const Img &in, const Img &out, const Taps &tx, const Taps &ty) {
  Img tmp = new_img(c, in.H, in.W, in.C);
  correlate(c, in, tmp, tx);
  correlate(c, tmp, out, ty);
}

// k_resize takes its source coordinates in 32-bit integers (resize_src)
void resize_fits(int H, int W, int nH, int nW) {
  REQUIRE(2LL * H * nH < (1LL << 31) && 2LL * W * nW < (1LL << 31), OF_ENOTSUP, "resize of a plane this large");
}

// the smoothed level `sm` resized by `ratio`
Img resize_img(of_ctx *c, const Img &sm, double ratio) {
  int nH, nW;
  resize_dims(sm.H, sm.W, ratio, &nH, &nW);
  resize_fits(sm.H, sm.W, nH, nW);
  Img out = new_img(c, nH, nW, sm.C);
  Grid2 g = grid2(nH, nW);
  launch(c, "resize", k_resize<float>, gz(g, sm.C), g.block, 0, (const float *)sm.p, sm.H, sm.W, sm.P, sm.ps(),
         out.p, nH, nW, out.P, out.ps(), 1.0f);
  return out;
}
Img pyramid_step(of_ctx *c, const Img &in, const Taps &tx, const Taps &ty, double ratio) {
  Img tmp = new_img(c, in.H, in.W, in.C);
  correlate_sep(c, in, tmp, tx, ty);
  return resize_img(c, tmp, ratio);
}
Img pyramid_step(of_ctx *c, const Img &in, const Taps &t, double ratio) {
  Img tmp = new_img(c, in.H, in.W, in.C);
  correlate(c, in, tmp, t);
  return resize_img(c, tmp, ratio);
}

// _build_pyramid (base.py:174-190)
std::vector<Img> build_pyramid(of_ctx *c, const Img &img, int levels, double spacing) {
  double sig = std::sqrt(spacing) / std::sqrt(2.0);
  int ks = 2 * (int)std::nearbyint(1.5 * sig) + 1;
  // fspecial('gaussian') is the outer product of the normalised 1-D
  // Gaussian (its eps cut-off removes nothing at these sizes: the smallest
  // entry is >= 1.8 % of the largest)
  std::vector<double> g1(ks);
  double s1 = 0.0;
  for (int b = 0; b < ks; ++b) s1 += (g1[b] = std::exp(-(b - (ks - 1) / 2.0) * (b - (ks - 1) / 2.0) / (2 * sig * sig)));
  for (auto &v : g1) v /= s1;
  const Taps tx = make_taps(g1.data(), 1, ks), ty = make_taps(g1.data(), ks, 1);
  std::vector<Img> pyr{img};
  for (int l = 1; l < levels; ++l) pyr.push_back(pyramid_step(c, pyr.back(), tx, ty, 1.0 / spacing));
  return pyr;
}

// structure_texture_decomposition_rof (image_processing.py:52-136) on all planes
Img rof_texture(of_ctx *c, const Img &in, double theta, int iters, double alp) {
  c->cur_px = (double)in.H * in.W * in.C;
  Img nrm = new_img(c, in.H, in.W, in.C);
  copy_img(c, nrm, in);
  scale_img(c, nrm, -1.0f, 1.0f, 0);
  const size_t ps = nrm.ps();  // C planes of float2 p
  float2 *p0 = (float2 *)c->arena.alloc(sizeof(float2) * ps * in.C);
  float2 *p1 = (float2 *)c->arena.alloc(sizeof(float2) * ps * in.C);
  HIPCHK(hipMemsetAsync(p0, 0, sizeof(float2) * ps * in.C, c->stream));
  Grid2 g = grid2(in.H, in.W);
  const float th = (float)theta, delta = (float)(1.0 / (4.0 * theta));
  const dim3 rg((in.W + ROF_TW - 1) / ROF_TW, (in.H + ROF_TH - 1) / ROF_TH, in.C);  // 64 x 4 blocks
  for (int it = 0; it < iters; it += ROF_K) {
    launch(c, "rof_iters", k_rof_iters, rg, g.block, 0, (const float *)nrm.p, (const float2 *)p0, p1, in.H, in.W,
           nrm.P, ps, th, delta, std::min(ROF_K, iters - it));
    std::swap(p0, p1);
  }
  Img out = new_img(c, in.H, in.W, in.C);
  launch(c, "rof_final", k_rof_final, gz(g, in.C), g.block, 0, (const float *)nrm.p, (const float2 *)p0, out.p, in.H,
         in.W, nrm.P, ps, th, (float)alp);
  scale_img(c, out, 0.0f, 255.0f, 1);
  return out;
}

// ---- per-level derivative planes ---------------------------------------------
struct LevelDeriv {
  Img I1x, I1y, A, B, Cc;
  DerivArgs args;
};

LevelDeriv level_deriv(of_ctx *c, const Img &im, int nc, int interp, const double *filt, double blend) {
  LevelDeriv L;
  Img I1 = view(im, 0, nc), I2 = view(im, nc, nc);
  Taps tx = make_taps(filt, 1, 5), ty = make_taps(filt, 5, 1);
  L.I1x = new_img(c, im.H, im.W, nc);
  L.I1y = new_img(c, im.H, im.W, nc);
  correlate(c, I1, L.I1x, tx);
  correlate(c, I1, L.I1y, ty);
  L.A = new_img(c, im.H, im.W, nc);
  L.B = new_img(c, im.H, im.W, nc);
  L.Cc = new_img(c, im.H, im.W, nc);
  correlate(c, I2, L.A, tx);
  correlate(c, I2, L.B, ty);
  if (interp == OF_INTERP_BICUBIC) {
    // DXY = correlate(I2, filt^T filt) (derivatives.py:27-145), separably:
    // the row pass is A itself
    correlate(c, L.A, L.Cc, ty);
  } else if (interp == OF_INTERP_CUBIC) {
    // B-spline coefficients of I2x, I2y (in place via tmp) and of I2 (into Cc)
    BsplTaps bt;
    const double z = std::sqrt(3.0) - 2.0, c0 = -6.0 * z / (1.0 - z * z);
    for (int k = 0; k <= OF_BSPL_K; ++k) bt.h[k] = (float)(c0 * std::pow(z, (double)k));
    Img tmp = new_img(c, im.H, im.W, nc);
    Grid2 g = grid2(im.H, im.W);
    auto pf = [&](const Img &src, const Img &dst) {
      launch(c, "bspline_rows", k_bspline_rows, gz(g, nc), g.block, 0, (const float *)src.p, tmp.p, im.H, im.W, im.P,
             im.ps(), bt);
      launch(c, "bspline_cols", k_bspline_cols, gz(g, nc), g.block, 0, (const float *)tmp.p, dst.p, im.H, im.W, im.P,
             im.ps(), bt);
    };
    pf(L.A, L.A);
    pf(L.B, L.B);
    pf(I2, L.Cc);
  }
  DerivArgs &d = L.args;
  d.I1 = I1.p;
  d.I2 = I2.p;
  d.I1x = L.I1x.p;
  d.I1y = L.I1y.p;
  d.A = L.A.p;
  d.B = L.B.p;
  d.Cc = L.Cc.p;
  d.nc = nc;
  d.blend = (float)blend;
  return L;
}

void partial_deriv(of_ctx *c, const LevelDeriv &L, int interp, const F2 &uv, const Img &It, const Img &Ix,
                   const Img &Iy) {
  Grid2 g = grid2(uv.H, uv.W);
  const size_t ps = It.ps();
  auto go = [&](const char *name, auto k) {
    launch(c, name, k, g.grid, g.block, 0, L.args, (const float2 *)uv.p, uv.H, uv.W, uv.P, ps, It.p, Ix.p, Iy.p);
  };
  if (interp == OF_INTERP_BICUBIC) go("partial_deriv_hermite", k_partial_deriv<1>);
  else if (interp == OF_INTERP_CUBIC) go("partial_deriv_bspline", k_partial_deriv<0>);
  else go("partial_deriv_bilinear", k_partial_deriv<2>);
}

// ---- filters and resampling of a flow field -----------------------------------
void median2(of_ctx *c, const F2 &in, const F2 &out, int size) {
  Grid2 g = grid2(in.H, in.W);
  auto go = [&](const char *name, auto k) {
    launch(c, name, k, g.grid, g.block, 0, (const float2 *)in.p, out.p, in.H, in.W, in.P);
  };
  if (size == 5) go("median5", k_median2<5>);
  else if (size == 3) go("median3", k_median2<3>);
  else if (size == 7) go("median7", k_median2<7>);
  else throw OfError{OF_ENOTSUP, "median_filter_size must be 3, 5 or 7"};
}

// out = weighted median of uv; with base: out = base + (median - base)
// (classic_nl.py:271-275's uv0 + (filtered - uv0), fused; out may be base)
void wmf(of_ctx *c, const F2 &uv, const Img &guide, const float *occ, const F2 &out, int hsz, double sigma_i,
         const float2 *base = nullptr) {
  REQUIRE(guide.C == 1 || guide.C == 3, OF_ENOTSUP, "weighted median guide must have 1 or 3 channels");
  REQUIRE(hsz >= 0 && hsz <= 12, OF_ENOTSUP, "area_hsz must be <= 12");
  const int RW = WMF_T + 2 * hsz, nreg = RW * RW;
  const int RP = RW + ((8 - RW) % 16 + 16) % 16;  // record row pitch, RP % 16 == 8 (conflict-free window reads)
  int npow2 = 64;
  while (npow2 < nreg) npow2 <<= 1;
  const int nper = npow2 / 64;  // sort keys per lane: 1..16
  const size_t shm = 2 * (size_t)WMF_NC * 64 * sizeof(double) + (size_t)RW * RP * (guide.C == 3 ? 16 : 8) +
                     2 * (size_t)npow2 * sizeof(uint16_t) + 2 * (size_t)RW * RP;
  dim3 grid((uv.W + WMF_T - 1) / WMF_T, (uv.H + WMF_T - 1) / WMF_T);
  const float nk = (float)(-1.4426950408889634 / (2.0 * sigma_i * sigma_i));  // -log2(e) / (2 sigma^2)
  const dim3 block(64);
  auto pick = [&](auto k1, auto k2, auto k4, auto k8, auto k8h7, auto k16) {
    auto k = nper == 1 ? k1 : nper == 2 ? k2 : nper == 4 ? k4 : nper == 8 ? (hsz == 7 ? k8h7 : k8) : k16;
    launch(c, "wmf", k, grid, block, shm, (const float2 *)uv.p, (const float *)guide.p, occ, out.p, uv.H, uv.W,
           uv.P, guide.ps(), hsz, nk, RW, RP, base);
  };
  if (guide.C == 3)
    pick(k_wmf<3, 1, 0>, k_wmf<3, 2, 0>, k_wmf<3, 4, 0>, k_wmf<3, 8, 0>, k_wmf<3, 8, 7>, k_wmf<3, 16, 0>);
  else
    pick(k_wmf<1, 1, 0>, k_wmf<1, 2, 0>, k_wmf<1, 4, 0>, k_wmf<1, 8, 0>, k_wmf<1, 8, 7>, k_wmf<1, 16, 0>);
}

void resample_f2(of_ctx *c, const F2 &in, const F2 &out) {
  const float ratio = (float)((double)out.H / (double)in.H);
  resize_fits(in.H, in.W, out.H, out.W);
  Grid2 g = grid2(out.H, out.W);
  launch(c, "resample_flow", k_resize<float2>, g.grid, g.block, 0, (const float2 *)in.p, in.H, in.W, in.P,
         (size_t)in.H * in.P, out.p, out.H, out.W, out.P, (size_t)out.H * out.P, ratio);
}

}  // namespace
