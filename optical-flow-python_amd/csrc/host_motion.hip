// host_motion.hip — host side of the global motion estimation
// (kernels_motion.hip): option checks, the robust parametric fit as one chain
// of launches on a device-resident flow, the affine warp, the path smoothing
// (host arithmetic on 2 x 3 matrices), the two stage entries on host buffers
// and the per-context stabiliser session.
namespace {

void check_motion_opts(const of_motion_opts *o) {
  REQUIRE(o, OF_EINVAL, "no motion options");
  REQUIRE(o->model >= OF_MOTION_TRANSLATION && o->model <= OF_MOTION_AFFINE, OF_EINVAL,
          "motion model must be 0 (translation), 1 (similarity) or 2 (affine)");
  REQUIRE(o->iters >= 0 && o->iters <= 64, OF_EINVAL, "motion iters must be 0..64");
  REQUIRE(std::isfinite(o->kappa) && o->kappa > 0, OF_EINVAL, "kappa must be finite and > 0");
  REQUIRE(std::isfinite(o->decay) && o->decay > 0 && o->decay <= 1, OF_EINVAL, "decay must be in (0, 1]");
  REQUIRE(std::isfinite(o->c_min) && o->c_min > 0, OF_EINVAL, "c_min must be finite and > 0");
}
void check_stab_opts(const of_stab_opts *o) {
  REQUIRE(o, OF_EINVAL, "no stabiliser options");
  check_motion_opts(&o->fit);
  REQUIRE(o->radius >= 1 && o->radius <= 30, OF_EINVAL, "stabiliser radius must be 1..30");
  REQUIRE(std::isfinite(o->sigma_t) && o->sigma_t > 0, OF_EINVAL, "sigma_t must be finite and > 0");
  check_alphas(o->alpha1, o->alpha2);
}

// th in normalised coordinates -> the pixel-coordinate matrix
void motion_matrix(const double *th, const MotionFrame &fr, double *M) {
  OF_NOCONTRACT
  const double s = fr.s;
  M[0] = 1.0 + th[1] / s;
  M[1] = th[2] / s;
  M[2] = th[0] - (th[1] * fr.cx + th[2] * fr.cy) / s;
  M[3] = th[4] / s;
  M[4] = 1.0 + th[5] / s;
  M[5] = th[3] - (th[4] * fr.cx + th[5] * fr.cy) / s;
}

// What the passes of a fit on an H x W flow share: the tile geometry, the
// frame's coordinates and the two arena buffers of the group tree.
struct MotionPasses {
  int H, W, ntx, nty, nt;  // nt < 2^31 / 8
  MotionFrame fr;
  double *rec[2];
  int stride[2];
  unsigned tile_blocks() const { return (unsigned)((nt + MOT_WAVES - 1) / MOT_WAVES); }
};
MotionPasses motion_passes(of_ctx *c, int H, int W) {
  MotionPasses p;
  p.H = H;
  p.W = W;
  p.ntx = (W + MOT_TW - 1) / MOT_TW;
  p.nty = (H + MOT_TH - 1) / MOT_TH;
  p.nt = p.ntx * p.nty;
  p.stride[0] = p.nt;
  p.stride[1] = (p.nt + 63) / 64;
  for (int k = 0; k < 2; ++k) p.rec[k] = (double *)c->arena.alloc(sizeof(double) * MOT_NS * p.stride[k]);
  p.fr.s = 0.5 * (double)(H > W ? H : W);
  p.fr.cx = 0.5 * (double)(W - 1);
  p.fr.cy = 0.5 * (double)(H - 1);
  return p;
}
// the tile records of one pass into p.rec[0]
void motion_part(of_ctx *c, const MotionPasses &p, const F2 &f, const float *dw, const uint8_t *ds,
                 const MotionState *ms, int pass, float *d_inl) {
  launch(c, "motion_part", k_motion_part, dim3(p.tile_blocks()), dim3(MOT_WAVES * 64), 0, (const float2 *)f.p, p.H, p.W,
         f.P, dw, ds, ms, pass, p.fr, p.ntx, p.nt, p.stride[0], p.rec[0], d_inl);
}
// One pass queued on the stream: the tile sums, the group tree down to <= 64
// values, then the last level with the solve; th and c2 stay in ms.
void motion_pass(of_ctx *c, const MotionPasses &p, const F2 &f, const float *dw, const uint8_t *ds, MotionState *ms,
                 int pass, int model, double kappa2, double decay, double cmin2, float *d_inl) {
  motion_part(c, p, f, dw, ds, ms, pass, d_inl);
  int n = p.nt, src = 0;
  while (n > 64) {  // the upper levels ping-pong between the two buffers
    const int ng = (n + 63) / 64;
    launch(c, "motion_group", k_motion_group, dim3((unsigned)((ng + MOT_WAVES - 1) / MOT_WAVES)), dim3(MOT_WAVES * 64),
           0, (const double *)p.rec[src], n, p.stride[src], p.rec[src ^ 1], p.stride[src ^ 1], (const MotionState *)ms,
           pass);
    n = ng;
    src ^= 1;
  }
  launch(c, "motion_final", k_motion_final, dim3(1), dim3(64), 0, (const double *)p.rec[src], n, p.stride[src], ms, pass,
         model, kappa2, decay, cmin2);
}

// The fit of `o` on the device-resident flow f; dw (dense H x W weights) and
// ds (dense H x W states) may be nullptr, d_inl (dense H x W) too.  Pass 0,
// o.iters robust passes and the last pass are queued as one chain.  One small
// read-back and one stream synchronisation at the end.
void fit_motion_dev(of_ctx *c, const F2 &f, const float *dw, const uint8_t *ds, const of_motion_opts &o,
                    of_motion_fit *out, float *d_inl) {
  const MotionPasses p = motion_passes(c, f.H, f.W);
  const MotionFrame &fr = p.fr;
  MotionState *ms = (MotionState *)c->arena.alloc(sizeof(MotionState));
  const double kappa2 = o.kappa * o.kappa, cmin2 = o.c_min * o.c_min;
  c->cur_px = (double)f.H * f.W;
  launch(c, "motion_init", k_motion_init, dim3(1), dim3(64), 0, ms, cmin2);
  for (int k = 0; k <= o.iters + 1; ++k) {
    const int pass = k == 0 ? MOT_PASS_FIRST : (k <= o.iters ? MOT_PASS_ROBUST : MOT_PASS_LAST);
    motion_pass(c, p, f, dw, ds, ms, pass, o.model, kappa2, o.decay, cmin2,
                pass == MOT_PASS_LAST ? d_inl : (float *)nullptr);
  }
  MotionState h;
  HIPCHK(hipMemcpyAsync(&h, ms, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 6; ++k) out->theta[k] = h.th[k];
  motion_matrix(h.th, fr, out->matrix);
  out->cutoff = std::sqrt(h.c2);
  out->support = h.sums[0];
  out->rms = std::sqrt(h.sums[12] / h.sums[0]);
  out->passes = h.passes;
  out->degenerate = h.degenerate;
}

// device-resident frame (dense H x W x C) through the matrix A into the host buffers
void warp_affine_dev(of_ctx *c, const float *dim, int H, int W, int C, const double A[6], float *out, uint8_t *valid) {
  const size_t px = (size_t)H * W;
  float *dout = new_dense<float>(c, px * C);
  uint8_t *dv = new_dense<uint8_t>(c, px, valid);
  AffineMat M;
  for (int k = 0; k < 6; ++k) M.a[k] = A[k];
  c->cur_px = (double)px;
  const Grid2 g = grid2(H, W);
  launch(c, "warp_affine", k_warp_affine, g.grid, g.block, 0, dim, C, M, H, W, dout, dv);
  download_dense(c, out, dout, px * C);
  download_dense(c, valid, dv, px);
  HIPCHK(hipStreamSynchronize(c->stream));
}

// ---- path smoothing: 2 x 3 matrices [a b tx; c d ty] on the host ----
const Mat6 MAT6_I = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}};

bool mat6_invertible(const Mat6 &m) {
  OF_NOCONTRACT
  for (double v : m.a)
    if (!std::isfinite(v)) return false;
  const double det = m.a[0] * m.a[4] - m.a[1] * m.a[3];
  return std::fabs(det) >= 1e-12;
}
// the inverse of an invertible matrix
Mat6 mat6_inv(const Mat6 &m) {
  OF_NOCONTRACT
  const double a = m.a[0], b = m.a[1], tx = m.a[2], cc = m.a[3], d = m.a[4], ty = m.a[5];
  const double det = a * d - b * cc;
  const double ia = d / det, ib = -b / det, ic = -cc / det, id = a / det;
  return Mat6{{ia, ib, -(ia * tx + ib * ty), ic, id, -(ic * tx + id * ty)}};
}
// X o Y: Y first
Mat6 mat6_mul(const Mat6 &X, const Mat6 &Y) {
  OF_NOCONTRACT
  const double *x = X.a, *y = Y.a;
  return Mat6{{x[0] * y[0] + x[1] * y[3], x[0] * y[1] + x[1] * y[4], (x[0] * y[2] + x[1] * y[5]) + x[2],
               x[3] * y[0] + x[4] * y[3], x[3] * y[1] + x[4] * y[4], (x[3] * y[2] + x[4] * y[5]) + x[5]}};
}

// S_t of the session: the Gaussian-weighted mean of the paths from frame t to
// its neighbours t + d, d = 0, -1, +1, -2, +2, ... within the radius and the
// clip so far (frames 0 .. s->frames - 1; M_k links k and k + 1)
Mat6 stab_smooth(const Stabilizer *s, int t) {
  OF_NOCONTRACT
  const int R = s->opt.radius;
  const double two_s2 = (2.0 * s->opt.sigma_t) * s->opt.sigma_t;
  auto M = [&](int k) -> const Mat6 & { return s->motion[k - s->motion0]; };
  double num[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, den = 0.0;
  Mat6 back = MAT6_I, fwd = MAT6_I;  // P(t -> t - d), P(t -> t + d)
  auto add = [&](const Mat6 &P, int d) {
    OF_NOCONTRACT
    const double g = std::exp(-((double)d * (double)d) / two_s2);
    for (int e = 0; e < 6; ++e) num[e] = num[e] + g * P.a[e];
    den = den + g;
  };
  add(MAT6_I, 0);
  for (int d = 1; d <= R; ++d) {
    if (t - d >= 0) {
      back = mat6_mul(mat6_inv(M(t - d)), back);
      add(back, d);
    }
    if (t + d <= s->frames - 1) {
      fwd = mat6_mul(M(t + d - 1), fwd);
      add(fwd, d);
    }
  }
  Mat6 S;
  for (int e = 0; e < 6; ++e) S.a[e] = num[e] / den;
  return S;
}

// frame t of the session warped onto the smoothed path, into the host buffers
void stab_emit(of_ctx *c, Stabilizer *s, int t, float *out, uint8_t *out_valid, double *out_transform,
               int32_t *degenerate) {
  const Mat6 S = stab_smooth(s, t);
  if (out_transform)
    for (int e = 0; e < 6; ++e) out_transform[e] = S.a[e];
  Mat6 inv = MAT6_I;
  if (mat6_invertible(S)) inv = mat6_inv(S);
  else *degenerate |= 4;
  warp_affine_dev(c, s->frame[t % s->frame.size()], s->H, s->W, s->C, inv.a, out, out_valid);
  // motions before t + 1 - radius are not needed again
  while (s->motion0 < t + 1 - s->opt.radius && !s->motion.empty()) {
    s->motion.pop_front();
    ++s->motion0;
  }
}

}  // namespace

extern "C" {

int of_fit_motion(of_ctx *c, const float *uv, int H, int W, const float *weight, const uint8_t *state,
                  const of_motion_opts *o, of_motion_fit *out, float *out_inlier) {
  API_BEGIN(c)
  REQUIRE(uv && out, OF_EINVAL, "bad arguments");
  check_frame(H, W, "global motion");
  check_motion_opts(o);
  const size_t px = (size_t)H * W;
  if (weight)
    for (size_t k = 0; k < px; ++k)
      REQUIRE(std::isfinite(weight[k]) && weight[k] >= 0, OF_EINVAL, "weight must be finite and >= 0 everywhere");
  const F2 f = upload_f2(c, uv, H, W);
  float *dw = upload_dense(c, weight, px);
  uint8_t *ds = upload_dense(c, state, px);
  float *dinl = new_dense<float>(c, px, out_inlier);
  fit_motion_dev(c, f, dw, ds, *o, out, dinl);
  download_dense(c, out_inlier, dinl, px);
  if (out_inlier) HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_warp_affine(of_ctx *c, const float *im, int H, int W, int C, const double A[6], float *out, uint8_t *valid) {
  API_BEGIN(c)
  REQUIRE(im && A && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= OF_MAX_NC, OF_EINVAL, "images must have 1 to 4 channels");
  check_frame(H, W, "global motion");
  const size_t px = (size_t)H * W;
  warp_affine_dev(c, upload_dense(c, im, px * C), H, W, C, A, out, valid);
  API_END(c)
}

int of_stab_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_stab_opts *o) {
  API_BEGIN(c)
  session_open<Stabilizer>(c, SES_STAB, P, H, W, C, o, check_stab_opts,
                           [&](Stabilizer *s) { s->alloc_frames(o->radius + 1); });
  API_END(c)
}

int of_stab_push(of_ctx *c, const float *frame, float *out, uint8_t *out_valid, double *out_transform,
                 double *out_motion, int32_t *degenerate, int32_t *out_index) {
  API_BEGIN(c)
  Stabilizer *s = session_get<Stabilizer>(c, SES_STAB);
  REQUIRE(frame && out && degenerate && out_index, OF_EINVAL, "bad arguments");
  session_not_flushed(s, SES_STAB);
  *degenerate = 0;
  uint8_t *sf = new_dense<uint8_t>(c, (size_t)s->H * s->W, s->frames > 0);
  const PushPair p = session_push(c, s, frame, s->opt.alpha1, s->opt.alpha2, sf, nullptr, nullptr, nullptr);
  if (s->frames > 0) {
    of_motion_fit fit;
    fit_motion_dev(c, p.fw, nullptr, sf, s->opt.fit, &fit, nullptr);
    Mat6 M;
    for (int e = 0; e < 6; ++e) M.a[e] = fit.matrix[e];
    *degenerate = fit.degenerate;
    if (!mat6_invertible(M)) {
      M = MAT6_I;
      *degenerate |= 4;
    }
    s->motion.push_back(M);
    if (out_motion)
      for (int e = 0; e < 6; ++e) out_motion[e] = M.a[e];
  }
  *out_index = -1;
  const int t = session_next_emit(s, s->opt.radius, false);
  if (t >= 0) {
    stab_emit(c, s, t, out, out_valid, out_transform, degenerate);
    *out_index = t;
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));  // the caller's frame has been read
  }
  API_END(c)
}

int of_stab_flush(of_ctx *c, float *out, uint8_t *out_valid, double *out_transform, int32_t *degenerate,
                  int32_t *out_index) {
  API_BEGIN(c)
  Stabilizer *s = session_get<Stabilizer>(c, SES_STAB);
  REQUIRE(out && degenerate && out_index, OF_EINVAL, "bad arguments");
  *degenerate = 0;
  *out_index = -1;
  const int t = session_next_emit(s, s->opt.radius, true);
  if (t >= 0) {
    stab_emit(c, s, t, out, out_valid, out_transform, degenerate);
    *out_index = t;
  }
  API_END(c)
}

int of_stab_close(of_ctx *c) { return session_close(c, SES_STAB); }

}  // extern "C"
