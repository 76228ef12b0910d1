// host_upsample.hip — host side of the reduced-resolution flow
// (kernels_upsample.hip): option checks, the box reduction and the edge-aware
// upsampling on device-resident frames and flows, the scaled estimates built
// from them and the existing estimates, and the stage and one-call entries on
// host buffers.  The sessions' switch (of_session_set_flow_scale) lives with
// the sessions, host_session.hip.
namespace {

// scale 1 ("off") is valid only where `allow_off` says so; range is then not read
void check_upsample_opts(const of_upsample_opts *o, bool allow_off = false) {
  REQUIRE(o, OF_EINVAL, "no upsample options");
  if (allow_off && o->scale == 1) return;
  REQUIRE(o->scale >= UP_MIN_S && o->scale <= UP_MAX_S, OF_EINVAL, "scale must be 2..4");
  REQUIRE(std::isfinite(o->range) && o->range > 0, OF_EINVAL, "range must be finite and > 0");
}

inline int low_size(int n, int s) { return (n + s - 1) / s; }

// the box reduction of a device-resident frame (dense H x W x C) into `out`
// (dense hs x ws x C)
void reduce_frame_dev(of_ctx *c, const float *im, int H, int W, int C, int s, float *out) {
  const int hs = low_size(H, s), ws = low_size(W, s);
  c->cur_px = (double)hs * ws;
  const Grid2 g = grid2(hs, ws);
  launch(c, "reduce_frame", k_reduce_frame, g.grid, g.block, 0, im, H, W, C, s, hs, ws, out);
}

// the low flow `lo` (hs x ws) with its low guide L (dense hs x ws x C) onto
// the full guide G (dense H x W x C): out is H x W, info dense H x W or nullptr
void flow_upsample_dev(of_ctx *c, const F2 &lo, const float *L, const float *G, int H, int W, int C,
                       const of_upsample_opts &o, const F2 &out, uint8_t *info) {
  const int s = o.scale, hs = low_size(H, s), ws = low_size(W, s);
  REQUIRE(lo.H == hs && lo.W == ws && out.H == H && out.W == W, OF_EINVAL, "flows of the wrong size");
  const double h2 = o.range * o.range, ch2 = (double)C * h2;
  const int gx = (W + UP_TW - 1) / UP_TW, gy = (H + UP_TH - 1) / UP_TH;
  const dim3 grid((unsigned)gx * (unsigned)gy), block(256);
  c->cur_px = (double)H * W;
  auto go = [&](auto kernel) {
    launch(c, "flow_upsample", kernel, grid, block, 0, (const float2 *)lo.p, lo.P, L, G, H, W, hs, ws, C, s, ch2, gx,
           out.p, out.P, info);
  };
  if (C == 1) go(k_flow_upsample<1>);
  else if (C == 3) go(k_flow_upsample<3>);
  else go(k_flow_upsample<0>);
}

// The reduced frames of a scaled estimate, their size and the GPU time of the
// reduction (between the two events, for preprocess_ms)
struct LowPair {
  float *L1 = nullptr, *L2 = nullptr;
  int hs = 0, ws = 0;
  hipEvent_t t0 = nullptr, t1 = nullptr;
};
LowPair reduce_pair(of_ctx *c, const float *rgb1, const float *rgb2, int H, int W, int C, int s) {
  LowPair p;
  p.hs = low_size(H, s);
  p.ws = low_size(W, s);
  const size_t n = (size_t)p.hs * p.ws * C;
  p.L1 = new_dense<float>(c, n);
  p.L2 = new_dense<float>(c, n);
  p.t0 = timing_event(c);
  p.t1 = timing_event(c);
  HIPCHK(hipEventRecord(p.t0, c->stream));
  reduce_frame_dev(c, rgb1, H, W, C, s, p.L1);
  reduce_frame_dev(c, rgb2, H, W, C, s, p.L2);
  HIPCHK(hipEventRecord(p.t1, c->stream));
  return p;
}

// estimate_dev on the reduced pair, upsampled along frame 1.  rgb1 / rgb2:
// (H, W, C) fp32 frames on the device; uv: the full-resolution result.
void estimate_scaled_dev(of_ctx *c, of_params *P, const float *rgb1, const float *rgb2, int H, int W, int C,
                         const of_upsample_opts &o, const F2 &uv, of_stats *st) {
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "images must be (H,W) or (H,W,3)");
  const LowPair p = reduce_pair(c, rgb1, rgb2, H, W, C, o.scale);
  F2 lo = init_flow(c, nullptr, p.hs, p.ws);
  estimate_dev(c, P, p.L1, p.L2, false, p.hs, p.ws, C, lo, st);  // ends in a stream synchronisation
  add_preprocess_ms(st, p.t0, p.t1);
  flow_upsample_dev(c, lo, p.L1, rgb1, H, W, C, o, uv, nullptr);
}

// estimate_bidir_dev on the reduced pair; each low flow upsampled along its
// own first frame; the states from the full-resolution flows.  st_fw / st_bw:
// dense H x W device bytes or nullptr.
void estimate_bidir_scaled_dev(of_ctx *c, of_params *P, const float *rgb1, const float *rgb2, int H, int W, int C,
                               const of_upsample_opts &o, const F2 &uv_fw, const F2 &uv_bw, double alpha1,
                               double alpha2, uint8_t *st_fw, uint8_t *st_bw, of_stats *sf, of_stats *sb) {
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "images must be (H,W) or (H,W,3)");
  const LowPair p = reduce_pair(c, rgb1, rgb2, H, W, C, o.scale);
  F2 lf = init_flow(c, nullptr, p.hs, p.ws), lb = init_flow(c, nullptr, p.hs, p.ws);
  estimate_bidir_dev(c, P, p.L1, p.L2, p.hs, p.ws, C, lf, lb, alpha1, alpha2, nullptr, nullptr, sf, sb);
  add_preprocess_ms(sf, p.t0, p.t1);
  flow_upsample_dev(c, lf, p.L1, rgb1, H, W, C, o, uv_fw, nullptr);
  flow_upsample_dev(c, lb, p.L2, rgb2, H, W, C, o, uv_bw, nullptr);
  if (st_fw) fb_check(c, uv_fw, uv_bw, alpha1, alpha2, st_fw, nullptr, st_bw, nullptr);
  else if (st_bw) fb_check(c, uv_bw, uv_fw, alpha1, alpha2, st_bw, nullptr, nullptr, nullptr);
}

}  // namespace

extern "C" {

int of_reduce_frame(of_ctx *c, const float *im, int H, int W, int C, int scale, float *out) {
  API_BEGIN(c)
  REQUIRE(im && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= UP_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  REQUIRE(scale >= UP_MIN_S && scale <= UP_MAX_S, OF_EINVAL, "scale must be 2..4");
  check_frame(H, W, "the reduced-resolution flow");
  const size_t n = (size_t)low_size(H, scale) * low_size(W, scale) * C;
  const float *dim = upload_dense(c, im, (size_t)H * W * C);
  float *dout = new_dense<float>(c, n);
  reduce_frame_dev(c, dim, H, W, C, scale, dout);
  download_dense(c, out, dout, n);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_flow_upsample(of_ctx *c, const float *f_lo, const float *L, const float *G, int H, int W, int C,
                     const of_upsample_opts *o, float *out_uv, uint8_t *out_info) {
  API_BEGIN(c)
  REQUIRE(f_lo && L && G && out_uv, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= UP_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_upsample_opts(o);
  check_frame(H, W, "the reduced-resolution flow");
  const int hs = low_size(H, o->scale), ws = low_size(W, o->scale);
  const size_t px = (size_t)H * W;
  const F2 lo = upload_f2(c, f_lo, hs, ws), out = new_f2(c, H, W);
  const float *dL = upload_dense(c, L, (size_t)hs * ws * C), *dG = upload_dense(c, G, px * C);
  uint8_t *di = new_dense<uint8_t>(c, px, out_info);
  flow_upsample_dev(c, lo, dL, dG, H, W, C, *o, out, di);
  download_f2(c, out, out_uv);
  download_dense(c, out_info, di, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_estimate_flow_scaled(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                            const of_upsample_opts *o, float *out_uv, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out_uv, OF_EINVAL, "bad arguments");
  check_upsample_opts(o);
  check_frame(H, W, "the reduced-resolution flow");
  if (st) memset(st, 0, sizeof(*st));
  const WallClock wall;
  float *d1, *d2;
  upload_frames(c, im1, im2, (size_t)H * W * C, &d1, &d2);
  const F2 uv = new_f2(c, H, W);
  estimate_scaled_dev(c, P, d1, d2, H, W, C, *o, uv, st);
  download_f2(c, uv, out_uv);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) st->total_ms = wall.ms();
  API_END(c)
}

int of_estimate_flow_bidir_scaled(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                                  const of_upsample_opts *o, double alpha1, double alpha2, float *out_fw,
                                  float *out_bw, uint8_t *state_fw, uint8_t *state_bw, of_stats *sf, of_stats *sb) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out_fw && out_bw, OF_EINVAL, "bad arguments");
  check_upsample_opts(o);
  check_alphas(alpha1, alpha2);
  check_frame(H, W, "the reduced-resolution flow");
  if (sf) memset(sf, 0, sizeof(*sf));
  if (sb) memset(sb, 0, sizeof(*sb));
  const WallClock wall;  // the forward pass's total_ms; the backward pass has its own
  const size_t px = (size_t)H * W;
  float *d1, *d2;
  upload_frames(c, im1, im2, px * C, &d1, &d2);
  const F2 uf = new_f2(c, H, W), ub = new_f2(c, H, W);
  uint8_t *dsf = new_dense<uint8_t>(c, px, state_fw), *dsb = new_dense<uint8_t>(c, px, state_bw);
  estimate_bidir_scaled_dev(c, P, d1, d2, H, W, C, *o, uf, ub, alpha1, alpha2, dsf, dsb, sf, sb);
  download_f2(c, uf, out_fw);
  download_f2(c, ub, out_bw);
  download_dense(c, state_fw, dsf, px);
  download_dense(c, state_bw, dsb, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (sf) sf->total_ms = wall.ms();
  API_END(c)
}

}  // extern "C"
