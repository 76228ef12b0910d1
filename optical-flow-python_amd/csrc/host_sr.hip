// host_sr.hip — host side of the multi-frame super-resolution
// (kernels_sr.hip): option checks, the resampling with its neighbour weights
// (k_fuse_weights) and the back-projection step on device-resident frames,
// flows and states, the stage entry on host buffers and the per-context
// super-resolver session, which keeps the denoiser's rings (host_fuse.hip).
namespace {

void check_sr_opts(const of_sr_opts *o) {
  REQUIRE(o, OF_EINVAL, "no super-resolution options");
  REQUIRE(o->factor >= SR_MIN_S && o->factor <= SR_MAX_S, OF_EINVAL, "factor must be 2..4");
  REQUIRE(o->radius >= 1 && o->radius <= 2, OF_EINVAL, "super-resolution radius must be 1..2");
  REQUIRE(o->patch >= 0 && o->patch <= FUSE_MAX_R, OF_EINVAL, "patch must be 0..3");
  REQUIRE(std::isfinite(o->sigma) && o->sigma > 0 && std::isfinite(o->strength) && o->strength > 0, OF_EINVAL,
          "sigma and strength must be finite and > 0");
  REQUIRE(std::isfinite(o->reach) && o->reach >= 0.75 && o->reach <= 1.5, OF_EINVAL, "reach must be 0.75..1.5");
  REQUIRE(std::isfinite(o->back) && o->back >= 0 && o->back <= 1, OF_EINVAL, "back must be 0..1");
  check_alphas(o->alpha1, o->alpha2);
}

// an output of s*H x s*W whose pixel index fits 31 bits
void check_sr_frame(int H, int W, int s) {
  check_frame(H, W, "super-resolution");
  REQUIRE((size_t)s * s * (size_t)H * W < ((size_t)1 << 31), OF_ENOTSUP, "super-resolution takes s*s*H*W < 2^31");
}

// the frame `center` and n neighbours (0..8) along flows centre -> neighbour
// onto the grid s times finer; everything device-resident (frames dense
// H x W x C, flows of pitch P, states dense or nullptr), out dense
// sH x sW x C, out_s dense sH x sW or nullptr
void super_resolve_dev(of_ctx *c, const float *center, int H, int W, int C, int P, int n, const float *const *neigh,
                       const float2 *const *flow, const uint8_t *const *state, const of_sr_opts &o, float *out,
                       float *out_s) {
  const int s = o.factor, sH = s * H, sW = s * W;
  const size_t px = (size_t)H * W;
  float *wk = new_dense<float>(c, px * n, n > 0);
  if (n > 0) fuse_weights_dev(c, center, H, W, C, P, n, neigh, flow, state, o.sigma, o.strength, o.patch, wk);
  const FuseArgs A = fuse_args(n, neigh, flow, state);
  const int gx = (sW + SR_TW - 1) / SR_TW, gy = (sH + SR_TH - 1) / SR_TH;
  const dim3 grid((unsigned)gx * (unsigned)gy), block(SR_TW * SR_TH);
  c->cur_px = (double)sH * sW;
  auto go = [&](auto kernel) {
    launch(c, "super_resolve", kernel, grid, block, 0, center, A, (const float *)wk, n, H, W, P, C, s,
           o.reach * o.reach, gx, out, out_s);
  };
  if (C == 1) go(k_super_resolve<1>);
  else if (C == 3) go(k_super_resolve<3>);
  else go(k_super_resolve<0>);
  if (o.back > 0) {
    float *L = new_dense<float>(c, px * C);
    reduce_frame_dev(c, out, sH, sW, C, s, L);
    c->cur_px = (double)sH * sW;
    const Grid2 g = grid2(sH, sW);
    launch(c, "sr_back", k_sr_back, g.grid, g.block, 0, center, (const float *)L, sH, sW, W, C, s, o.back, out);
  }
}

// frame t of the session with its neighbours (ring_neighbours), written to the
// host buffers
void sr_emit(of_ctx *c, SuperResolver *d, int t, float *out, float *out_support) {
  const int H = d->H, W = d->W, C = d->C, s = d->opt.factor;
  const size_t opx = (size_t)s * s * H * W;
  const float *neigh[4];
  const float2 *flow[4];
  const uint8_t *state[4];
  const int n = ring_neighbours(c, d, t, d->opt.radius, neigh, flow, state);
  float *dout = new_dense<float>(c, opx * C), *dsup = new_dense<float>(c, opx, out_support);
  super_resolve_dev(c, d->frame[t % (int)d->frame.size()], H, W, C, d->pitch, n, neigh, flow, state, d->opt, dout,
                    dsup);
  download_dense(c, out, dout, opx * C);
  download_dense(c, out_support, dsup, opx);
  HIPCHK(hipStreamSynchronize(c->stream));
}

}  // namespace

extern "C" {

int of_super_resolve(of_ctx *c, const float *center, int H, int W, int C, int n, const float *neigh, const float *flows,
                     const uint8_t *states, const of_sr_opts *o, float *out, float *out_support) {
  API_BEGIN(c)
  REQUIRE(center && out && n >= 0 && n <= FUSE_MAX_N && (n == 0 || (neigh && flows)), OF_EINVAL,
          "bad arguments (0..8 neighbours)");
  REQUIRE(C >= 1 && C <= FUSE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_sr_opts(o);
  check_sr_frame(H, W, o->factor);
  const size_t opx = (size_t)o->factor * o->factor * H * W;
  const FuseInputs in = upload_fuse_inputs(c, center, H, W, C, n, neigh, flows, states);
  float *dout = new_dense<float>(c, opx * C), *dsup = new_dense<float>(c, opx, out_support);
  super_resolve_dev(c, in.center, H, W, C, of_pitch(W), n, in.neigh, in.flow, in.state, *o, dout, dsup);
  download_dense(c, out, dout, opx * C);
  download_dense(c, out_support, dsup, opx);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_sr_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_sr_opts *o) {
  API_BEGIN(c)
  session_open<SuperResolver>(c, SES_SR, P, H, W, C, o, check_sr_opts, [&](SuperResolver *d) {
    check_sr_frame(H, W, o->factor);
    ring_alloc(d, o->radius);
  });
  API_END(c)
}

int of_sr_push(of_ctx *c, const float *frame, float *out, float *out_support, int32_t *out_index) {
  API_BEGIN(c)
  SuperResolver *d = session_get<SuperResolver>(c, SES_SR);
  REQUIRE(frame && out && out_index, OF_EINVAL, "bad arguments");
  session_not_flushed(d, SES_SR);
  ring_push(c, d, d->opt.radius, frame, d->opt.alpha1, d->opt.alpha2);
  *out_index = -1;
  const int t = session_next_emit(d, d->opt.radius, false);
  if (t >= 0) {
    sr_emit(c, d, t, out, out_support);
    *out_index = t;
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));  // the caller's frame has been read
  }
  API_END(c)
}

int of_sr_flush(of_ctx *c, float *out, float *out_support, int32_t *out_index) {
  API_BEGIN(c)
  SuperResolver *d = session_get<SuperResolver>(c, SES_SR);
  REQUIRE(out && out_index, OF_EINVAL, "bad arguments");
  *out_index = -1;
  const int t = session_next_emit(d, d->opt.radius, true);
  if (t >= 0) {
    sr_emit(c, d, t, out, out_support);
    *out_index = t;
  }
  API_END(c)
}

int of_sr_close(of_ctx *c) { return session_close(c, SES_SR); }

}  // extern "C"
