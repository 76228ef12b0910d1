// host_mask.hip — host side of the mask propagation (kernels_mask.hip):
// option checks, one step on a device-resident mask, guide, flow and state, the
// stage entry on host buffers and the per-context mask propagator session,
// which estimates its pairs through session_push (host_session.hip) and keeps
// the previous frame and the current mask.
namespace {

void check_mask_opts(const of_mask_opts *o) {
  REQUIRE(o, OF_EINVAL, "no mask options");
  REQUIRE(o->vote_radius >= 1 && o->vote_radius <= MSK_MAX_R, OF_EINVAL, "vote_radius must be 1..12");
  REQUIRE(o->smooth >= 0 && o->smooth <= MSK_MAX_S, OF_EINVAL, "smooth must be 0..2");
  REQUIRE(std::isfinite(o->range) && o->range > 0, OF_EINVAL, "range must be finite and > 0");
  check_alphas(o->alpha1, o->alpha2);
}

// One step: the mask M of the previous frame along the flow B (current ->
// previous, state S or nullptr) under the guide G, the current frame;
// everything device-resident (M, S, out and status dense H x W bytes, G dense
// H x W x C, status or nullptr).  out may be M: the carry has read M before the
// later kernels write.
void mask_advance_dev(of_ctx *c, const uint8_t *M, const float *G, int H, int W, int C, const F2 &B, const uint8_t *S,
                      const of_mask_opts &o, uint8_t *out, uint8_t *status) {
  const size_t px = (size_t)H * W;
  const Grid2 g = grid2(H, W);
  const int gx = (W + MSK_TW - 1) / MSK_TW, gy = (H + MSK_TH - 1) / MSK_TH;
  const dim3 tiles((unsigned)gx * (unsigned)gy), block(MSK_TW * MSK_TH);
  float *A = new_dense<float>(c, px);
  uint8_t *lab = o.smooth > 0 ? new_dense<uint8_t>(c, px) : out;
  c->cur_px = (double)px;
  launch(c, "mask_carry", k_mask_carry, g.grid, g.block, 0, M, (const float2 *)B.p, S, H, W, B.P, A);
  auto go = [&](auto kernel) {
    launch(c, "mask_vote", kernel, tiles, block, 0, (const float *)A, G, H, W, C, o.vote_radius, o.range * o.range, gx, lab,
           status);
  };
  if (C == 1) go(k_mask_vote<1>);
  else if (C == 3) go(k_mask_vote<3>);
  else go(k_mask_vote<0>);
  if (o.smooth > 0) launch(c, "mask_mode", k_mask_mode, tiles, block, 0, (const uint8_t *)lab, H, W, o.smooth, gx, out);
}

}  // namespace

extern "C" {

int of_mask_advance(of_ctx *c, const uint8_t *prev_mask, const float *guide, int H, int W, int C, const float *flow,
                    const uint8_t *state, const of_mask_opts *o, uint8_t *out_mask, uint8_t *out_status) {
  API_BEGIN(c)
  REQUIRE(prev_mask && guide && flow && out_mask, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= MSK_MAX_C, OF_EINVAL, "the guide must have 1..4 channels");
  check_mask_opts(o);
  check_frame(H, W, "mask propagation");
  const size_t px = (size_t)H * W;
  const uint8_t *dm = upload_dense(c, prev_mask, px), *ds = upload_dense(c, state, px);
  const float *dg = upload_dense(c, guide, px * C);
  const F2 b = upload_f2(c, flow, H, W);
  uint8_t *dout = new_dense<uint8_t>(c, px), *dst = new_dense<uint8_t>(c, px, out_status);
  mask_advance_dev(c, dm, dg, H, W, C, b, ds, *o, dout, dst);
  download_dense(c, out_mask, dout, px);
  download_dense(c, out_status, dst, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_masks_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_mask_opts *o) {
  API_BEGIN(c)
  session_open<MaskPropagator>(c, SES_MASKS, P, H, W, C, o, check_mask_opts, [&](MaskPropagator *d) {
    d->alloc_frames(2);
    d->mask = d->alloc<uint8_t>((size_t)H * W);
  });
  API_END(c)
}

int of_masks_push(of_ctx *c, const float *frame, const uint8_t *mask, uint8_t *out_mask, uint8_t *out_status) {
  API_BEGIN(c)
  MaskPropagator *d = session_get<MaskPropagator>(c, SES_MASKS);
  REQUIRE(frame && out_mask, OF_EINVAL, "bad arguments");
  REQUIRE(mask || d->frames > 0, OF_EINVAL, "the first push of the mask propagator takes a mask");
  const int H = d->H, W = d->W, C = d->C;
  const size_t px = (size_t)H * W;
  if (mask) {
    // a keyframe: the frame becomes the previous one, the mask is stored as mask != 0, nothing is estimated
    float *cur = d->frame[d->frames % 2];
    HIPCHK(hipMemcpyAsync(cur, frame, sizeof(float) * px * C, hipMemcpyHostToDevice, c->stream));
    mask_grow_dev(c, upload_dense(c, mask, px), nullptr, H, W, 0, d->mask, nullptr, 0);
    download_dense(c, out_mask, (const uint8_t *)d->mask, px);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out_status) memset(out_status, OF_MASK_GIVEN, px);
  } else {
    uint8_t *dsb = new_dense<uint8_t>(c, px), *dst = new_dense<uint8_t>(c, px, out_status);
    const PushPair p = session_push(c, d, frame, d->opt.alpha1, d->opt.alpha2, nullptr, dsb, nullptr, nullptr);
    mask_advance_dev(c, d->mask, p.cur, H, W, C, p.bw, dsb, d->opt, d->mask, dst);
    download_dense(c, out_mask, (const uint8_t *)d->mask, px);
    download_dense(c, out_status, dst, px);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  d->frames += 1;
  API_END(c)
}

int of_masks_close(of_ctx *c) { return session_close(c, SES_MASKS); }

}  // extern "C"
