// host_inpaint.hip — host side of the flow-guided video inpainting
// (kernels_inpaint.hip): option checks, the mask growing and the pair weight,
// the fill on device-resident frames, masks and flows, the blended fill (the
// fill with the masks grown by one more, then two Poisson solves,
// host_poisson.hip), the stage entries on
// host buffers and the per-context inpainter session, which estimates its
// pairs with the pair weight (estimate_dev, host_flow.hip) and keeps its own
// rings.
namespace {

void check_inpaint_opts(const of_inpaint_opts *o) {
  REQUIRE(o, OF_EINVAL, "no inpainting options");
  REQUIRE(o->radius >= 1 && o->radius <= INP_MAX_R, OF_EINVAL, "inpainting radius must be 1..16");
  REQUIRE(o->grow >= 0 && o->grow <= OF_INPAINT_MAX_GROW, OF_EINVAL, "grow must be 0..8");
  REQUIRE(o->margin >= 0 && o->margin <= OF_INPAINT_MAX_MARGIN, OF_EINVAL, "margin must be 0..16");
}

// grow(a | b, g) on the device: a, b (or nullptr) dense H x W bytes; out_m
// dense bytes or nullptr; out_w fp32 rows of pitch wP or nullptr
void mask_grow_dev(of_ctx *c, const uint8_t *a, const uint8_t *b, int H, int W, int g, uint8_t *out_m, float *out_w,
                   int wP) {
  const int gx = (W + INP_TW - 1) / INP_TW, gy = (H + INP_TH - 1) / INP_TH;
  c->cur_px = (double)H * W;
  launch(c, "mask_grow", k_mask_grow, dim3((unsigned)gx * (unsigned)gy), dim3(INP_TW * INP_TH), 0, a, b, H, W, g, gx,
         out_m, out_w, wP);
}

// frame I with grown mask D filled along the hops of A; everything
// device-resident, out dense H x W x C, status and hops dense or nullptr
void inpaint_fill_dev(of_ctx *c, const float *I, const uint8_t *D, const InpaintArgs &A, int H, int W, int C, int P,
                      float *out, uint8_t *status, uint8_t *hops) {
  const Grid2 g = grid2(H, W);
  c->cur_px = (double)H * W;
  auto go = [&](auto kernel) { launch(c, "inpaint_fill", kernel, g.grid, g.block, 0, I, D, A, H, W, P, C, out, status, hops); };
  if (C == 1) go(k_inpaint_fill<1>);
  else if (C == 3) go(k_inpaint_fill<3>);
  else go(k_inpaint_fill<0>);
}

// The hops of frame t among frames 0 .. T-1 within radius R: frame_of(s),
// mask_of(s), fw_of(s) and bw_of(s) give frame s, its grown mask and the flows
// of pair (s, s+1) on the device.
template <typename Fr, typename Mk, typename Fw, typename Bw>
InpaintArgs inpaint_hops(int t, int T, int R, Fr frame_of, Mk mask_of, Fw fw_of, Bw bw_of) {
  InpaintArgs A = {};
  for (int d = 1; d <= R && t + d < T; ++d) {
    A.flow[0][d - 1] = fw_of(t + d - 1);
    A.mask[0][d - 1] = mask_of(t + d);
    A.frame[0][d - 1] = frame_of(t + d);
    A.n[0] = d;
  }
  for (int d = 1; d <= R && t - d >= 0; ++d) {
    A.flow[1][d - 1] = bw_of(t - d);
    A.mask[1][d - 1] = mask_of(t - d);
    A.frame[1][d - 1] = frame_of(t - d);
    A.n[1] = d;
  }
  return A;
}

// The blended fill of frame I (of_inpaint_blend, include/optflow.h): D1 and
// the masks of A are grown by one more than Om, the frame's grown mask, whose
// bounding box `box` was taken on the host.  Everything device-resident, out
// dense H x W x C, status dense or nullptr.
void inpaint_blend_dev(of_ctx *c, const float *I, const uint8_t *D1, const uint8_t *Om, const InpaintArgs &A, int H,
                       int W, int C, int P, const PsnBox &box, const of_blend_opts &bo, float *out, uint8_t *status) {
  const size_t px = (size_t)H * W;
  const Grid2 g = grid2(H, W);
  PsnPlan p;
  PsnWin win = {0, 0, 0, 0};
  const double *x = nullptr;
  const uint8_t *hs = nullptr;
  if (!box.empty()) {
    float *s = new_dense<float>(c, px * C);
    uint8_t *st = new_dense<uint8_t>(c, px);
    inpaint_fill_dev(c, I, D1, A, H, W, C, P, s, st, nullptr);
    uint8_t *lab1 = new_dense<uint8_t>(c, px), *lab2 = new_dense<uint8_t>(c, px), *h = new_dense<uint8_t>(c, px);
    c->cur_px = (double)px;
    launch(c, "blend_labels", k_blend_labels, g.grid, g.block, 0, Om, (const uint8_t *)st, H, W, lab1, lab2, h);
    p = psn_plan(c, H, W, C, box);
    psn_setup(c, p, lab1, I, s, s, h, H, W, false);
    psn_run(c, p, bo);
    psn_setup(c, p, lab2, I, nullptr, nullptr, nullptr, H, W, true);
    psn_run(c, p, bo);
    win = p.lv[0].win;
    x = p.lv[0].x[p.lv[0].cur];
    hs = h;
  }
  c->cur_px = (double)px;
#define PSN_CALL(CT) launch(c, "blend_store", k_blend_store<CT>, g.grid, g.block, 0, I, Om, hs, x, win, H, W, out, status)
  PSN_FOR_C(C, PSN_CALL);
#undef PSN_CALL
}

// frame t of the session filled from the frames and pairs within its radius
// that exist (blended after of_inpaint_set_blend), written to the host buffers
void inpaint_emit(of_ctx *c, Inpainter *d, int t, float *out, uint8_t *out_status) {
  const int H = d->H, W = d->W, C = d->C, R = d->opt.radius, NF = 2 * R + 1, NP = 2 * R;
  const size_t px = (size_t)H * W;
  const std::vector<uint8_t *> &masks = d->blend ? d->mask1 : d->mask;
  const InpaintArgs A = inpaint_hops(
      t, d->frames, R, [&](int s) { return (const float *)d->frame[s % NF]; },
      [&](int s) { return (const uint8_t *)masks[s % NF]; }, [&](int s) { return (const float2 *)d->fw[s % NP]; },
      [&](int s) { return (const float2 *)d->bw[s % NP]; });
  float *dout = new_dense<float>(c, px * C);
  uint8_t *dst = new_dense<uint8_t>(c, px, out_status);
  if (d->blend)
    inpaint_blend_dev(c, d->frame[t % NF], d->mask1[t % NF], d->mask[t % NF], A, H, W, C, d->pitch, d->box[t % NF],
                      d->bopt, dout, dst);
  else
    inpaint_fill_dev(c, d->frame[t % NF], d->mask[t % NF], A, H, W, C, d->pitch, dout, dst, nullptr);
  download_dense(c, out, dout, px * C);
  download_dense(c, out_status, dst, px);
  HIPCHK(hipStreamSynchronize(c->stream));
}

}  // namespace

extern "C" {

int of_mask_grow(of_ctx *c, const uint8_t *a, const uint8_t *b, int H, int W, int g, uint8_t *out_mask,
                 float *out_weight) {
  API_BEGIN(c)
  REQUIRE(a && (out_mask || out_weight), OF_EINVAL, "bad arguments");
  REQUIRE(g >= 0 && g <= INP_MAX_G, OF_EINVAL, "g must be 0..24");
  check_frame(H, W, "video inpainting");
  const size_t px = (size_t)H * W;
  const uint8_t *da = upload_dense(c, a, px), *db = upload_dense(c, b, px);
  uint8_t *dm = new_dense<uint8_t>(c, px, out_mask);
  float *dw = new_dense<float>(c, px, out_weight);
  mask_grow_dev(c, da, db, H, W, g, dm, dw, W);
  download_dense(c, out_mask, dm, px);
  download_dense(c, out_weight, dw, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_inpaint_fill(of_ctx *c, const float *frames, const uint8_t *masks, const float *fw, const float *bw, int T,
                    int H, int W, int C, int t, const of_inpaint_opts *o, float *out, uint8_t *out_status,
                    uint8_t *out_hops) {
  API_BEGIN(c)
  REQUIRE(frames && masks && out && T >= 1 && t >= 0 && t < T && (T == 1 || (fw && bw)), OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= INP_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_inpaint_opts(o);
  check_frame(H, W, "video inpainting");
  const size_t px = (size_t)H * W;
  const int R = o->radius, lo = t - R > 0 ? t - R : 0, hi = t + R < T - 1 ? t + R : T - 1, n = hi - lo + 1;
  // the frames within reach, their grown masks, the forward flows from t on and the backward flows before it
  const float *dfr = upload_dense(c, frames + (size_t)lo * px * C, px * C * n);
  const uint8_t *draw = upload_dense(c, masks + (size_t)lo * px, px * n);
  uint8_t *dgr = new_dense<uint8_t>(c, px * n);
  for (int s = 0; s < n; ++s) mask_grow_dev(c, draw + (size_t)s * px, nullptr, H, W, o->grow, dgr + (size_t)s * px, nullptr, 0);
  std::vector<const float2 *> dfw(T, nullptr), dbw(T, nullptr);
  for (int s = t; s < hi; ++s) dfw[s] = upload_f2(c, fw + (size_t)s * 2 * px, H, W).p;
  for (int s = lo; s < t; ++s) dbw[s] = upload_f2(c, bw + (size_t)s * 2 * px, H, W).p;
  const InpaintArgs A = inpaint_hops(
      t, T, R, [&](int s) { return dfr + (size_t)(s - lo) * px * C; },
      [&](int s) { return (const uint8_t *)dgr + (size_t)(s - lo) * px; }, [&](int s) { return dfw[s]; },
      [&](int s) { return dbw[s]; });
  float *dout = new_dense<float>(c, px * C);
  uint8_t *dst = new_dense<uint8_t>(c, px, out_status), *dh = new_dense<uint8_t>(c, 2 * px, out_hops);
  inpaint_fill_dev(c, dfr + (size_t)(t - lo) * px * C, dgr + (size_t)(t - lo) * px, A, H, W, C, of_pitch(W), dout, dst,
                   dh);
  download_dense(c, out, dout, px * C);
  download_dense(c, out_status, dst, px);
  download_dense(c, out_hops, dh, 2 * px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_inpaint_blend(of_ctx *c, const float *frames, const uint8_t *masks, const float *fw, const float *bw, int T,
                     int H, int W, int C, int t, const of_inpaint_opts *o, const of_blend_opts *bo, float *out,
                     uint8_t *out_status) {
  API_BEGIN(c)
  REQUIRE(frames && masks && out && T >= 1 && t >= 0 && t < T && (T == 1 || (fw && bw)), OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= INP_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_inpaint_opts(o);
  check_blend_opts(bo);
  check_frame(H, W, "video inpainting");
  const size_t px = (size_t)H * W;
  const int R = o->radius, lo = t - R > 0 ? t - R : 0, hi = t + R < T - 1 ? t + R : T - 1, n = hi - lo + 1;
  const PsnBox box = psn_box(masks + (size_t)t * px, H, W, -1, o->grow);
  // as of_inpaint_fill, the masks grown by one more; and frame t's own grown mask
  const float *dfr = upload_dense(c, frames + (size_t)lo * px * C, px * C * n);
  const uint8_t *draw = upload_dense(c, masks + (size_t)lo * px, px * n);
  uint8_t *dgr = new_dense<uint8_t>(c, px * n), *dom = new_dense<uint8_t>(c, px);
  for (int s = 0; s < n; ++s)
    mask_grow_dev(c, draw + (size_t)s * px, nullptr, H, W, o->grow + 1, dgr + (size_t)s * px, nullptr, 0);
  mask_grow_dev(c, draw + (size_t)(t - lo) * px, nullptr, H, W, o->grow, dom, nullptr, 0);
  std::vector<const float2 *> dfw(T, nullptr), dbw(T, nullptr);
  for (int s = t; s < hi; ++s) dfw[s] = upload_f2(c, fw + (size_t)s * 2 * px, H, W).p;
  for (int s = lo; s < t; ++s) dbw[s] = upload_f2(c, bw + (size_t)s * 2 * px, H, W).p;
  const InpaintArgs A = inpaint_hops(
      t, T, R, [&](int s) { return dfr + (size_t)(s - lo) * px * C; },
      [&](int s) { return (const uint8_t *)dgr + (size_t)(s - lo) * px; }, [&](int s) { return dfw[s]; },
      [&](int s) { return dbw[s]; });
  float *dout = new_dense<float>(c, px * C);
  uint8_t *dst = new_dense<uint8_t>(c, px, out_status);
  inpaint_blend_dev(c, dfr + (size_t)(t - lo) * px * C, dgr + (size_t)(t - lo) * px, dom, A, H, W, C, of_pitch(W), box,
                    *bo, dout, dst);
  download_dense(c, out, dout, px * C);
  download_dense(c, out_status, dst, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_inpaint_set_blend(of_ctx *c, const of_blend_opts *bo) {
  if (!c) return OF_EINVAL;
  try {
    Inpainter *d = session_get<Inpainter>(c, SES_INPAINT);
    REQUIRE(d->frames == 0 && !d->flushed, OF_EINVAL,
            "the inpainter has taken a frame already (set the blending before the first push)");
    if (!bo) {
      d->blend = false;
      return OF_OK;
    }
    check_blend_opts(bo);
    HIPCHK(hipSetDevice(c->device));
    const int NF = 2 * d->opt.radius + 1;
    while ((int)d->mask1.size() < NF) d->mask1.push_back(d->alloc<uint8_t>((size_t)d->H * d->W));
    d->box.assign(NF, PsnBox());
    d->bopt = *bo;
    d->blend = true;
    return OF_OK;
  }
  API_CATCH(c)
}

int of_inpaint_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_inpaint_opts *o) {
  API_BEGIN(c)
  session_open<Inpainter>(c, SES_INPAINT, P, H, W, C, o, check_inpaint_opts, [&](Inpainter *d) {
    check_weight_params(P, true);  // every pair is a weighted estimate
    const int R = o->radius;
    d->pitch = of_pitch(W);
    d->alloc_frames(2 * R + 1);
    for (int k = 0; k < 2 * R + 1; ++k) d->mask.push_back(d->alloc<uint8_t>((size_t)H * W));
    for (int k = 0; k < 2 * R; ++k) {
      d->fw.push_back(d->alloc<float2>((size_t)H * d->pitch));
      d->bw.push_back(d->alloc<float2>((size_t)H * d->pitch));
    }
  });
  API_END(c)
}

int of_inpaint_push(of_ctx *c, const float *frame, const uint8_t *mask, float *out, uint8_t *out_status,
                    int32_t *out_index) {
  API_BEGIN(c)
  Inpainter *d = session_get<Inpainter>(c, SES_INPAINT);
  REQUIRE(frame && mask && out && out_index, OF_EINVAL, "bad arguments");
  session_not_flushed(d, SES_INPAINT);
  const int H = d->H, W = d->W, C = d->C, R = d->opt.radius, NF = 2 * R + 1, k = d->frames;
  const size_t px = (size_t)H * W;
  float *cur = d->frame[k % NF];
  HIPCHK(hipMemcpyAsync(cur, frame, sizeof(float) * px * C, hipMemcpyHostToDevice, c->stream));
  mask_grow_dev(c, upload_dense(c, mask, px), nullptr, H, W, d->opt.grow, d->mask[k % NF], nullptr, 0);
  if (d->blend) {  // square windows compose: the ring's mask grown by one more
    mask_grow_dev(c, d->mask[k % NF], nullptr, H, W, 1, d->mask1[k % NF], nullptr, 0);
    d->box[k % NF] = psn_box(mask, H, W, -1, d->opt.grow);
  }
  if (k > 0) {
    // the pair (previous, this): its weight, then both directions as two weighted estimates from zero flows
    const float *prev = d->frame[(k - 1) % NF];
    const Img wgt = new_img(c, H, W, 1);
    mask_grow_dev(c, d->mask[(k - 1) % NF], d->mask[k % NF], H, W, d->opt.margin, nullptr, wgt.p, wgt.P);
    const int p = (k - 1) % (2 * R);
    const size_t fb = sizeof(float2) * (size_t)H * d->pitch;  // new_f2's pitch is of_pitch(W), the ring's
    of_params Pf = d->P, Pb = d->P;
    const std::vector<size_t> mark = c->arena.mark();
    F2 uf = init_flow(c, nullptr, H, W);
    estimate_dev(c, &Pf, prev, cur, false, H, W, C, uf, nullptr, wgt);
    HIPCHK(hipMemcpyAsync(d->fw[p], uf.p, fb, hipMemcpyDeviceToDevice, c->stream));
    c->arena.rewind(mark);  // the second estimate reuses the first one's memory, in stream order
    F2 ub = init_flow(c, nullptr, H, W);
    estimate_dev(c, &Pb, cur, prev, false, H, W, C, ub, nullptr, wgt);
    HIPCHK(hipMemcpyAsync(d->bw[p], ub.p, fb, hipMemcpyDeviceToDevice, c->stream));
  }
  *out_index = -1;
  const int t = session_next_emit(d, R, false);
  if (t >= 0) {
    inpaint_emit(c, d, t, out, out_status);
    *out_index = t;
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));  // the caller's frame and mask have been read
  }
  API_END(c)
}

int of_inpaint_flush(of_ctx *c, float *out, uint8_t *out_status, int32_t *out_index) {
  API_BEGIN(c)
  Inpainter *d = session_get<Inpainter>(c, SES_INPAINT);
  REQUIRE(out && out_index, OF_EINVAL, "bad arguments");
  *out_index = -1;
  const int t = session_next_emit(d, d->opt.radius, true);
  if (t >= 0) {
    inpaint_emit(c, d, t, out, out_status);
    *out_index = t;
  }
  API_END(c)
}

int of_inpaint_close(of_ctx *c) { return session_close(c, SES_INPAINT); }

}  // extern "C"
