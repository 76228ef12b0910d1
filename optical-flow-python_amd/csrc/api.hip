// api.hip — the C entries (include/optflow.h) that are not batch calls:
// context create and destroy, options, profiling, the solve log, the
// single-pair calls, the stage entries of the parity tests and flow colour.
namespace {
// the caller's H x W data weight on the device, or p == nullptr without one;
// its values and what it cannot be combined with are checked on the host
// before anything is launched
Img upload_weight(of_ctx *c, const of_params *P, const float *weight, int H, int W) {
  if (!weight) return Img();
  REQUIRE(P && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  check_weight_values(weight, H, W);
  check_weight_params(P, true);
  return upload_new_img(c, weight, H, W, 1);
}
}  // namespace

extern "C" {

int of_abi_version(void) { return OF_ABI_VERSION; }

int of_device_count(int *count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (count) *count = n;
  return OF_OK;
}

int of_ctx_create(int device, of_ctx **out) {
  if (!out) return OF_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    g_err = "no HIP device";
    return OF_EHIP;
  }
  of_ctx *c = new of_ctx();
  c->device = device;
  try {
    HIPCHK(hipSetDevice(device));
    create_stream(&c->stream);
    HIPCHK(hipMalloc(&c->d_state, sizeof(PcgState)));
    HIPCHK(hipHostMalloc(&c->h_state, 2 * sizeof(PcgState), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(&c->h_flag, OF_SOLVE_RING * sizeof(CgFlag), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostMalloc(&c->h_ring, OF_SOLVE_RING * sizeof(PcgState), hipHostMallocDefault));
    HIPCHK(hipHostGetDevicePointer((void **)&c->d_flag, c->h_flag, 0));
    HIPCHK(hipEventCreateWithFlags(&c->ev_state[0], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_state[1], hipEventDisableTiming));
    HIPCHK(hipMalloc(&c->d_partials, sizeof(double) * 16 * PCG_MAX_BLOCKS));
    HIPCHK(hipMalloc(&c->d_sor_sync, OF_SOR_SYNC_BYTES));
    HIPCHK(hipMalloc(&c->d_rpart, sizeof(double) * 2 * PCG_MAX_BLOCKS));
    HIPCHK(hipMalloc(&c->d_rlog, sizeof(double) * 4 * OF_SLOG_MAX));
    HIPCHK(hipFuncSetAttribute((const void *)k_sor_lex, hipFuncAttributeMaxDynamicSharedMemorySize, OF_SOR_SHM));
    HIPCHK(hipFuncSetAttribute((const void *)k_sor_pipe, hipFuncAttributeMaxDynamicSharedMemorySize, OF_SOR_PIPE_SHM));
    HIPCHK(hipFuncSetAttribute((const void *)k_sor_wg, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(OF_SORW_RING_BYTES + sizeof(SorWgShared))));
    HIPCHK(hipMalloc(&c->d_mm, sizeof(uint32_t) * 64));
    HIPCHK(hipMalloc(&c->d_norm, sizeof(double)));
    HIPCHK(hipHostMalloc(&c->h_norm, sizeof(double), hipHostMallocDefault));
  } catch (const OfError &e) {
    g_err = e.msg;
    delete c;
    return e.code;
  }
  *out = c;
  return OF_OK;
}

int of_ctx_destroy(of_ctx *c) {
  if (!c) return OF_OK;
  if (c->pool) of_pairs_close(c);
  for (int k = 0; k < SES_KINDS; ++k) session_free(c, k);
  for (of_ctx *l : c->lanes) of_ctx_destroy(l);
  c->lanes.clear();
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  stage_free(c);
  if (c->comm) ncclCommDestroy(c->comm);
  c->arena.release();
  for (auto &s : c->slots) {
    hipFree(s.rgb1);
    hipFree(s.rgb2);
    hipFree(s.uv);
  }
  if (c->own_epoch && c->epoch) hipEventDestroy(c->epoch);
  for (auto e : c->ev_pool) hipEventDestroy(e);
  for (auto e : c->tev_pool) hipEventDestroy(e);
  for (auto e : c->ev_state)
    if (e) hipEventDestroy(e);
  hipFree(c->d_state);
  hipHostFree(c->h_state);
  if (c->h_flag) hipHostFree(c->h_flag);
  if (c->h_ring) hipHostFree(c->h_ring);
  hipFree(c->d_partials);
  hipFree(c->d_sor_sync);
  if (c->d_sorp) hipFree(c->d_sorp);
  if (c->d_sor_ring) hipFree(c->d_sor_ring);
  if (c->d_gather) hipFree(c->d_gather);
  if (c->gstream) {
    hipStreamSynchronize(c->gstream);
    hipStreamDestroy(c->gstream);
  }
  hipFree(c->d_rpart);
  hipFree(c->d_rlog);
  hipFree(c->d_mm);
  if (c->d_noise) hipFree(c->d_noise);
  hipFree(c->d_norm);
  hipHostFree(c->h_norm);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return OF_OK;
}

const char *of_last_error(of_ctx *c) { return c ? c->err.c_str() : g_err.c_str(); }

int of_synchronize(of_ctx *c) {
  if (!c) return OF_EINVAL;
  return hipStreamSynchronize(c->stream) == hipSuccess ? OF_OK : OF_EHIP;
}

// Settings and profiling tables the pool's lanes read (lane 0 is the context
// itself) are refused while a pair stream is open: changing them under a
// running lane would give its pairs other arithmetic than the lanes that
// copied them at of_pairs_open, or race the lane's own writes.
#define REFUSE_WHILE_POOL(c)                                                          \
  if ((c)->pool) {                                                                   \
    (c)->err = "a pair stream is open on this context (of_pairs_close first)";       \
    return OF_EINVAL;                                                                \
  }

int of_set_option(of_ctx *c, int option, int value) {
  if (!c) return OF_EINVAL;
  REFUSE_WHILE_POOL(c)
  switch (option) {
    case OF_OPT_SOR_PIPELINE:
      c->opt_sor_pipe = value < 0 ? 0 : (value > 2 ? 2 : value);
      return OF_OK;
    case OF_OPT_FUSED_WARP:
      c->opt_fused_warp = value ? 1 : 0;
      return OF_OK;
    default:
      c->err = "unknown option";
      return OF_EINVAL;
  }
}

int of_set_progress(of_ctx *c, of_progress_fn fn, void *user, int flags) {
  if (!c) return OF_EINVAL;
  if (c->pool) pool_set_progress(c->pool, fn);  // takes effect when the pair stream closes
  else c->prog_fn = fn;
  c->prog_user = user;
  c->prog_flags = flags;
  return OF_OK;
}

int of_get_option(of_ctx *c, int option, int64_t *value) {
  if (!c || !value) return OF_EINVAL;
  switch (option) {
    case OF_OPT_SOR_PIPELINE:
      *value = c->opt_sor_pipe;
      return OF_OK;
    case OF_OPT_FUSED_WARP:
      *value = c->opt_fused_warp;
      return OF_OK;
    case OF_OPT_SOR_FALLBACKS: {
      int64_t n = c->sor_fallbacks;
      for (of_ctx *l : c->lanes) n += l->sor_fallbacks;
      *value = n;
      return OF_OK;
    }
    case OF_OPT_DEVICE_BYTES: {
      // grow-only device buffers of the context and its lanes: the arena
      // chunks, the pipelined SOR's sweep ring and the RCCL gather buffer;
      // and the open sessions' (point tracker, temporal denoiser, stabiliser, super-resolver, inpainter, mask propagator, temporal consistency) buffers
      auto held = [](const of_ctx *x) {
        return (int64_t)(x->arena.reserved() + x->sor_ring_cap + x->gather_cap);
      };
      int64_t n = held(c);
      for (of_ctx *l : c->lanes) n += held(l);
      for (const Session *s : c->session)
        if (s) n += (int64_t)s->bytes;
      *value = n;
      return OF_OK;
    }
    case OF_OPT_RCCL_NRANKS: {
      // ranks of the context's RCCL communicator as RCCL reports them (0: none)
      int n = 0;
      if (c->comm && ncclCommCount(c->comm, &n) != ncclSuccess) n = -1;
      *value = n;
      return OF_OK;
    }
    default:
      c->err = "unknown option";
      return OF_EINVAL;
  }
}

int of_set_profiling(of_ctx *c, int enable) {
  if (!c) return OF_EINVAL;
  REFUSE_WHILE_POOL(c)
  try {
    flush_prof(c);
  } catch (const OfError &e) {
    return fail(c, e);
  }
  c->prof = enable < 0 ? 0 : (enable > 3 ? 3 : enable);
  if (enable) {
    c->ktimes.clear();
    c->tl.clear();
  }
  if (c->prof == 3) {
    if (!c->epoch) {
      if (hipEventCreate(&c->epoch) != hipSuccess) return OF_EHIP;
      c->own_epoch = true;
    }
    if (hipEventRecord(c->epoch, c->stream) != hipSuccess) return OF_EHIP;
  }
  return OF_OK;
}

int of_kernel_times(of_ctx *c, int max, const char **names, double *ms, int64_t *count, double *pixels, int *n) {
  if (!c || !n) return OF_EINVAL;
  REFUSE_WHILE_POOL(c)
  int k = 0;
  for (auto &kv : c->ktimes) {
    if (k < max) {
      if (names) names[k] = kv.first.c_str();
      if (ms) ms[k] = kv.second.ms;
      if (count) count[k] = kv.second.n;
      if (pixels) pixels[k] = kv.second.px;
    }
    ++k;
  }
  *n = k;
  return OF_OK;
}

int of_kernel_timeline(of_ctx *c, int max, const char **names, double *pixels, double *t0_ms, double *t1_ms,
                       int *n) {
  if (!c || !n) return OF_EINVAL;
  REFUSE_WHILE_POOL(c)
  const int m = (int)c->tl.size();
  for (int k = 0; k < m && k < max; ++k) {
    if (names) names[k] = c->tl[k].name;
    if (pixels) pixels[k] = c->tl[k].px;
    if (t0_ms) t0_ms[k] = c->tl[k].t0;
    if (t1_ms) t1_ms[k] = c->tl[k].t1;
  }
  *n = m;
  return OF_OK;
}

int of_set_solve_log(of_ctx *c, int enable) {
  if (!c) return OF_EINVAL;
  REFUSE_WHILE_POOL(c)
  c->slog = enable ? 1 : 0;
  c->slog_rec.clear();
  return OF_OK;
}

int of_solve_log(of_ctx *c, int max, of_solve_record *out, int *n) {
  API_BEGIN(c)
  REQUIRE(n && (out || max <= 0), OF_EINVAL, "bad arguments");
  HIPCHK(hipStreamSynchronize(c->stream));
  drain_solves(c);
  const int m = (int)c->slog_rec.size();
  *n = m;
  const int k = std::min(m, max);
  if (k > 0) {
    std::vector<double> h(4 * (size_t)k);
    HIPCHK(hipMemcpy(h.data(), c->d_rlog, sizeof(double) * 4 * k, hipMemcpyDeviceToHost));
    for (int e = 0; e < k; ++e) {
      const auto &l = c->slog_rec[e];
      of_solve_record &o = out[e];
      memset(&o, 0, sizeof(o));
      o.h = l.h;
      o.w = l.w;
      o.solver = l.solver;
      o.iters = l.iters;
      o.done = l.done;
      o.true_rel = h[4 * e + 1] > 0 ? std::sqrt(h[4 * e] / h[4 * e + 1]) : 0.0;
      o.true_rel_out = h[4 * e + 3] > 0 ? std::sqrt(h[4 * e + 2] / h[4 * e + 3]) : 0.0;
      o.est_rel = l.est;
    }
  }
  API_END(c)
}

int of_solver_geometry(int H, int W, int solver, of_cg_geometry *out) {
  if (!out || solver < 0 || solver > 2) return OF_EINVAL;
  memset(out, 0, sizeof(*out));
  if (solver == OF_SOLVER_SOR) {
    if (H < 1 || W < 1) return OF_EINVAL;
    const int ns = (H + 63) / 64;
    out->grid_x = 2 * ns;
    out->grid_y = 1;
    out->rows = 64;
    out->bands = ns;
    out->blocks = 2 * ns;
    out->strip_cols = W;
    return ns <= SOR_MAXS ? OF_OK : OF_ENOTSUP;
  }
  return cg_geometry(H, W, solver == OF_SOLVER_BACKSLASH, out);
}

// The *_weighted entries carry their unweighted siblings' bodies: a NULL
// weight uploads nothing and launches the unweighted kernels.
int of_estimate_flow_weighted(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                              const float *init_uv, const float *weight, float *out_uv, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out_uv && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  const Img wgt = upload_weight(c, P, weight, H, W);
  if (st) memset(st, 0, sizeof(*st));
  const WallClock wall;
  float *d1, *d2;
  upload_frames(c, im1, im2, (size_t)H * W * C, &d1, &d2);
  F2 uv = init_flow(c, init_uv, H, W);
  estimate_dev(c, P, d1, d2, false, H, W, C, uv, st, wgt);
  download_f2(c, uv, out_uv);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) st->total_ms = wall.ms();
  API_END(c)
}

int of_estimate_flow(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                     const float *init_uv, float *out_uv, of_stats *st) {
  return of_estimate_flow_weighted(c, P, im1, im2, H, W, C, init_uv, nullptr, out_uv, st);
}

int of_compute_flow_weighted(of_ctx *c, of_params *P, const float *images, int H, int W, int nc, const float *guide,
                             int gc, const float *init_uv, const float *weight, float *out_uv, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(P && images && out_uv && H > 0 && W > 0 && nc >= 1, OF_EINVAL, "bad arguments");
  const Img wgt = upload_weight(c, P, weight, H, W);
  if (st) memset(st, 0, sizeof(*st));
  const WallClock wall;
  Img im = upload_new_img(c, images, H, W, 2 * nc);
  Img g;
  if (guide && gc > 0) g = upload_new_img(c, guide, H, W, gc);
  F2 uv = init_flow(c, init_uv, H, W);
  compute_flow_dev(c, P, im, g, uv, st, wgt);
  download_f2(c, uv, out_uv);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) st->total_ms = wall.ms();
  API_END(c)
}

int of_compute_flow(of_ctx *c, of_params *P, const float *images, int H, int W, int nc, const float *guide, int gc,
                    const float *init_uv, float *out_uv, of_stats *st) {
  return of_compute_flow_weighted(c, P, images, H, W, nc, guide, gc, init_uv, nullptr, out_uv, st);
}

int of_fb_consistency(of_ctx *c, const float *fw, const float *bw, int H, int W, double alpha1, double alpha2,
                      uint8_t *state, float *err) {
  API_BEGIN(c)
  REQUIRE(fw && bw && state && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  check_alphas(alpha1, alpha2);
  const size_t n = (size_t)H * W;
  F2 f = upload_f2(c, fw, H, W), b = upload_f2(c, bw, H, W);
  uint8_t *ds = new_dense<uint8_t>(c, n);
  float *de = new_dense<float>(c, n, err);
  fb_check(c, f, b, alpha1, alpha2, ds, de, nullptr, nullptr);
  download_dense(c, state, ds, n);
  download_dense(c, err, de, n);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_estimate_flow_bidir(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                           const float *init_fw, const float *init_bw, float *out_fw, float *out_bw, double alpha1,
                           double alpha2, uint8_t *state_fw, uint8_t *state_bw, of_stats *sf, of_stats *sb) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out_fw && out_bw && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  check_alphas(alpha1, alpha2);
  if (sf) memset(sf, 0, sizeof(*sf));
  if (sb) memset(sb, 0, sizeof(*sb));
  const WallClock wall;  // the forward pass's total_ms; the backward pass has its own
  const size_t px = (size_t)H * W;
  float *d1, *d2;
  upload_frames(c, im1, im2, px * C, &d1, &d2);
  F2 uf = init_flow(c, init_fw, H, W), ub = init_flow(c, init_bw, H, W);
  uint8_t *dsf = new_dense<uint8_t>(c, px, state_fw), *dsb = new_dense<uint8_t>(c, px, state_bw);
  estimate_bidir_dev(c, P, d1, d2, H, W, C, uf, ub, alpha1, alpha2, dsf, dsb, sf, sb);
  download_f2(c, uf, out_fw);
  download_f2(c, ub, out_bw);
  download_dense(c, state_fw, dsf, px);
  download_dense(c, state_bw, dsb, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (sf) sf->total_ms = wall.ms();
  API_END(c)
}

int of_warp_image(of_ctx *c, const float *im, int H, int W, int C, const float *uv, float *out, uint8_t *valid) {
  API_BEGIN(c)
  REQUIRE(im && uv && out && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= OF_MAX_NC, OF_EINVAL, "images must have 1 to 4 channels");
  const size_t px = (size_t)H * W;
  float *dim = upload_dense(c, im, px * C);
  F2 f = upload_f2(c, uv, H, W);
  float *dout = new_dense<float>(c, px * C);
  uint8_t *dv = new_dense<uint8_t>(c, px, valid);
  c->cur_px = (double)px;
  Grid2 g = grid2(H, W);
  launch(c, "warp_image", k_warp_image, g.grid, g.block, 0, (const float *)dim, C, (const float2 *)f.p, H, W, f.P,
         dout, dv);
  download_dense(c, out, dout, px * C);
  download_dense(c, valid, dv, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_interp_frames(of_ctx *c, const float *im1, const float *im2, int H, int W, int C, const float *fw,
                     const float *bw, double alpha1, double alpha2, int n, const double *t, float *out,
                     float *out_ut, uint8_t *out_info) {
  API_BEGIN(c)
  REQUIRE(im1 && im2 && fw && bw && out && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= OF_MAX_NC, OF_EINVAL, "images must have 1 to 4 channels");
  check_interp_args(H, W, alpha1, alpha2, n, t);
  const size_t px = (size_t)H * W;
  float *d1, *d2;
  upload_frames(c, im1, im2, px * C, &d1, &d2);
  F2 f = upload_f2(c, fw, H, W), b = upload_f2(c, bw, H, W);
  uint8_t *dsf = (uint8_t *)c->arena.alloc(px), *dsb = (uint8_t *)c->arena.alloc(px);
  fb_check(c, f, b, alpha1, alpha2, dsf, nullptr, dsb, nullptr);
  interp_frames_dev(c, d1, d2, H, W, C, f, b, dsf, dsb, n, t, out, out_ut, out_info);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_estimate_interp(of_ctx *c, of_params *P, const float *im1, const float *im2, int H, int W, int C,
                       double alpha1, double alpha2, int n, const double *t, float *out, float *out_fw,
                       float *out_bw, uint8_t *out_info, of_stats *sf, of_stats *sb) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out && H > 0 && W > 0, OF_EINVAL, "bad arguments");
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "images must be (H,W) or (H,W,3)");
  check_interp_args(H, W, alpha1, alpha2, n, t);
  if (sf) memset(sf, 0, sizeof(*sf));
  if (sb) memset(sb, 0, sizeof(*sb));
  const WallClock wall;
  const size_t px = (size_t)H * W;
  float *d1, *d2;
  upload_frames(c, im1, im2, px * C, &d1, &d2);
  F2 uf = init_flow(c, nullptr, H, W), ub = init_flow(c, nullptr, H, W);
  uint8_t *dsf = (uint8_t *)c->arena.alloc(px), *dsb = (uint8_t *)c->arena.alloc(px);
  estimate_bidir_dev(c, P, d1, d2, H, W, C, uf, ub, alpha1, alpha2, dsf, dsb, sf, sb);
  interp_frames_dev(c, d1, d2, H, W, C, uf, ub, dsf, dsb, n, t, out, nullptr, out_info);
  if (out_fw) download_f2(c, uf, out_fw);
  if (out_bw) download_f2(c, ub, out_bw);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (sf) sf->total_ms = wall.ms();
  API_END(c)
}

int of_compute_flow_base_weighted(of_ctx *c, of_params *P, const float *images, int H, int W, int nc,
                                  const float *guide, int gc, double alpha, const float *uv_in, const float *weight,
                                  float *out_uv) {
  API_BEGIN(c)
  REQUIRE(P && images && uv_in && out_uv, OF_EINVAL, "bad arguments");
  check_params(P);
  LevelIn L;
  L.wgt = upload_weight(c, P, weight, H, W);
  L.im = upload_new_img(c, images, H, W, 2 * nc);
  if (guide && gc > 0 && P->method == OF_METHOD_CLASSIC_NL) L.guide = upload_new_img(c, guide, H, W, gc);
  F2 uv = upload_f2(c, uv_in, H, W);
  c->prog_stage = 0;
  c->prog_level = -1;
  if (P->method == OF_METHOD_HS) hs_base(c, P, L, uv, nullptr);
  else if (P->method == OF_METHOD_ALT_BA) throw OfError{OF_ENOTSUP, "AltBA compute_flow_base needs uvhat"};
  else irls_base(c, P, L, uv, alpha, P->max_linear, nullptr);
  download_f2(c, uv, out_uv);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_compute_flow_base(of_ctx *c, of_params *P, const float *images, int H, int W, int nc, const float *guide,
                         int gc, double alpha, const float *uv_in, float *out_uv) {
  return of_compute_flow_base_weighted(c, P, images, H, W, nc, guide, gc, alpha, uv_in, nullptr, out_uv);
}

// AltBAOpticalFlow.compute_flow_base(uv, uvhat) (alt_ba.py:189-274): one
// pyramid level of the coupled IRLS with lambda2 annealing and the Li-Osher
// median update of uvhat; returns both fields
int of_alt_ba_flow_base(of_ctx *c, of_params *P, const float *images, int H, int W, int nc, double alpha,
                        int replacement, const float *uv_in, const float *uvhat_in, float *out_uv,
                        float *out_uvhat) {
  API_BEGIN(c)
  REQUIRE(P && images && uv_in && uvhat_in && out_uv && out_uvhat && H > 0 && W > 0 && nc >= 1, OF_EINVAL,
          "bad arguments");
  REQUIRE(P->method == OF_METHOD_ALT_BA, OF_EINVAL, "of_alt_ba_flow_base needs an AltBA parameter set");
  check_params(P);
  LevelIn L;
  L.im = upload_new_img(c, images, H, W, 2 * nc);
  F2 uv = upload_f2(c, uv_in, H, W), uvhat = upload_f2(c, uvhat_in, H, W);
  altba_base(c, P, L, uv, uvhat, alpha, replacement != 0, nullptr);
  download_f2(c, uv, out_uv);
  download_f2(c, uvhat, out_uvhat);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

// ---- stage entries ----
int of_preprocess(of_ctx *c, const float *rgb1, const float *rgb2, int H, int W, float *gray_pair, float *lab) {
  API_BEGIN(c)
  REQUIRE(rgb1 && rgb2 && gray_pair, OF_EINVAL, "bad arguments");
  float *d1, *d2;
  upload_frames(c, rgb1, rgb2, (size_t)H * W * 3, &d1, &d2);
  Img gray = new_img(c, H, W, 2), g3 = new_img(c, H, W, 3);
  rgb_prep(c, (const float *)d1, (const float *)d2, H, W, 3, gray, g3);
  download_img(c, gray, gray_pair);
  if (lab) download_img(c, g3, lab);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_rof_texture(of_ctx *c, const float *im, int H, int W, int C, double theta, int iters, double alp, float *out) {
  API_BEGIN(c)
  REQUIRE(im && out && C >= 1, OF_EINVAL, "bad arguments");
  Img m = upload_new_img(c, im, H, W, C);
  Img t = rof_texture(c, m, theta, iters, alp);
  download_img(c, t, out);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_pyramid_level(of_ctx *c, const float *im, int H, int W, int C, const double *kern, int ksize, double ratio,
                     float *out, int *outH, int *outW) {
  API_BEGIN(c)
  REQUIRE(im && out && kern && ksize >= 1 && ksize <= 5 && (ksize & 1), OF_EINVAL, "bad arguments");
  Img m = upload_new_img(c, im, H, W, C);
  Img o = pyramid_step(c, m, make_taps(kern, ksize, ksize), ratio);
  download_img(c, o, out);
  if (outH) *outH = o.H;
  if (outW) *outW = o.W;
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_resample_flow(of_ctx *c, const float *uv, int H, int W, int nH, int nW, float *out) {
  API_BEGIN(c)
  REQUIRE(uv && out, OF_EINVAL, "bad arguments");
  F2 a = upload_f2(c, uv, H, W);
  if (H == nH && W == nW) {
    download_f2(c, a, out);
  } else {
    F2 b = new_f2(c, nH, nW);
    resample_f2(c, a, b);
    download_f2(c, b, out);
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_partial_deriv(of_ctx *c, const float *images, int H, int W, int nc, const float *uv, int interp,
                     const double *filt, double blend, float *It, float *Ix, float *Iy) {
  API_BEGIN(c)
  REQUIRE(images && uv && filt && It && Ix && Iy && nc >= 1 && nc <= OF_MAX_NC, OF_EINVAL, "bad arguments");
  REQUIRE(interp >= 0 && interp <= 2, OF_EINVAL, "Unknown interpolation method");
  Img im = upload_new_img(c, images, H, W, 2 * nc);
  F2 f = upload_f2(c, uv, H, W);
  LevelDeriv D = level_deriv(c, im, nc, interp, filt, blend);
  Img a = new_img(c, H, W, nc), b = new_img(c, H, W, nc), d = new_img(c, H, W, nc);
  partial_deriv(c, D, interp, f, a, b, d);
  download_img(c, a, It);
  download_img(c, b, Ix);
  download_img(c, d, Iy);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_flow_operator_weighted(of_ctx *c, const of_params *P, double alpha, const float *uv, const float *duv,
                              const float *weight, const float *It, const float *Ix, const float *Iy, int H, int W,
                              int nc, float *coef, float *rhs) {
  API_BEGIN(c)
  REQUIRE(P && uv && It && Ix && Iy && coef && rhs && nc >= 1, OF_EINVAL, "bad arguments");
  const Img wgt = upload_weight(c, P, weight, H, W);
  F2 f = upload_f2(c, uv, H, W);
  F2 df;
  if (duv) df = upload_f2(c, duv, H, W);
  Img a = upload_new_img(c, It, H, W, nc), b = upload_new_img(c, Ix, H, W, nc), d = upload_new_img(c, Iy, H, W, nc);
  Img cf = new_img(c, H, W, 7);
  F2 r = new_f2(c, H, W);
  flow_operator(c, op_args(P, alpha, 0.0), f, duv ? &df : nullptr, a, b, d, nullptr, cf, r, wgt);
  download_img(c, cf, coef);
  download_f2(c, r, rhs);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_flow_operator(of_ctx *c, const of_params *P, double alpha, const float *uv, const float *duv, const float *It,
                     const float *Ix, const float *Iy, int H, int W, int nc, float *coef, float *rhs) {
  return of_flow_operator_weighted(c, P, alpha, uv, duv, nullptr, It, Ix, Iy, H, W, nc, coef, rhs);
}

int of_solve(of_ctx *c, const of_params *P, const float *coef, const float *rhs, int H, int W, float *x, int *iters,
             double *rel_residual) {
  API_BEGIN(c)
  REQUIRE(P && coef && rhs && x, OF_EINVAL, "bad arguments");
  check_params(P);
  Img cf = upload_new_img(c, coef, H, W, 7);
  F2 b = upload_f2(c, rhs, H, W), xx = new_f2(c, H, W);
  SolveResult r = solve(c, P, cf, b, xx);
  download_f2(c, xx, x);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (r.slot >= 0) {
    if (r.name) note_active(c, r.name, resolved(c, r.slot).iters + 1, r.px);
    r = resolved(c, r.slot);
  }
  if (iters) *iters = r.iters;
  if (rel_residual) *rel_residual = r.rel;
  API_END(c)
}

int of_flow_operator_dia(of_ctx *c, const of_params *P, double alpha, const float *uv, const float *duv,
                         const float *It, const float *Ix, const float *Iy, int H, int W, int nc, int *D_out,
                         float *planes, float *rhs) {
  API_BEGIN(c)
  REQUIRE(P && uv && It && Ix && Iy && planes && rhs && nc >= 1, OF_EINVAL, "bad arguments");
  REQUIRE(P->filters.general, OF_EINVAL, "of_flow_operator_dia needs params->filters.general");
  check_params(P);
  F2 f = upload_f2(c, uv, H, W);
  F2 df;
  if (duv) df = upload_f2(c, duv, H, W);
  Img a = upload_new_img(c, It, H, W, nc), b = upload_new_img(c, Ix, H, W, nc), d = upload_new_img(c, Iy, H, W, nc);
  GenLevel L = gen_level(c, P, H, W);
  F2 r = new_f2(c, H, W);
  gen_flow_operator(c, P, op_args(P, alpha, 0.0), f, duv ? &df : nullptr, a, b, d, nullptr, L, r);
  download_img(c, L.pl, planes);
  download_f2(c, r, rhs);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (D_out) *D_out = L.D;
  API_END(c)
}
int of_solve_dia(of_ctx *c, const of_params *P, int D, const float *planes, const float *rhs, int H, int W, float *x,
                 int *iters, double *rel_residual) {
  API_BEGIN(c)
  REQUIRE(P && planes && rhs && x && D >= 0 && D <= GEN_MAXD, OF_EINVAL, "bad arguments");
  check_params(P);
  GenLevel L = gen_solver_level(c, D, H, W);
  upload_img(c, L.pl, planes);
  F2 b = upload_f2(c, rhs, H, W), xx = new_f2(c, H, W);
  const SolveResult r = gen_solve_logged(c, P, L, b, xx);
  download_f2(c, xx, x);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (iters) *iters = r.iters;
  if (rel_residual) *rel_residual = r.rel;
  API_END(c)
}
int of_detect_occlusion(of_ctx *c, const float *uv, const float *images, int H, int W, int nc, float *occ) {
  API_BEGIN(c)
  REQUIRE(uv && images && occ && nc >= 1, OF_EINVAL, "bad arguments");
  F2 f = upload_f2(c, uv, H, W), z = new_f2(c, H, W), u1 = new_f2(c, H, W);
  fill_f2(c, z, 0.0f);
  Img im = upload_new_img(c, images, H, W, 2 * nc);
  Img o = new_img(c, H, W, 1);
  Grid2 g = grid2(H, W);
  launch(c, "update_occ", k_update_occ, g.grid, g.block, 0, (const float2 *)f.p, (const float2 *)z.p, 0, u1.p,
         (const float *)im.p, (const float *)im.plane(nc), nc, o.p, H, W, f.P, im.ps());
  download_img(c, o, occ);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_weighted_median_base(of_ctx *c, const float *uv, const float *guide, int gc, const float *occ, int H, int W,
                            int area_hsz, double sigma_i, const float *base, float *out) {
  API_BEGIN(c)
  REQUIRE(uv && guide && occ && out && gc >= 1, OF_EINVAL, "bad arguments");
  F2 f = upload_f2(c, uv, H, W), o;
  Img g = upload_new_img(c, guide, H, W, gc), oc = upload_new_img(c, occ, H, W, 1);
  // with a base the store goes to the base's own buffer, as irls_base has it
  if (base) o = upload_f2(c, base, H, W);
  else o = new_f2(c, H, W);
  wmf(c, f, g, oc.p, o, area_hsz, sigma_i, base ? (const float2 *)o.p : nullptr);
  download_f2(c, o, out);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_weighted_median(of_ctx *c, const float *uv, const float *guide, int gc, const float *occ, int H, int W,
                       int area_hsz, double sigma_i, float *out) {
  return of_weighted_median_base(c, uv, guide, gc, occ, H, W, area_hsz, sigma_i, nullptr, out);
}

// level_deriv + warp_operator, as hs_base / irls_base run them on a level
int of_warp_operator(of_ctx *c, const of_params *P, double alpha, const float *images, int H, int W, int nc,
                     const float *uv, const float *weight, double blend, float *coef, float *rhs) {
  API_BEGIN(c)
  REQUIRE(P && images && uv && coef && rhs && nc >= 1 && nc <= OF_MAX_NC, OF_EINVAL, "bad arguments");
  REQUIRE(P->interp >= 0 && P->interp <= 2, OF_EINVAL, "Unknown interpolation method");
  const OpArgs o = op_args(P, alpha, 0.0);
  REQUIRE(can_fuse_warp_op(c, o, nc), OF_ENOTSUP,
          "the fused warp + assembly takes 1 or 3 channels, not AltBA, with OF_OPT_FUSED_WARP on");
  const Img wgt = upload_weight(c, P, weight, H, W);
  Img im = upload_new_img(c, images, H, W, 2 * nc);
  F2 f = upload_f2(c, uv, H, W);
  c->cur_px = (double)H * W;
  LevelDeriv D = level_deriv(c, im, nc, P->interp, P->deriv_filter, blend);
  Img cf = new_img(c, H, W, 7);
  F2 r = new_f2(c, H, W);
  warp_operator(c, D, P->interp, o, f, cf, r, wgt);
  download_img(c, cf, coef);
  download_f2(c, r, rhs);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

// k_update_occ as irls_base launches it: out_uv1 = uv + clip(x) and, with
// out_occ, detect_occlusion of that field
int of_flow_update(of_ctx *c, const float *uv, const float *x, int clip, const float *images, int H, int W, int nc,
                   float *out_uv1, float *out_occ) {
  API_BEGIN(c)
  REQUIRE(uv && x && out_uv1 && (!out_occ || (images && nc >= 1 && nc <= OF_MAX_NC)), OF_EINVAL, "bad arguments");
  F2 f = upload_f2(c, uv, H, W), dx = upload_f2(c, x, H, W), u1 = new_f2(c, H, W);
  Img im, o;
  if (images) im = upload_new_img(c, images, H, W, 2 * nc);
  if (out_occ) o = new_img(c, H, W, 1);
  c->cur_px = (double)H * W;
  Grid2 g = grid2(H, W);
  launch(c, out_occ ? "update_occ" : "update", k_update_occ, g.grid, g.block, 0, (const float2 *)f.p,
         (const float2 *)dx.p, clip ? 1 : 0, u1.p, (const float *)im.p,
         (const float *)(images ? im.plane(nc) : nullptr), nc, o.p, H, W, f.P, images ? im.ps() : (size_t)0);
  download_f2(c, u1, out_uv1);
  if (out_occ) download_img(c, o, out_occ);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

// median2(): the float2 median of hs_base / irls_base (k_median2<size>)
int of_median_filter_flow(of_ctx *c, const float *uv, int H, int W, int size, float *out) {
  API_BEGIN(c)
  REQUIRE(uv && out, OF_EINVAL, "bad arguments");
  F2 f = upload_f2(c, uv, H, W), o = new_f2(c, H, W);
  c->cur_px = (double)H * W;
  median2(c, f, o, size);
  download_f2(c, o, out);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

// flow_to_color (viz/flow_color.py:77-107): the wheel of make_colorwheel
// (flow_color.py:5-40) built on the host, the radius reduction and the
// per-pixel map on the device (k_flow_rad_max, k_flow_color)
}  // extern "C"
namespace {
ColorWheel color_wheel() {
  ColorWheel cw{};
  const int n[6] = {15, 6, 4, 11, 13, 6};
  // per segment: the channel held at 255, the ramped channel and whether it ramps down
  const int hold[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2};
  int k = 0;
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < n[s]; ++i, ++k) {
      const double r = std::floor(255.0 * i / n[s]);  // np.floor(255 * np.arange(n) / n)
      cw.w[3 * k + hold[s]] = 255;
      cw.w[3 * k + ramp[s]] = (unsigned char)(s % 2 ? 255.0 - r : r);
    }
  return cw;
}
template <typename T>
void flow_color_dev(of_ctx *c, const void *flow, long n, double fixed, uint8_t *out) {
  using U = typename OrdBits<T>::U;
  T *d = (T *)c->arena.alloc(sizeof(T) * 2 * n);
  U *mx = (U *)c->arena.alloc(sizeof(U));
  unsigned char *o = (unsigned char *)c->arena.alloc(3 * n);
  HIPCHK(hipMemcpyAsync(d, flow, sizeof(T) * 2 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(mx, 0, sizeof(U), c->stream));
  const int blocks = (int)std::min<long>((n + 255) / 256, 2048);
  c->cur_px = (double)n;
  if (fixed <= 0) launch(c, "flow_rad_max", k_flow_rad_max<T>, dim3(blocks), dim3(256), 0, (const T *)d, n, mx);
  launch(c, "flow_color", k_flow_color<T>, dim3(blocks), dim3(256), 0, (const T *)d, n, (const U *)mx, fixed,
         color_wheel(), o);
  HIPCHK(hipMemcpyAsync(out, o, 3 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
}
}  // namespace
extern "C" {

int of_flow_to_color(of_ctx *c, const void *flow, int dtype, int H, int W, int has_max, double max_flow,
                     uint8_t *out_rgb) {
  API_BEGIN(c)
  REQUIRE(H >= 0 && W >= 0 && (dtype == 0 || dtype == 1) && (H * (long)W == 0 || (flow && out_rgb)), OF_EINVAL,
          "bad arguments");
  const long n = (long)H * W;
  // max_rad = max(max_flow, 1e-8) (flow_color.py:100): > 0 selects the fixed value
  const double fixed = has_max ? (max_flow > 1e-8 ? max_flow : 1e-8) : 0.0;
  if (n > 0) {
    if (dtype == 0) flow_color_dev<float>(c, flow, n, fixed, out_rgb);
    else flow_color_dev<double>(c, flow, n, fixed, out_rgb);
  }
  API_END(c)
}

int of_median_filter(of_ctx *c, const float *in, int H, int W, int planes, int size, float *out) {
  API_BEGIN(c)
  REQUIRE(in && out && planes >= 1, OF_EINVAL, "bad arguments");
  REQUIRE(size == 3 || size == 5 || size == 7, OF_ENOTSUP, "median size must be 3, 5 or 7");
  Img a = upload_new_img(c, in, H, W, planes), b = new_img(c, H, W, planes);
  Grid2 g = grid2(H, W);
  auto go = [&](auto k) {
    launch(c, "median1", k, gz(g, planes), g.block, 0, (const float *)a.p, b.p, H, W, a.P, a.ps());
  };
  if (size == 3) go(k_median1<3>);
  else if (size == 5) go(k_median1<5>);
  else go(k_median1<7>);
  download_img(c, b, out);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

}  // extern "C"

#ifdef CGS_PHASE_TIMING
// instrumented builds only (tools/micro): read and clear the k_cgs role timers
extern "C" int of_debug_cgs_times(unsigned long long *out12) {
  if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_cgs_t), sizeof(unsigned long long) * 12) != hipSuccess) return OF_EHIP;
  unsigned long long z[12] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_cgs_t), z, sizeof(z)) != hipSuccess) return OF_EHIP;
  return OF_OK;
}
#endif
