// host_fuse.hip — host side of the temporal denoising (kernels_fuse.hip):
// option checks, flow composition and frame fusion on device-resident frames,
// flows and states, the two stage entries on host buffers and the per-context
// denoiser session.
namespace {

void check_fuse_opts(const of_fuse_opts *o) {
  REQUIRE(o, OF_EINVAL, "no fuse options");
  REQUIRE(o->radius >= 1 && o->radius <= 2, OF_EINVAL, "fuse radius must be 1..2");
  REQUIRE(o->patch >= 0 && o->patch <= FUSE_MAX_R, OF_EINVAL, "fuse patch must be 0..3");
  REQUIRE(std::isfinite(o->sigma) && o->sigma > 0 && std::isfinite(o->strength) && o->strength > 0, OF_EINVAL,
          "sigma and strength must be finite and > 0");
  REQUIRE(std::isfinite(o->alpha1) && std::isfinite(o->alpha2) && o->alpha1 >= 0 && o->alpha2 >= 0, OF_EINVAL,
          "alpha1 and alpha2 must be finite and >= 0");
}
void check_fuse_frame(int H, int W) {
  REQUIRE(H > 0 && W > 0, OF_EINVAL, "bad arguments");
  REQUIRE((size_t)H * W < ((size_t)1 << 31), OF_ENOTSUP, "temporal fusion takes H * W < 2^31");
}

// out = f followed by g, device-resident; sf / sg / so: dense H x W bytes or nullptr
void flow_compose_dev(of_ctx *c, const F2 &f, const F2 &g, const uint8_t *sf, const uint8_t *sg, const F2 &out,
                      uint8_t *so) {
  REQUIRE(f.H == g.H && f.W == g.W && f.P == g.P && out.H == f.H && out.W == f.W && out.P == f.P, OF_EINVAL,
          "flows of different sizes");
  c->cur_px = (double)f.H * f.W;
  const Grid2 gr = grid2(f.H, f.W);
  launch(c, "flow_compose", k_flow_compose, gr.grid, gr.block, 0, (const float2 *)f.p, (const float2 *)g.p, f.H, f.W,
         f.P, sf, sg, out.p, so);
}

// the frame `center` fused with n neighbours along flows centre -> neighbour;
// everything device-resident (frames dense H x W x C, flows of pitch P, states
// dense or nullptr), out dense H x W x C, out_w dense H x W or nullptr
void fuse_dev(of_ctx *c, const float *center, int H, int W, int C, int P, int n, const float *const *neigh,
              const float2 *const *flow, const uint8_t *const *state, const of_fuse_opts &o, float *out,
              float *out_w) {
  FuseArgs A = {};
  for (int k = 0; k < n; ++k) {
    A.neigh[k] = neigh[k];
    A.flow[k] = flow[k];
    A.state[k] = state ? state[k] : nullptr;
  }
  const double two_s2 = 2.0 * (o.sigma * o.sigma);
  const double h2 = (o.strength * o.sigma) * (o.strength * o.sigma);
  const int gx = (W + FUSE_TW - 1) / FUSE_TW, gy = (H + FUSE_TH - 1) / FUSE_TH;
  c->cur_px = (double)H * W;
  launch(c, "fuse", k_fuse, dim3((unsigned)gx * (unsigned)gy), dim3(FUSE_TW * FUSE_TH), 0, center, A, n, H, W, P, C,
         o.patch, two_s2, h2, gx, out, out_w);
}

void denoiser_free(of_ctx *c) {
  Denoiser *d = c->den;
  if (!d) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (float *p : d->frame)
    if (p) hipFree(p);
  for (int k = 0; k < 4; ++k)
    for (void *p : {(void *)d->fw[k], (void *)d->bw[k], (void *)d->sf[k], (void *)d->sb[k]})
      if (p) hipFree(p);
  delete d;
  c->den = nullptr;
}

template <typename T>
void denoiser_alloc(Denoiser *d, T **p, size_t count) {
  HIPCHK(hipMalloc(p, sizeof(T) * count));
  d->bytes += sizeof(T) * count;
}

// Frame t of the session fused with the neighbours at offsets -1, +1, -2, +2
// that exist among the frames pushed so far (|offset| <= radius), written to
// the host buffers.  Offsets of 2 chain two adjacent pairs' flows.
void denoise_emit(of_ctx *c, Denoiser *d, int t, float *out, float *out_weight) {
  const int H = d->H, W = d->W, C = d->C, R = d->opt.radius, NF = 2 * R + 1, NP = 2 * R;
  const size_t px = (size_t)H * W;
  const float *neigh[4];
  const float2 *flow[4];
  const uint8_t *state[4];
  int n = 0;
  auto f2 = [&](float2 *p) {
    F2 f;
    f.p = p;
    f.H = H;
    f.W = W;
    f.P = d->pitch;
    return f;
  };
  for (int a = 1; a <= R; ++a)
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const int s = t + sgn * a;
      if (s < 0 || s >= d->frames) continue;
      neigh[n] = d->frame[s % NF];
      // the pairs along the way: forward t, then t+1; backward t-1, then t-2
      const int p0 = (sgn > 0 ? t : t - 1) % NP;
      float2 *const *fl = sgn > 0 ? d->fw : d->bw;
      uint8_t *const *st = sgn > 0 ? d->sf : d->sb;
      if (a == 1) {
        flow[n] = fl[p0];
        state[n] = st[p0];
      } else {
        const int p1 = (sgn > 0 ? t + 1 : t - 2) % NP;
        const F2 comp = new_f2(c, H, W);
        uint8_t *cs = (uint8_t *)c->arena.alloc(px);
        flow_compose_dev(c, f2(fl[p0]), f2(fl[p1]), st[p0], st[p1], comp, cs);
        flow[n] = comp.p;
        state[n] = cs;
      }
      ++n;
    }
  const float *center = d->frame[t % NF];
  if (n == 0) {  // a clip of one frame
    HIPCHK(hipMemcpyAsync(out, center, sizeof(float) * px * C, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out_weight) std::fill(out_weight, out_weight + px, 1.0f);
    return;
  }
  float *dout = (float *)c->arena.alloc(sizeof(float) * px * C);
  float *dw = out_weight ? (float *)c->arena.alloc(sizeof(float) * px) : nullptr;
  fuse_dev(c, center, H, W, C, d->pitch, n, neigh, flow, state, d->opt, dout, dw);
  HIPCHK(hipMemcpyAsync(out, dout, sizeof(float) * px * C, hipMemcpyDeviceToHost, c->stream));
  if (out_weight) HIPCHK(hipMemcpyAsync(out_weight, dw, sizeof(float) * px, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
}

}  // namespace

extern "C" {

int of_flow_compose(of_ctx *c, const float *f, const float *g, int H, int W, const uint8_t *state_f,
                    const uint8_t *state_g, float *out, uint8_t *out_state) {
  API_BEGIN(c)
  REQUIRE(f && g && out, OF_EINVAL, "bad arguments");
  check_fuse_frame(H, W);
  const size_t px = (size_t)H * W;
  const F2 df = upload_f2(c, f, H, W), dg = upload_f2(c, g, H, W), dout = new_f2(c, H, W);
  uint8_t *dsf = nullptr, *dsg = nullptr, *dso = nullptr;
  if (out_state) {
    if (state_f) {
      dsf = (uint8_t *)c->arena.alloc(px);
      HIPCHK(hipMemcpyAsync(dsf, state_f, px, hipMemcpyHostToDevice, c->stream));
    }
    if (state_g) {
      dsg = (uint8_t *)c->arena.alloc(px);
      HIPCHK(hipMemcpyAsync(dsg, state_g, px, hipMemcpyHostToDevice, c->stream));
    }
    dso = (uint8_t *)c->arena.alloc(px);
  }
  flow_compose_dev(c, df, dg, dsf, dsg, dout, dso);
  download_f2(c, dout, out);
  if (out_state) HIPCHK(hipMemcpyAsync(out_state, dso, px, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_fuse_frames(of_ctx *c, const float *center, int H, int W, int C, int n, const float *neigh, const float *flows,
                   const uint8_t *states, const of_fuse_opts *o, float *out, float *out_weight) {
  API_BEGIN(c)
  REQUIRE(center && neigh && flows && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= FUSE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  REQUIRE(n >= 1 && n <= FUSE_MAX_N, OF_EINVAL, "1..8 neighbours");
  check_fuse_frame(H, W);
  check_fuse_opts(o);
  const size_t px = (size_t)H * W;
  float *dc = (float *)c->arena.alloc(sizeof(float) * px * C);
  float *dn = (float *)c->arena.alloc(sizeof(float) * px * C * n);
  HIPCHK(hipMemcpyAsync(dc, center, sizeof(float) * px * C, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dn, neigh, sizeof(float) * px * C * n, hipMemcpyHostToDevice, c->stream));
  uint8_t *ds = nullptr;
  if (states) {
    ds = (uint8_t *)c->arena.alloc(px * n);
    HIPCHK(hipMemcpyAsync(ds, states, px * n, hipMemcpyHostToDevice, c->stream));
  }
  const float *pn[FUSE_MAX_N];
  const float2 *pf[FUSE_MAX_N];
  const uint8_t *pst[FUSE_MAX_N];
  for (int k = 0; k < n; ++k) {
    const F2 fk = upload_f2(c, flows + (size_t)k * 2 * px, H, W);
    pn[k] = dn + (size_t)k * px * C;
    pf[k] = fk.p;
    pst[k] = ds ? ds + (size_t)k * px : nullptr;
  }
  float *dout = (float *)c->arena.alloc(sizeof(float) * px * C);
  float *dw = out_weight ? (float *)c->arena.alloc(sizeof(float) * px) : nullptr;
  fuse_dev(c, dc, H, W, C, of_pitch(W), n, pn, pf, pst, *o, dout, dw);
  HIPCHK(hipMemcpyAsync(out, dout, sizeof(float) * px * C, hipMemcpyDeviceToHost, c->stream));
  if (out_weight) HIPCHK(hipMemcpyAsync(out_weight, dw, sizeof(float) * px, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_denoise_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_fuse_opts *o) {
  API_BEGIN(c)
  REQUIRE(!c->den, OF_EINVAL, "a temporal denoiser is open on this context (of_denoise_close first)");
  REQUIRE(P, OF_EINVAL, "bad arguments");
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "frames must be (H,W) or (H,W,3)");
  check_fuse_frame(H, W);
  check_fuse_opts(o);
  check_params(P);
  Denoiser *d = new Denoiser();
  c->den = d;
  try {
    d->H = H;
    d->W = W;
    d->C = C;
    d->pitch = of_pitch(W);
    d->P = *P;
    d->opt = *o;
    const size_t px = (size_t)H * W, fpx = (size_t)H * d->pitch;
    for (int k = 0; k < 2 * o->radius + 1; ++k) denoiser_alloc(d, &d->frame[k], px * C);
    for (int k = 0; k < 2 * o->radius; ++k) {
      denoiser_alloc(d, &d->fw[k], fpx);
      denoiser_alloc(d, &d->bw[k], fpx);
      denoiser_alloc(d, &d->sf[k], px);
      denoiser_alloc(d, &d->sb[k], px);
    }
  } catch (...) {
    denoiser_free(c);
    throw;
  }
  API_END(c)
}

int of_denoise_push(of_ctx *c, const float *frame, float *out, float *out_weight, int32_t *out_index) {
  API_BEGIN(c)
  Denoiser *d = c->den;
  REQUIRE(d, OF_EINVAL, "no temporal denoiser is open on this context (of_denoise_open first)");
  REQUIRE(frame && out && out_index, OF_EINVAL, "bad arguments");
  REQUIRE(!d->flushed, OF_EINVAL, "the temporal denoiser has been flushed (of_denoise_close, then open again)");
  const int H = d->H, W = d->W, C = d->C, R = d->opt.radius, k = d->frames;
  const size_t px = (size_t)H * W;
  float *cur = d->frame[k % (2 * R + 1)];
  HIPCHK(hipMemcpyAsync(cur, frame, sizeof(float) * px * C, hipMemcpyHostToDevice, c->stream));
  if (k > 0) {
    const int p = (k - 1) % (2 * R);
    of_params P = d->P;
    F2 uf = init_flow(c, nullptr, H, W), ub = init_flow(c, nullptr, H, W);
    estimate_bidir_dev(c, &P, d->frame[(k - 1) % (2 * R + 1)], cur, H, W, C, uf, ub, d->opt.alpha1, d->opt.alpha2,
                       d->sf[p], d->sb[p], nullptr, nullptr);
    const size_t fb = sizeof(float2) * (size_t)H * uf.P;  // new_f2's pitch is of_pitch(W), the ring's
    HIPCHK(hipMemcpyAsync(d->fw[p], uf.p, fb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d->bw[p], ub.p, fb, hipMemcpyDeviceToDevice, c->stream));
  }
  d->frames = k + 1;
  *out_index = -1;
  if (k >= R) {
    denoise_emit(c, d, k - R, out, out_weight);
    d->next_out = k - R + 1;
    *out_index = k - R;
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));  // the caller's frame has been read
  }
  API_END(c)
}

int of_denoise_flush(of_ctx *c, float *out, float *out_weight, int32_t *out_index) {
  API_BEGIN(c)
  Denoiser *d = c->den;
  REQUIRE(d, OF_EINVAL, "no temporal denoiser is open on this context (of_denoise_open first)");
  REQUIRE(out && out_index, OF_EINVAL, "bad arguments");
  d->flushed = true;
  *out_index = -1;
  if (d->next_out < d->frames) {
    denoise_emit(c, d, d->next_out, out, out_weight);
    *out_index = d->next_out++;
  }
  API_END(c)
}

int of_denoise_close(of_ctx *c) {
  if (!c) return OF_EINVAL;
  if (!c->den)
    return fail(c, OfError{OF_EINVAL, "no temporal denoiser is open on this context (of_denoise_open first)"});
  denoiser_free(c);
  return OF_OK;
}

}  // extern "C"
