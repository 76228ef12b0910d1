// host_fuse.hip — host side of the temporal denoising (kernels_fuse.hip):
// option checks, flow composition, frame fusion and its weights on
// device-resident frames, flows and states, the stage entries on host buffers,
// the rings of frames and pairs the denoiser and the super-resolver
// (host_sr.hip) keep, and the per-context denoiser session.
namespace {

void check_fuse_opts(const of_fuse_opts *o) {
  REQUIRE(o, OF_EINVAL, "no fuse options");
  REQUIRE(o->radius >= 1 && o->radius <= 2, OF_EINVAL, "fuse radius must be 1..2");
  REQUIRE(o->patch >= 0 && o->patch <= FUSE_MAX_R, OF_EINVAL, "fuse patch must be 0..3");
  REQUIRE(std::isfinite(o->sigma) && o->sigma > 0 && std::isfinite(o->strength) && o->strength > 0, OF_EINVAL,
          "sigma and strength must be finite and > 0");
  check_alphas(o->alpha1, o->alpha2);
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

// the kernels' view of n neighbours (state: nullptr, or one pointer or nullptr each)
FuseArgs fuse_args(int n, const float *const *neigh, const float2 *const *flow, const uint8_t *const *state) {
  FuseArgs A = {};
  for (int k = 0; k < n; ++k) {
    A.neigh[k] = neigh[k];
    A.flow[k] = flow[k];
    A.state[k] = state ? state[k] : nullptr;
  }
  return A;
}

// the frame `center` fused with n neighbours along flows centre -> neighbour;
// everything device-resident (frames dense H x W x C, flows of pitch P, states
// dense or nullptr), out dense H x W x C, out_w dense H x W or nullptr
void fuse_dev(of_ctx *c, const float *center, int H, int W, int C, int P, int n, const float *const *neigh,
              const float2 *const *flow, const uint8_t *const *state, const of_fuse_opts &o, float *out,
              float *out_w) {
  const FuseArgs A = fuse_args(n, neigh, flow, state);
  const double two_s2 = 2.0 * (o.sigma * o.sigma);
  const double h2 = (o.strength * o.sigma) * (o.strength * o.sigma);
  const int gx = (W + FUSE_TW - 1) / FUSE_TW, gy = (H + FUSE_TH - 1) / FUSE_TH;
  c->cur_px = (double)H * W;
  launch(c, "fuse", k_fuse, dim3((unsigned)gx * (unsigned)gy), dim3(FUSE_TW * FUSE_TH), 0, center, A, n, H, W, P, C,
         o.patch, two_s2, h2, gx, out, out_w);
}

// the neighbours' weights of that fusion on their own: out_w n dense H x W
// planes (sigma, strength and patch as of_fuse_opts')
void fuse_weights_dev(of_ctx *c, const float *center, int H, int W, int C, int P, int n, const float *const *neigh,
                      const float2 *const *flow, const uint8_t *const *state, double sigma, double strength, int patch,
                      float *out_w) {
  const FuseArgs A = fuse_args(n, neigh, flow, state);
  const double two_s2 = 2.0 * (sigma * sigma);
  const double h2 = (strength * sigma) * (strength * sigma);
  const int gx = (W + FUSE_TW - 1) / FUSE_TW, gy = (H + FUSE_TH - 1) / FUSE_TH;
  c->cur_px = (double)H * W;
  launch(c, "fuse_weights", k_fuse_weights, dim3((unsigned)gx * (unsigned)gy), dim3(FUSE_TW * FUSE_TH), 0, center, A,
         n, H, W, P, C, patch, two_s2, h2, gx, out_w);
}

// The host arguments of a fusion on the device: the frame, n neighbours, their
// flows (pitched) and states (nullptr: none given).  n = 0: no neighbours.
struct FuseInputs {
  float *center = nullptr;
  const float *neigh[FUSE_MAX_N];
  const float2 *flow[FUSE_MAX_N];
  const uint8_t *state[FUSE_MAX_N];
};
FuseInputs upload_fuse_inputs(of_ctx *c, const float *center, int H, int W, int C, int n, const float *neigh,
                              const float *flows, const uint8_t *states) {
  const size_t px = (size_t)H * W;
  FuseInputs in;
  in.center = upload_dense(c, center, px * C);
  if (n == 0) return in;
  float *dn = upload_dense(c, neigh, px * C * n);
  uint8_t *ds = upload_dense(c, states, px * n);
  for (int k = 0; k < n; ++k) {
    const F2 fk = upload_f2(c, flows + (size_t)k * 2 * px, H, W);
    in.neigh[k] = dn + (size_t)k * px * C;
    in.flow[k] = fk.p;
    in.state[k] = ds ? ds + (size_t)k * px : nullptr;
  }
  return in;
}

// the rings of a session that keeps the last 2R adjacent pairs
void ring_alloc(PairRing *d, int R) {
  d->pitch = of_pitch(d->W);
  const size_t px = (size_t)d->H * d->W, fpx = (size_t)d->H * d->pitch;
  d->alloc_frames(2 * R + 1);
  for (int k = 0; k < 2 * R; ++k) {
    d->fw[k] = d->alloc<float2>(fpx);
    d->bw[k] = d->alloc<float2>(fpx);
    d->sf[k] = d->alloc<uint8_t>(px);
    d->sb[k] = d->alloc<uint8_t>(px);
  }
}

// A push into such a session: the frame into the frame ring and, from the
// second frame on, the pair (previous, this) estimated into slot p of the pair
// rings (the states straight into them), which is returned (0 on the first).
struct RingPush {
  PushPair pr;
  int p;
};
RingPush ring_push(of_ctx *c, PairRing *d, int R, const float *frame, double alpha1, double alpha2) {
  RingPush r;
  const int k = d->frames;
  r.p = k > 0 ? (k - 1) % (2 * R) : 0;
  r.pr = session_push(c, d, frame, alpha1, alpha2, d->sf[r.p], d->sb[r.p], nullptr, nullptr);
  if (k > 0) {
    const size_t fb = sizeof(float2) * (size_t)d->H * r.pr.fw.P;  // new_f2's pitch is of_pitch(W), the ring's
    HIPCHK(hipMemcpyAsync(d->fw[r.p], r.pr.fw.p, fb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d->bw[r.p], r.pr.bw.p, fb, hipMemcpyDeviceToDevice, c->stream));
  }
  return r;
}

// The neighbours of frame t at offsets -1, +1, -2, +2 that exist among the
// frames pushed so far (|offset| <= R), in that order, with the flows t ->
// neighbour and their states; returns how many.  Offsets of 2 chain two
// adjacent pairs' flows (arena memory).
int ring_neighbours(of_ctx *c, PairRing *d, int t, int R, const float **neigh, const float2 **flow,
                    const uint8_t **state) {
  const int H = d->H, W = d->W, NF = (int)d->frame.size(), NP = 2 * R;
  const size_t px = (size_t)H * W;
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
        uint8_t *cs = new_dense<uint8_t>(c, px);
        flow_compose_dev(c, f2(fl[p0]), f2(fl[p1]), st[p0], st[p1], comp, cs);
        flow[n] = comp.p;
        state[n] = cs;
      }
      ++n;
    }
  return n;
}

// The sigma frame t of an automatic session is fused with: the root mean
// square of the estimates of its adjacent pairs (t-1, t) and (t, t+1), those
// that exist and rest on at least a quarter of the pixels (a scene cut leaves
// few consistent ones); with neither, the single-frame estimate of frame t
// (one more selection and read-back), or the floor where the frame has no
// 2 x 2 block; never below the floor.
double denoise_auto_sigma(of_ctx *c, Denoiser *d, int t) {
  const int H = d->H, W = d->W, NP = 2 * d->opt.radius;
  double s = 0.0;
  int m = 0;
  for (int j = t - 1; j <= t; ++j) {
    if (j < 0 || j + 1 >= d->frames) continue;
    const of_noise_estimate &e = d->est[j % NP];
    if (4 * e.n < (int64_t)H * W) continue;
    s = s + e.sigma * e.sigma;
    ++m;
  }
  double sigma = d->floor;
  if (m > 0) {
    sigma = std::sqrt(s / (double)m);
  } else if (H >= 2 && W >= 2) {
    of_noise_estimate e;
    noise_single_dev(c, d->frame[t % (int)d->frame.size()], H, W, d->C, &e);
    sigma = e.sigma;
  }
  return sigma >= d->floor ? sigma : d->floor;  // a NaN (no usable block) gives the floor too
}

// Frame t of the session fused with the neighbours at offsets -1, +1, -2, +2
// that exist among the frames pushed so far (|offset| <= radius), written to
// the host buffers.  Offsets of 2 chain two adjacent pairs' flows.
void denoise_emit(of_ctx *c, Denoiser *d, int t, float *out, float *out_weight) {
  const int H = d->H, W = d->W, C = d->C, NF = (int)d->frame.size();
  const size_t px = (size_t)H * W;
  const float *neigh[4];
  const float2 *flow[4];
  const uint8_t *state[4];
  const int n = ring_neighbours(c, d, t, d->opt.radius, neigh, flow, state);
  const float *center = d->frame[t % NF];
  of_fuse_opts opt = d->opt;
  if (d->auto_sigma) opt.sigma = denoise_auto_sigma(c, d, t);
  d->last_sigma = opt.sigma;
  d->emitted = true;
  if (n == 0) {  // a clip of one frame
    download_dense(c, out, center, px * C);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out_weight) std::fill(out_weight, out_weight + px, 1.0f);
    return;
  }
  float *dout = new_dense<float>(c, px * C), *dw = new_dense<float>(c, px, out_weight);
  fuse_dev(c, center, H, W, C, d->pitch, n, neigh, flow, state, opt, dout, dw);
  download_dense(c, out, dout, px * C);
  download_dense(c, out_weight, dw, px);
  HIPCHK(hipStreamSynchronize(c->stream));
}

// of_denoise_open and of_denoise_open_auto: the session and its rings
void denoise_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_fuse_opts *o, bool auto_sigma,
                  double floor) {
  session_open<Denoiser>(c, SES_DENOISE, P, H, W, C, o, check_fuse_opts, [&](Denoiser *d) {
    d->auto_sigma = auto_sigma;
    d->floor = floor;
    ring_alloc(d, o->radius);
  });
}

}  // namespace

extern "C" {

int of_flow_compose(of_ctx *c, const float *f, const float *g, int H, int W, const uint8_t *state_f,
                    const uint8_t *state_g, float *out, uint8_t *out_state) {
  API_BEGIN(c)
  REQUIRE(f && g && out, OF_EINVAL, "bad arguments");
  check_frame(H, W, "temporal fusion");
  const size_t px = (size_t)H * W;
  const F2 df = upload_f2(c, f, H, W), dg = upload_f2(c, g, H, W), dout = new_f2(c, H, W);
  // the states matter only where the composed state is asked for
  uint8_t *dsf = upload_dense(c, out_state ? state_f : nullptr, px);
  uint8_t *dsg = upload_dense(c, out_state ? state_g : nullptr, px);
  uint8_t *dso = new_dense<uint8_t>(c, px, out_state);
  flow_compose_dev(c, df, dg, dsf, dsg, dout, dso);
  download_f2(c, dout, out);
  download_dense(c, out_state, dso, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_fuse_frames(of_ctx *c, const float *center, int H, int W, int C, int n, const float *neigh, const float *flows,
                   const uint8_t *states, const of_fuse_opts *o, float *out, float *out_weight) {
  API_BEGIN(c)
  REQUIRE(center && neigh && flows && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= FUSE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  REQUIRE(n >= 1 && n <= FUSE_MAX_N, OF_EINVAL, "1..8 neighbours");
  check_frame(H, W, "temporal fusion");
  check_fuse_opts(o);
  const size_t px = (size_t)H * W;
  const FuseInputs in = upload_fuse_inputs(c, center, H, W, C, n, neigh, flows, states);
  float *dout = new_dense<float>(c, px * C), *dw = new_dense<float>(c, px, out_weight);
  fuse_dev(c, in.center, H, W, C, of_pitch(W), n, in.neigh, in.flow, in.state, *o, dout, dw);
  download_dense(c, out, dout, px * C);
  download_dense(c, out_weight, dw, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_fuse_weights(of_ctx *c, const float *center, int H, int W, int C, int n, const float *neigh, const float *flows,
                    const uint8_t *states, const of_fuse_opts *o, float *out_w) {
  API_BEGIN(c)
  REQUIRE(center && neigh && flows && out_w, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= FUSE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  REQUIRE(n >= 1 && n <= FUSE_MAX_N, OF_EINVAL, "1..8 neighbours");
  check_frame(H, W, "temporal fusion");
  check_fuse_opts(o);
  const size_t px = (size_t)H * W;
  const FuseInputs in = upload_fuse_inputs(c, center, H, W, C, n, neigh, flows, states);
  float *dw = new_dense<float>(c, px * n);
  fuse_weights_dev(c, in.center, H, W, C, of_pitch(W), n, in.neigh, in.flow, in.state, o->sigma, o->strength, o->patch,
                   dw);
  download_dense(c, out_w, dw, px * n);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_denoise_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_fuse_opts *o) {
  API_BEGIN(c)
  denoise_open(c, P, H, W, C, o, false, 0.0);
  API_END(c)
}

int of_denoise_open_auto(of_ctx *c, const of_params *P, int H, int W, int C, const of_fuse_opts *o, double floor) {
  API_BEGIN(c)
  REQUIRE(o, OF_EINVAL, "no fuse options");
  REQUIRE(std::isfinite(floor) && floor > 0, OF_EINVAL, "the noise floor must be finite and > 0");
  of_fuse_opts a = *o;
  a.sigma = floor;  // the caller's sigma is not read; the checks see a valid one
  denoise_open(c, P, H, W, C, &a, true, floor);
  API_END(c)
}

int of_denoise_last_sigma(of_ctx *c, double *sigma) {
  if (!c) return OF_EINVAL;
  try {
    Denoiser *d = session_get<Denoiser>(c, SES_DENOISE);
    REQUIRE(sigma, OF_EINVAL, "bad arguments");
    REQUIRE(d->emitted, OF_EINVAL, "the temporal denoiser has not emitted a frame yet");
    *sigma = d->last_sigma;
    return OF_OK;
  }
  API_CATCH(c)
}

int of_denoise_push(of_ctx *c, const float *frame, float *out, float *out_weight, int32_t *out_index) {
  API_BEGIN(c)
  Denoiser *d = session_get<Denoiser>(c, SES_DENOISE);
  REQUIRE(frame && out && out_index, OF_EINVAL, "bad arguments");
  session_not_flushed(d, SES_DENOISE);
  const int R = d->opt.radius, k = d->frames;
  const RingPush rp = ring_push(c, d, R, frame, d->opt.alpha1, d->opt.alpha2);
  // the pair's noise level, from what is still on the device: frames k-1 and k, the forward flow and its state
  if (k > 0 && d->auto_sigma)
    noise_pair_dev(c, d->frame[(k - 1) % (int)d->frame.size()], rp.pr.cur, d->H, d->W, d->C, rp.pr.fw.p, rp.pr.fw.P,
                   d->sf[rp.p], &d->est[rp.p]);
  *out_index = -1;
  const int t = session_next_emit(d, R, false);
  if (t >= 0) {
    denoise_emit(c, d, t, out, out_weight);
    *out_index = t;
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));  // the caller's frame has been read
  }
  API_END(c)
}

int of_denoise_flush(of_ctx *c, float *out, float *out_weight, int32_t *out_index) {
  API_BEGIN(c)
  Denoiser *d = session_get<Denoiser>(c, SES_DENOISE);
  REQUIRE(out && out_index, OF_EINVAL, "bad arguments");
  *out_index = -1;
  const int t = session_next_emit(d, d->opt.radius, true);
  if (t >= 0) {
    denoise_emit(c, d, t, out, out_weight);
    *out_index = t;
  }
  API_END(c)
}

int of_denoise_close(of_ctx *c) { return session_close(c, SES_DENOISE); }

}  // extern "C"
