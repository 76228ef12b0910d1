// host_screen.hip — host side of the blind temporal consistency
// (kernels_screen.hip): option checks, the screened solver's levels over the
// whole frame, their setup, the fixed W-cycle schedule (host_poisson.hip's,
// with the screened kernels), one consistency step on device-resident frames,
// flow and state, the stage entries on host buffers and the per-context
// session, which estimates its pairs through session_push (host_session.hip)
// and keeps the previous frame and the previous output.
namespace {

static_assert(PSN_MAX_C == OF_CONSIST_MAX_CHANNELS, "the kernels' channel count is the header's");

void check_consist_opts(const of_consist_opts *o) {
  REQUIRE(o, OF_EINVAL, "no consistency options");
  const of_fuse_opts &f = o->fuse;  // radius is not read
  REQUIRE(f.patch >= 0 && f.patch <= FUSE_MAX_R, OF_EINVAL, "patch must be 0..3");
  REQUIRE(std::isfinite(f.sigma) && f.sigma > 0 && std::isfinite(f.strength) && f.strength > 0, OF_EINVAL,
          "sigma and strength must be finite and > 0");
  check_alphas(f.alpha1, f.alpha2);
  check_blend_opts(&o->solve);
  REQUIRE(std::isfinite(o->lambda) && o->lambda >= 0, OF_EINVAL, "lambda must be finite and >= 0");
}

struct ScrLevel {
  PsnWin win;
  int *d = nullptr;
  ushort4 *wt = nullptr;
  double *q = nullptr;
  double *x[2] = {nullptr, nullptr}, *b = nullptr;  // x[cur] is the iterate (k_scr_smooth goes from one to the other)
  int cur = 0;
  size_t cells() const { return (size_t)win.h * win.w; }
};
struct ScrPlan {
  int C = 0, L = 0;
  std::vector<ScrLevel> lv;  // 0 .. L
};

// The levels of an H x W frame, their buffers from the arena: the coarsest
// window is the whole grid of level L and one cell more on every side, the
// finer ones are its children.
ScrPlan scr_plan(of_ctx *c, int H, int W, int C) {
  ScrPlan p;
  p.C = C;
  p.L = psn_levels(H, W);
  const int L = p.L;
  const int64_t hL = ((H - 1) >> L) + 3, wL = ((W - 1) >> L) + 3;
  REQUIRE((hL << L) < ((int64_t)1 << 30) && (wL << L) < ((int64_t)1 << 30), OF_ENOTSUP,
          "the frame's finest window does not fit the solver's index range");
  REQUIRE(hL * wL <= PSN_CMAX, OF_ENOTSUP, "the coarsest level does not fit one workgroup");
  p.lv.resize(L + 1);
  for (int l = 0; l <= L; ++l) {
    ScrLevel &v = p.lv[l];
    const int sh = L - l;
    v.win = PsnWin{-(1 << sh), -(1 << sh), (int)(hL << sh), (int)(wL << sh)};
    const size_t n = v.cells();
    v.d = new_dense<int>(c, n);
    v.wt = new_dense<ushort4>(c, n);
    v.q = new_dense<double>(c, n);
    v.b = new_dense<double>(c, n * C);
    v.x[0] = new_dense<double>(c, n * C);
    v.x[1] = l < L ? new_dense<double>(c, n * C) : nullptr;
  }
  return p;
}

// What k_scr_setup makes the finest level from (device-resident): the target
// P and either the planes A and Q, or the weight, the flow with its state and
// the previous output.
struct ScrInputs {
  const float *P = nullptr;
  const double *A = nullptr, *Q = nullptr;
  const float *wgt = nullptr;
  double lambda = 0.0;
  F2 flow;
  const uint8_t *state = nullptr;
  const float *prev_out = nullptr;
};

// the operators, screening planes and right-hand side of a solve
void scr_setup(of_ctx *c, ScrPlan &p, const ScrInputs &in, int H, int W) {
  ScrLevel &f = p.lv[0];
  const Grid2 g = grid2(f.win.h, f.win.w);
  c->cur_px = (double)f.cells();
#define SCR_CALL(CT)                                                                                              \
  launch(c, "scr_setup", k_scr_setup<CT>, g.grid, g.block, 0, in.P, in.A, in.Q, in.wgt, in.lambda,                \
         (const float2 *)in.flow.p, in.flow.P, in.state, in.prev_out, H, W, f.win, f.d, f.wt, f.q, f.b, f.x[f.cur])
  PSN_FOR_C(p.C, SCR_CALL);
#undef SCR_CALL
  for (int l = 1; l <= p.L; ++l) {
    ScrLevel &a = p.lv[l - 1], &b = p.lv[l];
    const Grid2 gc = grid2(b.win.h, b.win.w);
    c->cur_px = (double)b.cells();
    launch(c, "psn_coarsen", k_psn_coarsen, gc.grid, gc.block, 0, (const int *)a.d, (const ushort4 *)a.wt, a.win.w,
           b.win, b.d, b.wt);
    launch(c, "scr_coarsen_q", k_scr_coarsen_q, gc.grid, gc.block, 0, (const double *)a.q, a.win.w, b.win, b.q);
  }
}

void scr_smooth(of_ctx *c, ScrPlan &p, int l, int sweeps) {
  ScrLevel &v = p.lv[l];
  const int gx = (v.win.w + PSN_T - 1) / PSN_T, gy = (v.win.h + PSN_T - 1) / PSN_T;
  c->cur_px = (double)v.cells();
#define SCR_CALL(CT)                                                                                                  \
  launch(c, "scr_smooth", k_scr_smooth<CT>, dim3((unsigned)gx * (unsigned)gy), dim3(PSN_THREADS), 0, (const int *)v.d, \
         (const ushort4 *)v.wt, (const double *)v.q, (const double *)v.b, (const double *)v.x[v.cur], v.x[v.cur ^ 1],  \
         v.win, gx, sweeps)
  PSN_FOR_C(p.C, SCR_CALL);
#undef SCR_CALL
  v.cur ^= 1;
}

// one W-cycle from level l down, as psn_cycle
void scr_cycle(of_ctx *c, ScrPlan &p, int l, const of_blend_opts &o) {
  ScrLevel &v = p.lv[l];
  if (l == p.L) {
    c->cur_px = (double)v.cells();
    launch(c, "scr_coarsest", k_scr_coarsest, dim3(p.C), dim3(PSN_THREADS), 0, (const int *)v.d, (const ushort4 *)v.wt,
           (const double *)v.q, (const double *)v.b, v.x[v.cur], v.win, o.coarse_sweeps);
    return;
  }
  scr_smooth(c, p, l, o.sweeps);
  ScrLevel &n = p.lv[l + 1];
  const Grid2 gc = grid2(n.win.h, n.win.w);
  c->cur_px = (double)n.cells();
#define SCR_CALL(CT)                                                                                               \
  launch(c, "scr_restrict", k_scr_restrict<CT>, gc.grid, gc.block, 0, (const int *)v.d, (const ushort4 *)v.wt,     \
         (const double *)v.q, (const double *)v.b, (const double *)v.x[v.cur], v.win.h, v.win.w, (const int *)n.d, \
         (const double *)n.q, n.win, n.b, n.x[n.cur])
  PSN_FOR_C(p.C, SCR_CALL);
#undef SCR_CALL
  scr_cycle(c, p, l + 1, o);
  if (l + 1 < p.L) scr_cycle(c, p, l + 1, o);
  const Grid2 g = grid2(v.win.h, v.win.w);
  c->cur_px = (double)v.cells();
#define SCR_CALL(CT)                                                                                   \
  launch(c, "psn_prolong", k_psn_prolong<CT>, g.grid, g.block, 0, (const int *)v.d, v.win, v.x[v.cur], \
         (const double *)n.x[n.cur], n.win.w)
  PSN_FOR_C(p.C, SCR_CALL);
#undef SCR_CALL
  scr_smooth(c, p, l, o.sweeps);
}

// The screened solve of `in` on an H x W x C frame, everything device-resident:
// (float) of the result into outf and the result into outd, dense H x W x C,
// whichever is not nullptr.
void screened_solve_dev(of_ctx *c, const ScrInputs &in, int H, int W, int C, const of_blend_opts &o, float *outf,
                        double *outd) {
  ScrPlan p = scr_plan(c, H, W, C);
  scr_setup(c, p, in, H, W);
  for (int k = 0; k < o.cycles; ++k) scr_cycle(c, p, 0, o);
  const ScrLevel &f = p.lv[0];
  const Grid2 g = grid2(H, W);
  c->cur_px = (double)H * W;
#define SCR_CALL(CT) \
  launch(c, "scr_store", k_scr_store<CT>, g.grid, g.block, 0, (const double *)f.x[f.cur], f.win, H, W, outf, outd)
  PSN_FOR_C(C, SCR_CALL);
#undef SCR_CALL
}

// One step: the processed frame Pt (H x W x Cp) made consistent with the
// previous output prev_out along the flow B (V -> Vprev, state S or nullptr),
// V and Vprev the original frames (H x W x C); everything device-resident and
// dense.  out (H x W x Cp) may be prev_out: the setup has read it before the
// store writes.  out_w: H x W, the weight.
void consist_step_dev(of_ctx *c, const float *V, const float *Vprev, int H, int W, int C, const float *Pt,
                      const float *prev_out, int Cp, const F2 &B, const uint8_t *S, const of_consist_opts &o,
                      float *out, float *out_w) {
  const float2 *flow = B.p;
  fuse_weights_dev(c, V, H, W, C, B.P, 1, &Vprev, &flow, &S, o.fuse.sigma, o.fuse.strength, o.fuse.patch, out_w);
  ScrInputs in;
  in.P = Pt;
  in.wgt = out_w;
  in.lambda = o.lambda;
  in.flow = B;
  in.state = S;
  in.prev_out = prev_out;
  screened_solve_dev(c, in, H, W, Cp, o.solve, out, nullptr);
}

}  // namespace

extern "C" {

int of_screened_solve(of_ctx *c, const float *target, const double *anchor, const double *weight, int H, int W, int C,
                      const of_blend_opts *o, double *out) {
  API_BEGIN(c)
  REQUIRE(target && anchor && weight && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= PSN_MAX_C, OF_EINVAL, "the target must have 1..4 channels");
  check_blend_opts(o);
  check_frame(H, W, "the screened solver");
  const size_t px = (size_t)H * W;
  for (size_t k = 0; k < px; ++k)
    REQUIRE(std::isfinite(weight[k]) && weight[k] >= 0, OF_EINVAL, "the weights must be finite and >= 0");
  ScrInputs in;
  in.P = upload_dense(c, target, px * C);
  in.A = upload_dense(c, anchor, px * C);
  in.Q = upload_dense(c, weight, px);
  double *dout = new_dense<double>(c, px * C);
  screened_solve_dev(c, in, H, W, C, *o, nullptr, dout);
  download_dense(c, out, dout, px * C);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_consist_step(of_ctx *c, const float *frame, const float *prev_frame, int H, int W, int C,
                    const float *processed, const float *prev_out, int Cp, const float *flow, const uint8_t *state,
                    const of_consist_opts *o, float *out, float *out_weight) {
  API_BEGIN(c)
  REQUIRE(frame && prev_frame && processed && prev_out && flow && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= FUSE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  REQUIRE(Cp >= 1 && Cp <= PSN_MAX_C, OF_EINVAL, "processed frames must have 1..4 channels");
  check_consist_opts(o);
  check_frame(H, W, "temporal consistency");
  const size_t px = (size_t)H * W;
  const float *dv = upload_dense(c, frame, px * C), *dp = upload_dense(c, prev_frame, px * C);
  const float *dP = upload_dense(c, processed, px * Cp), *dO = upload_dense(c, prev_out, px * Cp);
  const uint8_t *ds = upload_dense(c, state, px);
  const F2 b = upload_f2(c, flow, H, W);
  float *dout = new_dense<float>(c, px * Cp), *dw = new_dense<float>(c, px);
  consist_step_dev(c, dv, dp, H, W, C, dP, dO, Cp, b, ds, *o, dout, dw);
  download_dense(c, out, dout, px * Cp);
  download_dense(c, out_weight, dw, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_consist_open(of_ctx *c, const of_params *P, int H, int W, int C, int Cp, const of_consist_opts *o) {
  API_BEGIN(c)
  REQUIRE(Cp >= 1 && Cp <= PSN_MAX_C, OF_EINVAL, "processed frames must have 1..4 channels");
  session_open<Consistency>(c, SES_CONSIST, P, H, W, C, o, check_consist_opts, [&](Consistency *d) {
    d->Cp = Cp;
    d->alloc_frames(2);
    d->out = d->alloc<float>((size_t)H * W * Cp);
  });
  API_END(c)
}

int of_consist_push(of_ctx *c, const float *frame, const float *processed, float *out, float *out_weight) {
  API_BEGIN(c)
  Consistency *d = session_get<Consistency>(c, SES_CONSIST);
  REQUIRE(frame && processed && out, OF_EINVAL, "bad arguments");
  const int H = d->H, W = d->W, C = d->C, Cp = d->Cp;
  const size_t px = (size_t)H * W;
  if (d->frames == 0) {
    // nothing to lean on: the frame becomes the previous one, the processed frame the output as it is
    session_push(c, d, frame, d->opt.fuse.alpha1, d->opt.fuse.alpha2, nullptr, nullptr, nullptr, nullptr);
    HIPCHK(hipMemcpyAsync(d->out, processed, sizeof(float) * px * Cp, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out != processed) memcpy(out, processed, sizeof(float) * px * Cp);
    if (out_weight) std::fill(out_weight, out_weight + px, 0.0f);
  } else {
    uint8_t *dsb = new_dense<uint8_t>(c, px);
    float *dw = new_dense<float>(c, px);
    const float *dP = upload_dense(c, processed, px * Cp);
    const PushPair p = session_push(c, d, frame, d->opt.fuse.alpha1, d->opt.fuse.alpha2, nullptr, dsb, nullptr, nullptr);
    consist_step_dev(c, p.cur, d->frame[(d->frames - 1) % 2], H, W, C, dP, d->out, Cp, p.bw, dsb, d->opt, d->out, dw);
    download_dense(c, out, (const float *)d->out, px * Cp);
    download_dense(c, out_weight, (const float *)dw, px);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  d->frames += 1;
  API_END(c)
}

int of_consist_close(of_ctx *c) { return session_close(c, SES_CONSIST); }

}  // extern "C"
