// host_flow.hip — the flow estimation itself: the assembly dispatch
// (kernels_assemble.hip), the lanes' token, progress reports, the per-level IRLS
// loops of the four methods, the coarse-to-fine GNC schedule and the
// device-side estimate_flow in one and both directions.
namespace {

// ---- assembly: operator arguments and the penalty dispatch ------------------
OpArgs op_args(const of_params *P, double alpha, double lambda2) {
  OpArgs o;
  memset(&o, 0, sizeof(o));
  o.qd = to_penf(P->qua_data);
  o.rd = to_penf(P->rho_data);
  for (int k = 0; k < 2; ++k) {
    o.qsu[k] = to_penf(P->qua_spatial_u[k]);
    o.qsv[k] = to_penf(P->qua_spatial_v[k]);
    o.rsu[k] = to_penf(P->rho_spatial_u[k]);
    o.rsv[k] = to_penf(P->rho_spatial_v[k]);
  }
  o.rc = to_penf(P->rho_couple);
  // alpha == 1: quadratic system only; alpha == 0: robust only; else blend
  // (classic_nl.py:237-248, ba.py:374-385)
  o.use_q = alpha > 0.0;
  o.use_r = alpha < 1.0;
  o.aq_s = (float)((o.use_r ? alpha : 1.0) * P->lambda_q);
  o.ar_s = (float)((o.use_q ? 1.0 - alpha : 1.0) * P->lambda_);
  o.aq_d = (float)(o.use_r ? alpha : 1.0);
  o.ar_d = (float)(o.use_q ? 1.0 - alpha : 1.0);
  o.lambda2 = (float)lambda2;
  // AltBA's robust stage (lorentzian + charbonnier(1e-3) coupling) is
  // ill-conditioned (~3.6e6): its diagonal, a sum of edge weights and a data
  // term, must be rounded once, not per fp32 operation (k_flow_operator_f64)
  o.f64 = P->method == OF_METHOD_ALT_BA;
  o.aq_s_d = (o.use_r ? alpha : 1.0) * P->lambda_q;
  o.ar_s_d = (o.use_q ? 1.0 - alpha : 1.0) * P->lambda_;
  o.aq_d_d = o.use_r ? alpha : 1.0;
  o.ar_d_d = o.use_q ? 1.0 - alpha : 1.0;
  o.lambda2_d = lambda2;
  return o;
}

// the assembly kernels' penalty mode (kernels_assemble.hip, PenMode): the
// quadratic stage or a robust stage whose penalties share one kind get a
// specialised kernel, anything else the run-time form
int pen_mode(const OpArgs &o) {
  auto all = [](std::initializer_list<const PenF *> ps, int kind) {
    for (const PenF *p : ps)
      if (p->kind != kind) return false;
    return true;
  };
  if (o.use_q && !o.use_r)
    return all({&o.qd, &o.qsu[0], &o.qsu[1], &o.qsv[0], &o.qsv[1]}, OF_PEN_QUADRATIC) ? OF_PM_Q : OF_PM_ANY;
  if (o.use_r && !o.use_q) {
    const int k = o.rd.kind;
    if ((k == OF_PEN_GEN_CHARBONNIER || k == OF_PEN_CHARBONNIER || k == OF_PEN_LORENTZIAN || k == OF_PEN_CONST) &&
        all({&o.rsu[0], &o.rsu[1], &o.rsv[0], &o.rsv[1]}, k))
      return OF_PM_R(k);
  }
  return OF_PM_ANY;
}
// calls f(kernel) with the instantiation of template K for mode m
#define OF_BY_PM(m, KT, ...)                                                               \
  switch (m) {                                                                            \
    case OF_PM_Q: f(KT<__VA_ARGS__ OF_PM_Q>); break;                                      \
    case OF_PM_R(OF_PEN_GEN_CHARBONNIER): f(KT<__VA_ARGS__ OF_PM_R(OF_PEN_GEN_CHARBONNIER)>); break; \
    case OF_PM_R(OF_PEN_CHARBONNIER): f(KT<__VA_ARGS__ OF_PM_R(OF_PEN_CHARBONNIER)>); break; \
    case OF_PM_R(OF_PEN_LORENTZIAN): f(KT<__VA_ARGS__ OF_PM_R(OF_PEN_LORENTZIAN)>); break; \
    case OF_PM_R(OF_PEN_CONST): f(KT<__VA_ARGS__ OF_PM_R(OF_PEN_CONST)>); break;           \
    default: f(KT<__VA_ARGS__ OF_PM_ANY>); break;                                          \
  }

// a per-pixel data weight (include/optflow.h) must be a plane of the level,
// pitched like the system's; the fp64 assembly (AltBA) has no weighted form
void check_weight(const Img &wgt, const OpArgs &o, const Img &coef) {
  REQUIRE(!o.f64, OF_ENOTSUP, "a data weight is not supported with AltBA (classic-c-a)");
  REQUIRE(wgt.H == coef.H && wgt.W == coef.W && wgt.P == coef.P && wgt.C == 1, OF_EHIP,
          "data weight: not a plane of this level");
}

// wgt: the level's data-weight plane, or p == nullptr (the <false, ...> kernels)
void flow_operator(of_ctx *c, const OpArgs &o, const F2 &uv, const F2 *duv, const Img &It, const Img &Ix,
                   const Img &Iy, const F2 *uvhat, const Img &coef, const F2 &rhs, const Img &wgt = Img()) {
  Grid2 g = grid2(uv.H, uv.W);
  auto go = [&](auto kern, auto... w) {
    launch(c, "flow_operator", kern, g.grid, g.block, 0, o, (const float2 *)uv.p,
           (const float2 *)(duv ? duv->p : nullptr), (const float *)It.p, (const float *)Ix.p, (const float *)Iy.p,
           It.C, (const float2 *)(uvhat ? uvhat->p : nullptr), uv.H, uv.W, uv.P, coef.ps(), coef.p, rhs.p, w...);
  };
  const int m = uvhat ? OF_PM_ANY : pen_mode(o);
  if (wgt.p) check_weight(wgt, o, coef);
  if (o.f64) {
    go(k_flow_operator_f64);
    return;
  }
  auto f = [&](auto kern) { go(kern, (const float *)wgt.p); };
  if (wgt.p) { OF_BY_PM(m, k_flow_operator, true, ) } else { OF_BY_PM(m, k_flow_operator, false, ) }
}

// partial_deriv + flow_operator fused (k_warp_operator): no It / Ix / Iy
// planes; nc = 1 or 3 image channels, the fp32 assembly, no duv / uvhat
bool can_fuse_warp_op(const of_ctx *c, const OpArgs &o, int nc) {
  return c->opt_fused_warp && !o.f64 && (nc == 1 || nc == 3);
}
// calls f(kernel) with the instantiation of KT for the weight flag WT, the
// interpolation, the channel count (1 or 3) and the penalty mode
#define OF_BY_INTERP_NC_PM(WT, interp, one, m, KT)                                            \
  if (interp == OF_INTERP_BICUBIC) {                                                          \
    if (one) { OF_BY_PM(m, KT, WT, 1, 1, ) } else { OF_BY_PM(m, KT, WT, 1, 3, ) }              \
  } else if (interp == OF_INTERP_CUBIC) {                                                     \
    if (one) { OF_BY_PM(m, KT, WT, 0, 1, ) } else { OF_BY_PM(m, KT, WT, 0, 3, ) }              \
  } else {                                                                                    \
    if (one) { OF_BY_PM(m, KT, WT, 2, 1, ) } else { OF_BY_PM(m, KT, WT, 2, 3, ) }              \
  }
void warp_operator(of_ctx *c, const LevelDeriv &L, int interp, const OpArgs &o, const F2 &uv, const Img &coef,
                   const F2 &rhs, const Img &wgt = Img()) {
  Grid2 g = grid2(uv.H, uv.W);
  const size_t ps = coef.ps();
  REQUIRE(L.I1x.ps() == ps && L.args.nc == L.I1x.C, OF_EHIP, "warp_operator: plane strides differ");
  const float2 *u = (const float2 *)uv.p;
  const char *name = interp == OF_INTERP_BICUBIC ? "warp_operator_hermite"
                     : interp == OF_INTERP_CUBIC ? "warp_operator_bspline"
                                                 : "warp_operator_bilinear";
  auto f = [&](auto kern) {
    launch(c, name, kern, g.grid, g.block, 0, L.args, o, u, uv.H, uv.W, uv.P, ps, coef.p, rhs.p,
           (const float *)wgt.p);
  };
  const int m = pen_mode(o);
  const bool one = L.args.nc == 1;
  if (wgt.p) {
    check_weight(wgt, o, coef);
    OF_BY_INTERP_NC_PM(true, interp, one, m, k_warp_operator)
  } else {
    OF_BY_INTERP_NC_PM(false, interp, one, m, k_warp_operator)
  }
}

// ---- the per-level IRLS loops ----------------------------------------------
struct LevelIn {
  Img im;     // 2*nc planes
  Img guide;  // gc planes or p == nullptr
  Img wgt;    // the per-pixel data weight (one plane) or p == nullptr
};

// Lanes mode (of_pairs_run, of_pairs_run_host, the pair pool): every linear
// solve on a level of >= big_px pixels (solve_tok below) holds one of the
// lanes' token slots (OF_TOKEN_SLOTS = 2) until its GPU work has drained, and
// runs its k_cgs launches with CGS_LANES_BLOCKS (256, one per CU) blocks, so
// two fine solves of different pairs fill the chip side by side with bands
// twice as tall as one solve's 504 blocks would have.  Until round 3 the token
// had one slot and a fine solve 504 blocks (two lanes' 504-block launches
// interleaving at block granularity stall each other: 2 slots x 504 blocks is
// only +4 %).  Only the fine solves hold the token: a fine level's assembly,
// warps and weighted median (VALU/LDS-bound) overlap another lane's CG (issue-
// and HBM-bound); measured 33.8 -> 34.5 pairs/s at 3 lanes vs holding the
// token through whole fine levels.  Tried and rejected (lanes and
// token): the holder's solve on a high-priority stream, and the full-size
// preprocessing under the token.  Outside lanes mode: no-op.
struct BigPhase {
  of_ctx *c;
  bool held = false;
  BigPhase(of_ctx *c_, double px) : c(c_) {
    if (c->big && px >= c->big_px) {
      c->big->lock();
      held = true;
    }
  }
  ~BigPhase() {
    if (held) {
      hipStreamSynchronize(c->stream);
      c->big->unlock();
    }
  }
};

SolveResult solve_tok(of_ctx *c, const of_params *P, const Img &coef, const F2 &b, const F2 &x) {
  BigPhase bp(c, (double)b.H * b.W);
  return solve(c, P, coef, b, x);
}

// ---- progress reports (of_set_progress) ----
struct ProgressOff {  // batch entries: the context (lane 0) does not report
  of_ctx *c;
  of_progress_fn fn;
  explicit ProgressOff(of_ctx *c_) : c(c_), fn(c_->prog_fn) { c->prog_fn = nullptr; }
  ~ProgressOff() { c->prog_fn = fn; }
};
of_progress prog_event(of_ctx *c, int event, int h, int w) {
  of_progress e;
  memset(&e, 0, sizeof(e));
  e.event = event;
  e.stage = c->prog_stage;
  e.level = c->prog_level;
  e.h = h;
  e.w = w;
  return e;
}
// an iteration's solve is done: ||clip(x) - d|| (d may be null) or, with
// limit < 0, ||x|| (HS)
void prog_iter(of_ctx *c, int it, int jl, const F2 &x, const F2 *d, int limit) {
  if (!c->prog_fn) return;
  of_progress e = prog_event(c, OF_EV_ITER, x.H, x.W);
  e.iter = it;
  e.lin = jl;
  e.norm = std::nan("");
  if (c->prog_flags & OF_PROGRESS_ITER) {
    Grid2 g = grid2(x.H, x.W, PCG_MAX_BLOCKS);
    launch(c, "step_norm2", k_step_norm2_part, g.grid, g.block, 0, (const float2 *)x.p,
           d ? (const float2 *)d->p : (const float2 *)nullptr, limit > 0 ? 1 : 0, x.H, x.W, x.P, c->d_partials);
    launch(c, "step_norm2", k_norm2_final, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)c->d_partials, g.nblocks,
           c->d_norm);
    HIPCHK(hipMemcpyAsync(c->h_norm, c->d_norm, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain_solves(c);
    e.norm = std::sqrt(*c->h_norm);
  }
  c->prog_fn(c->prog_user, &e);
}

// HSOpticalFlow.compute_flow_base (hs.py:109-142)
void hs_base(of_ctx *c, const of_params *P, const LevelIn &L, F2 &uv, of_stats *st) {
  const int H = L.im.H, W = L.im.W, nc = L.im.C / 2;
  c->cur_px = (double)H * W;
  LevelDeriv D = level_deriv(c, L.im, nc, P->interp, P->deriv_filter, 0.5);
  Img It = new_img(c, H, W, nc), Ix = new_img(c, H, W, nc), Iy = new_img(c, H, W, nc);
  Img coef = new_img(c, H, W, 7);
  F2 rhs = new_f2(c, H, W), x = new_f2(c, H, W), tmp = new_f2(c, H, W);
  OpArgs o = op_args(P, 0.0, 0.0);
  Grid2 g = grid2(H, W);
  const bool fuse = can_fuse_warp_op(c, o, nc);
  for (int it = 0; it < P->max_warping_iters; ++it) {
    if (fuse) {
      warp_operator(c, D, P->interp, o, uv, coef, rhs, L.wgt);
    } else {
      partial_deriv(c, D, P->interp, uv, It, Ix, Iy);
      flow_operator(c, o, uv, nullptr, It, Ix, Iy, nullptr, coef, rhs, L.wgt);
    }
    note_solve(c, st, solve_tok(c, P, coef, rhs, x));
    c->cur_px = (double)H * W;
    const double xn = std::sqrt(norm2(c, x));
    if (c->prog_fn) {  // hs.py:123-124 prints ||x|| before the exit test
      of_progress e = prog_event(c, OF_EV_ITER, H, W);
      e.iter = it;
      e.norm = xn;
      c->prog_fn(c->prog_user, &e);
    }
    if (xn < 1e-3) break;
    launch(c, "add_update", k_add_update, g.grid, g.block, 0, uv.p, (const float2 *)x.p, P->limit_update, H, W, uv.P);
    if (P->median_filter_size)
      for (int m = 0; m < P->mf_iter; ++m) {
        median2(c, uv, tmp, P->median_filter_size);
        std::swap(uv.p, tmp.p);
      }
  }
}

// BAOpticalFlow / ClassicNLOpticalFlow compute_flow_base (ba.py:143-206,
// classic_nl.py:200-277)
void irls_base(of_ctx *c, const of_params *P, const LevelIn &L, F2 &uv, double alpha, int max_linear,
               of_stats *st) {
  const int H = L.im.H, W = L.im.W, nc = L.im.C / 2;
  c->cur_px = (double)H * W;
  const double blend = P->method == OF_METHOD_BA ? P->blend : 0.5;  // classic_nl.py:232 passes no blend
  LevelDeriv D = level_deriv(c, L.im, nc, P->interp, P->deriv_filter, blend);
  Img It = new_img(c, H, W, nc), Ix = new_img(c, H, W, nc), Iy = new_img(c, H, W, nc);
  Img coef = new_img(c, H, W, 7);
  Img occ = new_img(c, H, W, 1);
  F2 rhs = new_f2(c, H, W), x = new_f2(c, H, W), uv1 = new_f2(c, H, W), uv2 = new_f2(c, H, W);
  F2 duv = new_f2(c, H, W);
  OpArgs o = op_args(P, alpha, 0.0);
  Grid2 g = grid2(H, W);
  const bool nl = P->method == OF_METHOD_CLASSIC_NL;
  const bool gen = P->filters.general;
  REQUIRE(!(gen && L.wgt.p), OF_ENOTSUP, "a data weight is not supported with a general spatial_filters list");
  GenLevel GL;
  if (gen) GL = gen_level(c, P, H, W);
  // one linearisation per warp: warp + assembly fused (no derivative planes)
  const bool fuse = !gen && max_linear == 1 && can_fuse_warp_op(c, o, nc);
  for (int it = 0; it < P->max_iters; ++it) {
    if (!fuse) partial_deriv(c, D, P->interp, uv, It, Ix, Iy);
    for (int jl = 0; jl < max_linear; ++jl) {
      if (gen) {
        gen_flow_operator(c, P, o, uv, jl ? &duv : nullptr, It, Ix, Iy, nullptr, GL, rhs);
        note_solve(c, st, gen_solve_logged(c, P, GL, rhs, x));
      } else if (fuse) {
        warp_operator(c, D, P->interp, o, uv, coef, rhs, L.wgt);
        note_solve(c, st, solve_tok(c, P, coef, rhs, x));
      } else {
        flow_operator(c, o, uv, jl ? &duv : nullptr, It, Ix, Iy, nullptr, coef, rhs, L.wgt);
        note_solve(c, st, solve_tok(c, P, coef, rhs, x));
      }
      c->cur_px = (double)H * W;
      prog_iter(c, it, jl, x, jl ? &duv : nullptr, P->limit_update);
      const bool filt = P->median_filter_size != 0;
      launch(c, nl && filt && L.guide.p ? "update_occ" : "update", k_update_occ, g.grid, g.block, 0,
             (const float2 *)uv.p, (const float2 *)x.p, P->limit_update, uv1.p, (const float *)L.im.p,
             (const float *)L.im.plane(nc), nc, (nl && filt && L.guide.p) ? occ.p : (float *)nullptr, H, W, uv.P,
             L.im.ps());
      const bool last = jl + 1 >= max_linear;
      if (last && filt && nl && L.guide.p) {
        // uv = uv0 + (filtered - uv0) (classic_nl.py:271-275) in the weighted
        // median's own store
        wmf(c, uv1, L.guide, occ.p, uv, P->area_hsz, P->sigma_i, (const float2 *)uv.p);
        continue;
      }
      F2 res = uv1;
      if (filt) {
        if (nl && L.guide.p) wmf(c, uv1, L.guide, occ.p, uv2, P->area_hsz, P->sigma_i);
        else median2(c, uv1, uv2, P->median_filter_size);
        res = uv2;
      }
      if (!last)  // duv = filtered - uv feeds the next linearisation
        launch(c, "sub2", k_sub2, g.grid, g.block, 0, (const float2 *)uv.p, (const float2 *)res.p, duv.p, H, W, uv.P);
      else  // uv = uv0 + (filtered - uv0)  (classic_nl.py:271-275, ba.py:404-407)
        launch(c, "axpy_diff", k_axpy_diff, g.grid, g.block, 0, uv.p, (const float2 *)uv.p, (const float2 *)res.p, H,
               W, uv.P);
    }
  }
}

// AltBAOpticalFlow.compute_flow_base (alt_ba.py:189-274)
void altba_base(of_ctx *c, const of_params *P, const LevelIn &L, F2 &uv, F2 &uvhat, double alpha, bool replacement,
                of_stats *st) {
  const int H = L.im.H, W = L.im.W, nc = L.im.C / 2;
  c->cur_px = (double)H * W;
  LevelDeriv D = level_deriv(c, L.im, nc, P->interp, P->deriv_filter, 0.5);
  Img It = new_img(c, H, W, nc), Ix = new_img(c, H, W, nc), Iy = new_img(c, H, W, nc);
  Img coef = new_img(c, H, W, 7);
  F2 rhs = new_f2(c, H, W), x = new_f2(c, H, W), duv = new_f2(c, H, W), t1 = new_f2(c, H, W), t2 = new_f2(c, H, W);
  Grid2 g = grid2(H, W);
  const int n = P->max_iters;
  const bool gen = P->filters.general;
  GenLevel GL;
  if (gen) GL = gen_level(c, P, H, W);
  std::vector<double> l2s(n + 1);
  const double a = std::log10(1e-4), b = std::log10(P->lambda2);
  for (int t = 0; t < n; ++t) l2s[t] = std::pow(10.0, n == 1 ? a : a + (b - a) * t / (n - 1));
  l2s[n] = P->lambda2;
  double lambda2 = l2s[0];
  for (int i = 0; i < n; ++i) {
    partial_deriv(c, D, P->interp, uv, It, Ix, Iy);
    OpArgs o = op_args(P, alpha, lambda2);
    bool have_duv = false;
    for (int jl = 0; jl < P->max_linear; ++jl) {
      if (gen) {
        gen_flow_operator(c, P, o, uv, have_duv ? &duv : nullptr, It, Ix, Iy, &uvhat, GL, rhs);
        note_solve(c, st, gen_solve_logged(c, P, GL, rhs, x));
      } else {
        flow_operator(c, o, uv, have_duv ? &duv : nullptr, It, Ix, Iy, &uvhat, coef, rhs);
        note_solve(c, st, solve_tok(c, P, coef, rhs, x));
      }
      c->cur_px = (double)H * W;
      prog_iter(c, i, jl, x, have_duv ? &duv : nullptr, P->limit_update);
      // duv = clip(x): computed as (0 + clip(x))
      HIPCHK(hipMemsetAsync(duv.p, 0, sizeof(float2) * (size_t)H * duv.P, c->stream));
      launch(c, "add_update", k_add_update, g.grid, g.block, 0, duv.p, (const float2 *)x.p, P->limit_update, H, W,
             duv.P);
      have_duv = true;
    }
    if (have_duv)
      launch(c, "add_update", k_add_update, g.grid, g.block, 0, uv.p, (const float2 *)duv.p, 0, H, W, uv.P);
    // uvhat = denoise_LO(uv) per component (denoising.py:6-30)
    if (P->median_filter_size) {
      HIPCHK(hipMemcpyAsync(t1.p, uv.p, sizeof(float2) * (size_t)H * uv.P, hipMemcpyDeviceToDevice, c->stream));
      const float lam = (float)(lambda2 / P->lambda3);
      for (int k = 0; k < P->itersLO; ++k) {
        launch(c, "lo_blend", k_lo_blend, g.grid, g.block, 0, (const float2 *)t1.p, (const float2 *)uv.p, lam, t2.p, H,
               W, uv.P);
        median2(c, t2, t1, P->median_filter_size);
      }
      HIPCHK(hipMemcpyAsync(uvhat.p, t1.p, sizeof(float2) * (size_t)H * uv.P, hipMemcpyDeviceToDevice, c->stream));
    } else {
      HIPCHK(hipMemcpyAsync(uvhat.p, uv.p, sizeof(float2) * (size_t)H * uv.P, hipMemcpyDeviceToDevice, c->stream));
    }
    if (replacement)
      HIPCHK(hipMemcpyAsync(uv.p, uvhat.p, sizeof(float2) * (size_t)H * uv.P, hipMemcpyDeviceToDevice, c->stream));
    lambda2 = l2s[i + 1];
  }
}

int auto_levels(int H, int W, double spacing) {
  int m = H < W ? H : W;  // base.py:192-195
  return 1 + (int)std::floor(std::log(m / 16.0) / std::log(spacing));
}

void check_params(const of_params *P) {
  REQUIRE(P->method >= 0 && P->method <= 3, OF_EINVAL, "unknown method");
  REQUIRE(P->solver >= 0 && P->solver <= 2, OF_EINVAL, "Unknown solver");
  REQUIRE(P->interp >= 0 && P->interp <= 2, OF_EINVAL, "Unknown interpolation method");
  REQUIRE(P->median_filter_size == 0 || P->median_filter_size == 3 || P->median_filter_size == 5 ||
              P->median_filter_size == 7,
          OF_ENOTSUP, "median_filter_size must be None, 3, 5 or 7");
  if (P->filters.general) {
    REQUIRE(P->filters.n >= 0 && P->filters.n <= OF_MAX_FILTERS, OF_ENOTSUP, "at most 8 spatial filters");
    for (int q = 0; q < P->filters.n; ++q)
      REQUIRE(P->filters.fh[q] >= 1 && P->filters.fh[q] <= OF_MAX_FDIM && P->filters.fw[q] >= 1 &&
                  P->filters.fw[q] <= OF_MAX_FDIM,
              OF_ENOTSUP, "spatial filters of at most 5 x 5 taps");
  }
}

// what a data weight cannot be combined with, refused before any launch
void check_weight_params(const of_params *P, bool weighted) {
  if (!weighted) return;
  REQUIRE(!P->filters.general, OF_ENOTSUP, "a data weight is not supported with a general spatial_filters list");
  REQUIRE(P->method != OF_METHOD_ALT_BA, OF_ENOTSUP, "a data weight is not supported with AltBA (classic-c-a)");
}

// a host weight plane (H x W dense): finite and >= 0, checked before any launch
void check_weight_values(const float *w, int H, int W) {
  const size_t n = (size_t)H * W;
  for (size_t k = 0; k < n; ++k)
    REQUIRE(std::isfinite(w[k]) && w[k] >= 0.0f, OF_EINVAL, "the data weight must be finite and >= 0");
}

// The pyramids one compute_flow runs on: the texture (or scaled) pair's for
// the first GNC stage and for the later ones, and the weighted median's colour
// guide's when Classic+NL has one
struct FlowPyr {
  std::vector<Img> pyr, gpyr, cpyr, cgpyr;
  std::vector<Img> wpyr, wgpyr;  // the data weight's own pyramids (empty: no weight)
  int levels = 0;
  bool use_guide = false;
};

void guide_pyramids(of_ctx *c, const of_params *P, const Img &guide, FlowPyr &F) {
  F.use_guide = P->method == OF_METHOD_CLASSIC_NL && guide.p;
  if (F.use_guide) {
    F.cpyr = build_pyramid(c, guide, F.levels, P->pyramid_spacing);
    F.cgpyr = build_pyramid(c, guide, P->gnc_pyramid_levels, P->gnc_pyramid_spacing);
  }
}

// compute_flow, first half: preprocessing and pyramids (hs.py:49-75,
// ba.py:57-99, classic_nl.py:89-139, alt_ba.py:81-126)
// images: device 2nc planes; guide: device gc planes or p == nullptr
// weight: the full-resolution data weight (one plane) or p == nullptr
FlowPyr flow_pyramids(of_ctx *c, of_params *P, const Img &images, const Img &guide, const Img &weight = Img()) {
  const int H = images.H, W = images.W, C = images.C, nc = C / 2;
  REQUIRE(nc >= 1 && nc <= OF_MAX_NC, OF_ENOTSUP, "1..4 channels per frame supported");
  Img img;
  if (P->texture) {
    const double alp = (P->method == OF_METHOD_HS || P->method == OF_METHOD_ALT_BA) ? 0.95 : P->alp;
    img = rof_texture(c, images, 1.0 / 8, 100, alp);
  } else if (P->fc && (P->method == OF_METHOD_BA || P->method == OF_METHOD_CLASSIC_NL)) {
    // images - alp * correlate(images, gaussian(5, 1.5)) then [0, 255]
    // (classic_nl.py:109-113, ba.py:280-285), per channel
    auto gk = gaussian(5, 1.5);
    Img sm = new_img(c, H, W, C);
    correlate(c, images, sm, make_taps(gk.data(), 5, 5));
    img = new_img(c, H, W, C);
    Grid2 g = grid2(H, W);
    launch(c, "sub_scaled", k_sub_scaled, gz(g, C), g.block, 0, (const float *)images.p, (const float *)sm.p,
           (float)P->alp, img.p, H, W, img.P, img.ps());
    scale_img(c, img, 0.0f, 255.0f, 2);
  } else {
    img = new_img(c, H, W, C);
    copy_img(c, img, images);
    scale_img(c, img, 0.0f, 255.0f, 2);
  }
  int levels = P->pyramid_levels;
  if (P->method == OF_METHOD_HS || P->method == OF_METHOD_ALT_BA || P->auto_level)
    levels = auto_levels(H, W, P->pyramid_spacing);
  P->pyramid_levels = levels;
  REQUIRE(levels <= OF_MAX_LEVELS, OF_EINVAL, "too many pyramid levels");
  FlowPyr F;
  F.levels = levels;
  F.pyr = build_pyramid(c, img, levels, P->pyramid_spacing);
  if (P->method != OF_METHOD_HS) F.gpyr = build_pyramid(c, img, P->gnc_pyramid_levels, P->gnc_pyramid_spacing);
  guide_pyramids(c, P, guide, F);
  if (weight.p) {
    // the Gaussian and the bilinear resize the frames get: convex
    // combinations, so every level stays >= 0
    F.wpyr = build_pyramid(c, weight, levels, P->pyramid_spacing);
    if (P->method != OF_METHOD_HS) F.wgpyr = build_pyramid(c, weight, P->gnc_pyramid_levels, P->gnc_pyramid_spacing);
  }
  return F;
}

// compute_flow, second half: the GNC x level schedule on given pyramids
// (hs.py:77-99, ba.py:101-138, classic_nl.py:141-198, alt_ba.py:128-187)
// uv_io: full-resolution flow (init in, result out).  Ends in a stream
// synchronisation.
void run_schedule(of_ctx *c, of_params *P, const FlowPyr &F, F2 &uv_io, of_stats *st) {
  const int H = uv_io.H, W = uv_io.W, levels = F.levels;
  const std::vector<Img> &pyr = F.pyr, &gpyr = F.gpyr, &cpyr = F.cpyr, &cgpyr = F.cgpyr;
  const bool use_guide = F.use_guide;
  F2 uv = uv_io, uvhat;
  if (P->method == OF_METHOD_ALT_BA) {
    uvhat = new_f2(c, H, W);
    HIPCHK(hipMemcpyAsync(uvhat.p, uv.p, sizeof(float2) * (size_t)H * uv.P, hipMemcpyDeviceToDevice, c->stream));
  }
  const double alpha_orig = P->alpha;
  const int gnc = P->method == OF_METHOD_HS ? 1 : P->gnc_iters;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> lev_ev;
  for (int ig = 0; ig < gnc; ++ig) {
    const int nl = ig == 0 ? levels : P->gnc_pyramid_levels;
    const std::vector<Img> &lv = ig == 0 ? pyr : gpyr;
    c->prog_stage = ig;
    c->prog_level = -1;
    if (c->prog_fn) {
      of_progress e = prog_event(c, OF_EV_STAGE, H, W);
      c->prog_fn(c->prog_user, &e);
    }
    for (int l = nl - 1; l >= 0; --l) {
      const int h = lv[l].H, w = lv[l].W;
      c->prog_level = l;
      if (c->prog_fn) {
        of_progress e = prog_event(c, OF_EV_LEVEL, h, w);
        c->prog_fn(c->prog_user, &e);
      }
      hipEvent_t e0 = timing_event(c), e1 = timing_event(c);
      HIPCHK(hipEventRecord(e0, c->stream));
      if (uv.H != h || uv.W != w) {
        F2 nuv = new_f2(c, h, w);
        resample_f2(c, uv, nuv);
        uv = nuv;
        if (uvhat.p) {
          F2 nh = new_f2(c, h, w);
          resample_f2(c, uvhat, nh);
          uvhat = nh;
        }
      }
      LevelIn L;
      L.im = lv[l];
      if (use_guide) L.guide = (ig == 0 ? cpyr : cgpyr)[l];
      if (!F.wpyr.empty()) L.wgt = (ig == 0 ? F.wpyr : F.wgpyr)[l];
      if (P->method == OF_METHOD_HS) hs_base(c, P, L, uv, st);
      else if (P->method == OF_METHOD_ALT_BA) altba_base(c, P, L, uv, uvhat, P->alpha, ig != gnc - 1, st);
      else irls_base(c, P, L, uv, P->alpha, ig == 0 ? 1 : P->max_linear, st);
      HIPCHK(hipEventRecord(e1, c->stream));
      if (st && st->n_levels < OF_MAX_LEVELS) {
        st->level_h[st->n_levels] = h;
        st->level_w[st->n_levels] = w;
        st->level_stage[st->n_levels] = ig;
        st->n_levels++;
        lev_ev.push_back({e0, e1});
      }
    }
    if (gnc > 1) {  // GNC alpha schedule (classic_nl.py:180-184, ba.py:329-333)
      const double na = 1.0 - (ig + 1.0) / (gnc - 1.0);
      P->alpha = std::max(0.0, std::min(P->alpha, na));
    }
    if (c->prog_fn) {  // classic_nl.py:186-196, ba.py:132-133, alt_ba.py:175-183
      const F2 &su = P->method == OF_METHOD_ALT_BA && uvhat.p ? uvhat : uv;
      of_progress e = prog_event(c, OF_EV_STAGE_END, su.H, su.W);
      e.level = 0;
      if (c->prog_flags & OF_PROGRESS_FLOW) {
        c->prog_uv.resize(2 * (size_t)su.H * su.W);
        download_f2(c, su, c->prog_uv.data());
        e.uv = c->prog_uv.data();
      }
      HIPCHK(hipStreamSynchronize(c->stream));
      drain_solves(c);
      e.elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->prog_t0).count();
      c->prog_fn(c->prog_user, &e);
    }
  }
  if (P->method == OF_METHOD_BA) P->alpha = alpha_orig;  // ba.py:338-339
  if (P->method == OF_METHOD_HS && P->median_filter_size && uv.H == H && uv.W == W) {  // hs.py:94-97
    F2 t = new_f2(c, H, W);
    median2(c, uv, t, P->median_filter_size);
    uv = t;
  }
  const F2 &res = P->method == OF_METHOD_ALT_BA && uvhat.H == H ? uvhat : uv;
  if (res.H == H && res.W == W && res.p != uv_io.p)
    HIPCHK(hipMemcpyAsync(uv_io.p, res.p, sizeof(float2) * (size_t)H * uv_io.P, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  drain_solves(c);
  if (st) {
    float ms = 0;
    for (size_t k = 0; k < lev_ev.size(); ++k) {
      HIPCHK(hipEventElapsedTime(&ms, lev_ev[k].first, lev_ev[k].second));
      st->level_ms[k] = ms;
    }
  }
}

// GPU time between two events of a finished stream into the preprocessing total
void add_preprocess_ms(of_stats *st, hipEvent_t t0, hipEvent_t t1) {
  if (!st) return;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, t0, t1));
  st->preprocess_ms += ms;
}

// compute_flow (hs.py:49-99, ba.py:57-138, classic_nl.py:89-198, alt_ba.py:81-187)
// images: device 2nc planes; guide: device gc planes or p == nullptr;
// uv_io: full-resolution flow (init in, result out).
// weight: the per-pixel data weight (one plane) or p == nullptr
void compute_flow_dev(of_ctx *c, of_params *P, const Img &images, const Img &guide, F2 &uv_io, of_stats *st,
                      const Img &weight = Img()) {
  check_params(P);
  check_weight_params(P, weight.p != nullptr);
  hipEvent_t t0 = timing_event(c), t1 = timing_event(c);
  HIPCHK(hipEventRecord(t0, c->stream));
  c->prog_t0 = std::chrono::steady_clock::now();
  const FlowPyr F = flow_pyramids(c, P, images, guide, weight);
  HIPCHK(hipEventRecord(t1, c->stream));
  run_schedule(c, P, F, uv_io, st);
  add_preprocess_ms(st, t0, t1);
}

// estimate_flow preprocessing (interface.py:41-64): host or device RGB input
// rgb1/rgb2: (H, W, C) frames on the device, fp32 or (u8) bytes
void estimate_dev(of_ctx *c, of_params *P, const void *rgb1, const void *rgb2, bool u8, int H, int W, int C, F2 &uv,
                  of_stats *st, const Img &weight = Img()) {
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "images must be (H,W) or (H,W,3)");
  check_weight_params(P, weight.p != nullptr);
  hipEvent_t t0 = timing_event(c), t1 = timing_event(c);
  HIPCHK(hipEventRecord(t0, c->stream));
  Img gray = new_img(c, H, W, 2);
  const bool guide_mode = P->guide_mode && P->method == OF_METHOD_CLASSIC_NL;
  Img guide;
  if (guide_mode) guide = new_img(c, H, W, C == 3 ? 3 : 1);
  if (u8) rgb_prep(c, (const uint8_t *)rgb1, (const uint8_t *)rgb2, H, W, C, gray, guide);
  else rgb_prep(c, (const float *)rgb1, (const float *)rgb2, H, W, C, gray, guide);
  HIPCHK(hipEventRecord(t1, c->stream));
  compute_flow_dev(c, P, gray, guide, uv, st, weight);
  add_preprocess_ms(st, t0, t1);
}

// forward-backward check of two device-resident flows (k_fb_check); st_* /
// er_* dense H x W on the device, st_bw / er_fw / er_bw may be nullptr
void fb_check(of_ctx *c, const F2 &fw, const F2 &bw, double alpha1, double alpha2, uint8_t *st_fw, float *er_fw,
              uint8_t *st_bw, float *er_bw) {
  REQUIRE(fw.H == bw.H && fw.W == bw.W && fw.P == bw.P, OF_EINVAL, "flows of different sizes");
  c->cur_px = (double)fw.H * fw.W;
  Grid2 g = grid2(fw.H, fw.W);
  launch(c, "fb_check", k_fb_check, g.grid, g.block, 0, (const float2 *)fw.p, (const float2 *)bw.p, fw.H, fw.W, fw.P,
         alpha1, alpha2, st_fw, er_fw, st_bw, er_bw);
}

// the same levels with the two frames' channel groups exchanged (copies)
std::vector<Img> swap_frames(of_ctx *c, const std::vector<Img> &pyr) {
  std::vector<Img> out;
  for (const Img &m : pyr) {
    const int nc = m.C / 2;
    Img s = new_img(c, m.H, m.W, m.C);
    const size_t half = sizeof(float) * m.ps() * nc;
    HIPCHK(hipMemcpyAsync(s.p, m.plane(nc), half, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s.plane(nc), m.p, half, hipMemcpyDeviceToDevice, c->stream));
    out.push_back(s);
  }
  return out;
}

// Lab guide of `rgb` (interface.py:58-61, 91-141) as estimate_dev builds it
// for its first frame: the /255 decision from this frame's own maximum.  The
// gray planes k_rgb_prep writes beside it go to a scratch pair.
Img lab_guide(of_ctx *c, const float *rgb, const float *other, int H, int W, int C, const Img &gray_out) {
  Img guide = new_img(c, H, W, C == 3 ? 3 : 1);
  rgb_prep(c, rgb, other, H, W, C, gray_out, guide);
  return guide;
}

// estimate_flow in both directions with the forward-backward masks.  Gray
// conversion, the texture split (or scaling) and the image pyramids run once:
// every one of them treats the two frames' planes alike (per-plane kernels,
// joint min / max), so the backward pass's pyramids are the forward ones with
// the planes exchanged.  The colour guide (Lab of each direction's own first
// frame) and its pyramids are built per direction.
// rgb1/rgb2: (H, W, C) fp32 frames on the device; st_fw / st_bw: dense H x W
// device bytes or nullptr
void estimate_bidir_dev(of_ctx *c, of_params *P, const float *rgb1, const float *rgb2, int H, int W, int C,
                        F2 &uv_fw, F2 &uv_bw, double alpha1, double alpha2, uint8_t *st_fw, uint8_t *st_bw,
                        of_stats *sf, of_stats *sb) {
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "images must be (H,W) or (H,W,3)");
  check_params(P);
  hipEvent_t t0 = timing_event(c), t1 = timing_event(c);
  HIPCHK(hipEventRecord(t0, c->stream));
  c->prog_t0 = std::chrono::steady_clock::now();
  const bool guide_mode = P->guide_mode && P->method == OF_METHOD_CLASSIC_NL;
  Img gray = new_img(c, H, W, 2), guide1, guide2;
  if (guide_mode) {
    guide1 = lab_guide(c, rgb1, rgb2, H, W, C, gray);
    guide2 = lab_guide(c, rgb2, rgb1, H, W, C, new_img(c, H, W, 2));
  } else {
    uint32_t *mm = c->d_mm + 2 * 8;
    launch(c, "mm_init", k_mm_init, dim3(1), dim3(64), 0, mm, 1);
    Grid2 g = grid2(H, W);
    launch(c, "rgb_prep", k_rgb_prep<float>, g.grid, g.block, 0, rgb1, rgb2, H, W, C, gray.p, gray.P, gray.ps(),
           (float *)nullptr, (const uint32_t *)mm);
  }
  const FlowPyr F = flow_pyramids(c, P, gray, guide1);
  FlowPyr B;
  B.levels = F.levels;
  B.pyr = swap_frames(c, F.pyr);
  B.gpyr = swap_frames(c, F.gpyr);
  guide_pyramids(c, P, guide2, B);
  HIPCHK(hipEventRecord(t1, c->stream));
  // both passes start from the caller's alpha and leave the same final one
  const double alpha0 = P->alpha;
  const std::vector<size_t> mark = c->arena.mark();
  run_schedule(c, P, F, uv_fw, sf);
  add_preprocess_ms(sf, t0, t1);
  c->arena.rewind(mark);  // run_schedule ended in a stream synchronisation
  P->alpha = alpha0;
  const WallClock wall1;  // the backward pass's total_ms starts here
  c->prog_t0 = wall1.t0;
  run_schedule(c, P, B, uv_bw, sb);
  if (sb) sb->total_ms = wall1.ms();
  if (st_fw || st_bw) {
    if (st_fw) fb_check(c, uv_fw, uv_bw, alpha1, alpha2, st_fw, nullptr, st_bw, nullptr);
    else fb_check(c, uv_bw, uv_fw, alpha1, alpha2, st_bw, nullptr, nullptr, nullptr);
  }
}

// a device counter's value, after everything queued on the stream so far
unsigned read_count(of_ctx *c, const unsigned *d) {
  unsigned h = 0;
  HIPCHK(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return h;
}

// Frames at times t[0..n) between two device-resident frames (dense
// H x W x C) from their flows and forward-backward states (k_interp_*): per
// t one splat, one resolve, as many fill passes as the holes need and one
// render; the frames, flows and states are shared.  out (n x H x W x C),
// out_ut (n x 2 x H x W planar or nullptr) and out_info (n x H x W or
// nullptr) are host buffers.
void interp_frames_dev(of_ctx *c, const float *d1, const float *d2, int H, int W, int C, const F2 &fw, const F2 &bw,
                       const uint8_t *sf, const uint8_t *sb, int n, const double *t, float *out, float *out_ut,
                       uint8_t *out_info) {
  const size_t px = (size_t)H * W;
  unsigned long long *key = (unsigned long long *)c->arena.alloc(sizeof(unsigned long long) * px);
  F2 ut[2] = {new_f2(c, H, W), new_f2(c, H, W)};
  uint8_t *hole[2] = {(uint8_t *)c->arena.alloc(px), (uint8_t *)c->arena.alloc(px)};
  unsigned *cnt = (unsigned *)c->arena.alloc(sizeof(unsigned));
  float *dout = (float *)c->arena.alloc(sizeof(float) * px * C);
  float *dut = out_ut ? (float *)c->arena.alloc(sizeof(float) * 2 * px) : nullptr;
  uint8_t *dinfo = (uint8_t *)c->arena.alloc(px);
  c->cur_px = (double)px;
  const Grid2 g = grid2(H, W);
  for (int k = 0; k < n; ++k) {
    const double tk = t[k], omt = 1.0 - tk;
    HIPCHK(hipMemsetAsync(key, 0xff, sizeof(unsigned long long) * px, c->stream));
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned), c->stream));
    launch(c, "interp_splat", k_interp_splat, gz(g, 2), g.block, 0, d1, d2, C, (const float2 *)fw.p,
           (const float2 *)bw.p, H, W, fw.P, tk, omt, key);
    launch(c, "interp_resolve", k_interp_resolve, g.grid, g.block, 0, (const unsigned long long *)key,
           (const float2 *)fw.p, (const float2 *)bw.p, H, W, fw.P, ut[0].p, hole[0], cnt);
    int cur = 0;
    // Jacobi passes until no hole is left; a pass that fills nothing means no
    // pixel has a motion at all: zero motion everywhere
    for (unsigned holes = read_count(c, cnt); holes > 0;) {
      HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned), c->stream));
      launch(c, "interp_fill", k_interp_fill, g.grid, g.block, 0, (const float2 *)ut[cur].p,
             (const uint8_t *)hole[cur], ut[cur ^ 1].p, hole[cur ^ 1], H, W, fw.P, cnt);
      cur ^= 1;
      const unsigned left = read_count(c, cnt);
      if (left == holes) {
        HIPCHK(hipMemsetAsync(ut[cur].p, 0, sizeof(float2) * (size_t)H * fw.P, c->stream));
        break;
      }
      holes = left;
    }
    launch(c, "interp_render", k_interp_render, g.grid, g.block, 0, d1, d2, C, (const float2 *)ut[cur].p,
           (const uint8_t *)hole[cur], sf, sb, H, W, fw.P, tk, omt, dout, dinfo);
    HIPCHK(hipMemcpyAsync(out + (size_t)k * px * C, dout, sizeof(float) * px * C, hipMemcpyDeviceToHost, c->stream));
    if (out_ut) {
      f2_to_dense(c, ut[cur], dut);
      HIPCHK(hipMemcpyAsync(out_ut + (size_t)k * 2 * px, dut, sizeof(float) * 2 * px, hipMemcpyDeviceToHost,
                            c->stream));
    }
    if (out_info) HIPCHK(hipMemcpyAsync(out_info + (size_t)k * px, dinfo, px, hipMemcpyDeviceToHost, c->stream));
  }
}

// the arguments the interpolation entries share (before anything is uploaded)
void check_interp_args(int H, int W, double alpha1, double alpha2, int n, const double *t) {
  REQUIRE((size_t)H * W < ((size_t)1 << 31), OF_ENOTSUP,
          "frame interpolation takes H * W < 2^31 (the splat key holds a 31-bit source index)");
  check_alphas(alpha1, alpha2);
  REQUIRE(n >= 1 && t, OF_EINVAL, "at least one time t");
  for (int k = 0; k < n; ++k) REQUIRE(t[k] > 0.0 && t[k] < 1.0, OF_EINVAL, "every t must lie strictly inside (0, 1)");
}

// estimate_flow on a device-resident slot, on ctx c's stream (synchronous)
void run_slot(of_ctx *c, const Slot &s, of_params *P, of_stats *st) {
  if (st) memset(st, 0, sizeof(*st));
  const WallClock wall;
  F2 uv = init_flow(c, nullptr, s.H, s.W);
  estimate_dev(c, P, s.rgb1, s.rgb2, s.u8, s.H, s.W, s.C, uv, st);
  f2_to_dense(c, uv, s.uv);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) st->total_ms = wall.ms();
}

}  // namespace
