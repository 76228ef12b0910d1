// host_solve.hip — host side of the linear solvers (kernels_solve.hip,
// kernels_cg.hip, kernels_cgs.hip, kernels_cg_wg.hip, kernels_sor.hip,
// kernels_gen.hip): the feed loops, the launch geometry, the CG and SOR
// dispatchers, the solve log, the deferred solve statistics and the
// general-filter (gen_*) solvers.
namespace {

// ---- iterative solve (base.py:87-172) -----------------------------------------
struct SolveResult {
  int iters;
  int done;
  double rel;
  int slot = -1;  // >= 0: CG solve whose state is still in flight (h_ring[slot])
  double px = 0;
  const char *name = nullptr;  // fused CG kernel whose active launches profiling counts
};

// grid for the 2-pixels-per-thread solver kernels, <= PCG_MAX_BLOCKS blocks
Grid2 pair_grid(int H, int W) {
  Grid2 g;
  g.block = dim3(OF_BX, OF_BY, 1);
  int gx = (W + 2 * OF_BX - 1) / (2 * OF_BX), gy = (H + OF_BY - 1) / OF_BY;
  int cap = std::max(1, PCG_MAX_BLOCKS / gx);
  g.grid = dim3(gx, std::min(gy, cap), 1);
  g.nblocks = g.grid.x * g.grid.y;
  return g;
}

// Enqueue iterations in chunks and poll the previous chunk's state (pinned,
// double-buffered) while the current one runs.  The first chunk is sized by
// `first` (the iteration count of the last solve of the same size and
// solver, when known), the second is short, later ones grow up to
// `max_chunk`: launches enqueued after convergence (cheap no-ops, but not
// free) stay few without leaving the GPU idle while the host polls.
template <typename Enq>
int run_chunked(of_ctx *c, int maxiter, int first, int max_chunk, Enq enqueue_iter) {
  int enq = 0, chunk = first, nchunks = 0;
  while (enq < maxiter) {
    const int n = std::min(chunk, maxiter - enq);
    for (int t = 0; t < n; ++t) enqueue_iter(enq + t);
    enq += n;
    const int slot = nchunks & 1;
    HIPCHK(hipMemcpyAsync(&c->h_state[slot], c->d_state, sizeof(PcgState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->ev_state[slot], c->stream));
    ++nchunks;
    if (nchunks >= 2) {
      HIPCHK(hipEventSynchronize(c->ev_state[slot ^ 1]));
      if (c->h_state[slot ^ 1].done) break;
    }
    chunk = nchunks == 1 ? 4 : std::min(std::max(chunk + chunk / 2, 8), max_chunk);
  }
  return enq;
}

// Feed CG launches `depth` ahead of the progress the kernels report in the
// mapped host flag; stop enqueueing as soon as a prologue has declared the
// solve done.  Returns the number of launches enqueued.
template <typename Enq>
int run_fed(of_ctx *c, volatile CgFlag *f, int nmax, int depth, Enq enqueue_iter) {
  f->done = 0;
  f->iter = 0;
  f->upd = 0;
  f->k = -1;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  int enq = 0;
  while (enq < nmax) {
    if (f->done) break;
    if (enq - f->k <= depth) {
      enqueue_iter(enq++);
      continue;
    }
    // the GPU is `depth` launches behind: wait for progress (bounded: after
    // 0.5 s drain the stream; the flag must then show every launch)
    const auto t0 = std::chrono::steady_clock::now();
    while (!f->done && enq - f->k > depth) {
      _mm_pause();
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) {
        HIPCHK(hipStreamSynchronize(c->stream));
        REQUIRE(f->done || f->k == enq - 1, OF_EHIP, "CG progress flag not visible to the host");
        break;
      }
    }
  }
  return enq;
}

// iteration-count hint of the last solve with this size and solver
int& iter_hint(of_ctx *c, int H, int W, int solver) {
  return c->iter_hints[((int64_t)H << 32) | ((int64_t)W << 8) | solver];
}

// profiling: launches of a solve that did work (the rest returned after the
// prologue); bench.py prices algorithmic bytes on these
void note_active(of_ctx *c, const char *name, int launches, double px) {
  if (!c->prof) return;
  const std::string key = std::string(name) + ".active";
  auto &s = c->ktimes[c->prof >= 2 ? key + "@" + std::to_string((long long)px) : key];
  s.px += launches * px;
  s.n += launches;
}

// ---- deferred solve statistics ------------------------------------------------
void note_solve_now(of_stats *st, const SolveResult &r) {
  if (!st) return;
  st->solves++;
  st->solver_iters_total += r.iters;
  st->solver_iters_max = std::max(st->solver_iters_max, r.iters);
  if (r.done == 2) st->solves_not_converged++;
}

// the final state of a deferred CG solve (valid after a stream sync)
SolveResult resolved(of_ctx *c, int slot) {
  const PcgState &s = c->h_ring[slot];
  return {s.iter, s.done, s.bnorm > 0 ? std::sqrt(s.rr) / s.bnorm : 0.0};
}

// statistics of the CG solves since the last stream synchronisation (call
// only after one)
void drain_solves(of_ctx *c) {
  for (auto &l : c->slog_rec)
    if (l.slot >= 0) {
      const SolveResult r = resolved(c, l.slot);
      l.iters = r.iters;
      l.done = r.done;
      l.est = r.rel;
      l.slot = -1;
    }
  for (const auto &p : c->pend) {
    const SolveResult r = resolved(c, p.slot);
    note_solve_now(p.st, r);
    if (p.name) note_active(c, p.name, r.iters + 1, p.px);
  }
  c->pend.clear();
}

void note_solve(of_ctx *c, of_stats *st, const SolveResult &r) {
  if (r.slot >= 0) c->pend.push_back({r.slot, r.px, st, r.name});
  else note_solve_now(st, r);
}

// Coefficients c_i of the degree-m polynomial preconditioner of k_cgs,
// M^-1 = sum_i c_i B^i D^-1 with B = I - X, X = D^-1 A: the Chebyshev
// residual polynomial 1 - X p(X) = T_{m+1}((b + a - 2X) / (b - a)) /
// T_{m+1}((b + a) / (b - a)), re-expanded in powers of B.
void cheb_poly(int m, double a, double b, double *cB) {
  std::vector<std::vector<double>> T(m + 2);
  T[0] = {1.0};
  T[1] = {0.0, 1.0};
  for (int i = 2; i <= m + 1; ++i) {
    T[i].assign(i + 1, 0.0);
    for (size_t j = 0; j < T[i - 1].size(); ++j) T[i][j + 1] += 2.0 * T[i - 1][j];
    for (size_t j = 0; j < T[i - 2].size(); ++j) T[i][j] -= T[i - 2][j];
  }
  auto binom = [](int n, int k) {
    double r = 1.0;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return r;
  };
  const double s = (b + a) / (b - a), g = -2.0 / (b - a);
  const std::vector<double> &t = T[m + 1];
  double Ts = 0.0;
  for (int kk = 0; kk <= m + 1; ++kk) Ts += t[kk] * std::pow(s, kk);
  std::vector<double> Rx(m + 2, 0.0);  // R(X) in powers of X
  for (int kk = 0; kk <= m + 1; ++kk)
    for (int j = 0; j <= kk; ++j) Rx[j] += t[kk] * binom(kk, j) * std::pow(s, kk - j) * std::pow(g, j) / Ts;
  std::vector<double> pX(m + 1);  // p(X) = (1 - R(X)) / X
  for (int j = 1; j <= m + 1; ++j) pX[j - 1] = -Rx[j];
  for (int i = 0; i <= m; ++i) {  // p(1 - B)
    double v = 0.0;
    for (int j = i; j <= m; ++j) v += pX[j] * binom(j, i) * ((i & 1) ? -1.0 : 1.0);
    cB[i] = v;
  }
}

// Chebyshev interval [CG_CHEB_A, 2] of the block-Jacobi-scaled spectrum
// D^-1 A of the 'backslash' preconditioner (kernels_cgs.hip, k_cgs).  The
// lower end trades iterations for parity: 0.06 saves 4 % of the iterations
// but moves the 48x64 smoke pair's mean |uv - oracle| from 6.7e-4 to 6.1e-3
// (knob sweep).
#define CG_CHEB_A 0.04
// the robust GNC stages (alpha < 0.5: D^-1 A with more small eigenvalues):
// 0.02 takes 479 instead of 488 CG iterations per 1080p pair (+1.5 %
// pairs/s; profiles/r3q_cheb_robust_ab.log); 0.01 476 (49.72 / 49.83 vs
// 49.25 / 49.35 pairs/s, parity suites green; profiles/r5aa_cheb01_ab.log).
// Offline at 540p (tools/poly_iters.py's operator): 56 / 54 / 52 / 52
// iterations at 0.04 / 0.02 / 0.01 / 0.005; least-squares polynomials of the
// same degree 62-73; an upper end below 2 makes p negative on the spectrum
#ifndef CG_CHEB_A_ROBUST
#define CG_CHEB_A_ROBUST 0.01
#endif

// Launch geometry of the fused CG iteration kernels for an H x W level.
// k_cg ('pcg'): strips of PCG_SW columns x bands of R rows, 4 bands (waves)
// per 256-thread block, ~CG_PCG_WAVES (640) waves per launch.  k_cgs ('backslash'): strips
// of PCG_SWP columns x bands of R rows, one band per block, ~512 blocks (2
// per CU).  Every block writes one slot of the partials buffer, so the grid
// may not exceed PCG_MAX_BLOCKS blocks: levels wider than PCG_MAX_BLOCKS
// strips are refused (OF_ENOTSUP), never silently mis-sized.
// k_cgs blocks per launch: 2 per CU (LDS-bound) on 256 CUs
#ifndef CGS_TARGET_BLOCKS
#define CGS_TARGET_BLOCKS PCG_MAX_BLOCKS
#endif
// fewest rows per k_cgs band (coarse levels, where the band count is not
// capped by CGS_TARGET_BLOCKS): a launch walks R + 19 row steps
#ifndef CGS_MIN_R
#define CGS_MIN_R 8
#endif
// k_cgs blocks of a fine solve in lanes mode, where OF_TOKEN_SLOTS (2) fine
// solves of different pairs run side by side: one block per CU each, so a
// band is twice as tall (R = 72 at 1080p; 78 at 18 strips) and walks R + 20
// row steps for R rows instead of 36 + 20 (the band halo is recomputed once
// per band).
// Measured (round 3, 2 x 2 reps): 1 slot x 504 blocks 38.9, 2 x 504 40.7,
// 2 x 336 42.8, 2 x 252 44.4 (4 lanes: 45.3), 2 x 200 42.9, 3 x 168 45.0,
// 4 x 128 42.6 pairs/s (profiles/r3y_token_slots_ab.log, r3z_ab.log); 2 x 270
// (15 bands) 42.2, 3 x 252 44.3 vs 44.8 (profiles/r3ak_ab.log).  All of
// those at 18 strips per 1080p row (14 bands of 78 rows at 252).  With the
// edge strips owning their outer halo lanes 1920 columns are 17 strips, and
// a target of 256 gives 15 bands of 72 rows (15 x 72 = 1080, 255 blocks,
// still one per CU): 92 row steps per launch instead of 98.  864 x 1536
// keeps its 14 strips x 18 bands.  (profiles/cgs_edge_strips/)
#ifndef CGS_LANES_BLOCKS
#define CGS_LANES_BLOCKS 256
#endif
// ... of a fine solve below 1.5 Mpx (864 x 1536, stage 2's first level):
// 168 / 196 / 336 measured 43.6 / 44.0 / 43.6 vs 44.9 pairs/s at 252
// (profiles/r3af_864_blocks_ab.log)
#ifndef CGS_LANES_BLOCKS_S
#define CGS_LANES_BLOCKS_S CGS_LANES_BLOCKS
#endif
// k_cgs blocks of the other (coarse) solves in lanes mode: 128 / 252 measured
// +1 % (45.3 / 45.2 vs 44.8 pairs/s, profiles/r3aa_coarse_blocks_ab.log) but
// would make batches of sub-Mpx pairs differ from estimate_flow; kept at 504
#ifndef CGS_LANES_COARSE_BLOCKS
#define CGS_LANES_COARSE_BLOCKS CGS_TARGET_BLOCKS
#endif
// k_cg waves per launch: config 3 (Classic-C + 'pcg', 720p, 4 lanes) 8.5 /
// 9.45 / 9.73 / 9.42 / 8.10 / 7.40 pairs/s at 256 / 384 / 512 / 768 / 1536 /
// 2048 (profiles/r5au_pcg_waves_ab.log, r5av_pcg_waves_ab.log): shorter
// bands lose to their halo rows and to the lanes' shared CUs; with the
// XCD-aware tile order 10.43 / 10.57 / 10.32 at 512 / 640 / 768
// (profiles/r5ba_pcg_waves_xcd_ab.log)
#ifndef CG_PCG_WAVES
#define CG_PCG_WAVES 640
#endif
int cg_geometry(int H, int W, bool split, of_cg_geometry *g, int target_blocks = CGS_TARGET_BLOCKS) {
  if (H < 1 || W < 1) return OF_EINVAL;
  const int sw = split ? PCG_SWP : PCG_SW;
  // k_cgs: the first and the last strip also own their outer halo lanes
  // (2 CGS_HALO columns each), so n strips cover PCG_SWP n + 4 CGS_HALO columns
  const int nstrips = split ? std::max(1, (W - 4 * CGS_HALO + sw - 1) / sw) : (W + sw - 1) / sw;
  if (nstrips > PCG_MAX_BLOCKS) return OF_ENOTSUP;
  int nbands, R, gy;
  if (split) {
    nbands = std::max(1, std::min((H + CGS_MIN_R - 1) / CGS_MIN_R, target_blocks / nstrips));
    R = (H + nbands - 1) / nbands;
    nbands = (H + R - 1) / R;
    gy = nbands;
  } else {
    nbands = std::max(1, std::min((H + 3) / 4, CG_PCG_WAVES / nstrips));
    R = (H + nbands - 1) / nbands;
    nbands = (H + R - 1) / R;
    gy = (nbands + 3) / 4;
    while (nstrips * gy > PCG_MAX_BLOCKS) {  // ends: gy = 1 once R >= H / 4
      ++R;
      nbands = (H + R - 1) / R;
      gy = (nbands + 3) / 4;
    }
  }
  g->grid_x = nstrips;
  g->grid_y = gy;
  g->rows = R;
  g->bands = nbands;
  g->blocks = nstrips * gy;
  // k_cgs: the widest strip is an edge strip (both edges when it is alone)
  g->strip_cols = !split ? sw : sw + (nstrips == 1 ? 4 : 2) * CGS_HALO;
  return g->blocks <= PCG_MAX_BLOCKS ? OF_OK : OF_ENOTSUP;
}

// 'backslash' residual-replacement offers (k_cg_update): before CG launch k
// for k = CG_UPD_FIRST, CG_UPD_FIRST + CG_UPD_EVERY, ... until one acted.
// Solves shorter than CG_UPD_FIRST iterations (the quadratic GNC stage) get
// none: their recursive residual drifts by < 1 % (solve log).
#define CG_UPD_FIRST 16
#define CG_UPD_EVERY 8

// fp64 true residual ||b - A (x [+ x_hi])||^2 and ||b||^2 into out[0..1]
// (solve log)
void log_resid(of_ctx *c, const Img &coef, const F2 &b, const F2 &x, const F2 *xh, double *out) {
  Grid2 g = grid2(b.H, b.W, PCG_MAX_BLOCKS);
  launch(c, "resid", k_resid_part, g.grid, g.block, 0, (const float *)coef.p, coef.ps(), (const float2 *)b.p,
         (const float2 *)x.p, xh ? (const float2 *)xh->p : nullptr, (const PcgState *)(xh ? c->d_state : nullptr),
         b.H, b.W, b.P, c->d_rpart);
  launch(c, "resid", k_resid_final, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)c->d_rpart, g.nblocks, out);
}

// end of a 'backslash' CG solve: with the solve log on, the true residual of
// the solver's iterate x_hi + x_lo (fp64 sum); then x = fl32(x_hi + x_lo)
void finish_backslash(of_ctx *c, const Img &coef, const F2 &b, const F2 &x, const F2 &xh) {
  if (c->slog_idx >= 0) {
    log_resid(c, coef, b, x, &xh, c->d_rlog + 4 * c->slog_idx);
    c->slog_iter = true;
  }
  Grid2 g = grid2(x.H, x.W);
  launch(c, "cg_finalize", k_cg_finalize, g.grid, g.block, 0, x.p, (const float2 *)xh.p, (const PcgState *)c->d_state,
         x.H, x.W, x.P);
}

// ---- the CG arms ('pcg', 'backslash') ---------------------------------------
// what the two CG arms share: the ring slot, the tolerances and, for
// 'backslash', the preconditioner polynomial and x_hi beside the solve's x
struct CgSetup {
  bool block = false;  // 'backslash'
  float poly[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int slot = 0;
  double rtol = 0, upd_rel = 0;
  int maxiter = 0;
  F2 xh;
};
CgSetup cg_setup(of_ctx *c, const of_params *P, int H, int W) {
  CgSetup s;
  s.block = P->solver == OF_SOLVER_BACKSLASH;
  if (s.block) {
    double cb[CG_DEG + 1];
    cheb_poly(CG_DEG, P->alpha < 0.5 ? CG_CHEB_A_ROBUST : CG_CHEB_A, 2.0, cb);
    for (int i = 0; i <= CG_DEG; ++i) s.poly[i] = (float)cb[i];
  }
  // ring slot of this solve; a slot is reused only after a synchronisation
  // has drained its previous solve
  if ((int)c->pend.size() >= OF_SOLVE_RING - 1) {
    HIPCHK(hipStreamSynchronize(c->stream));
    drain_solves(c);
  }
  s.slot = c->ring_next;
  c->ring_next = (s.slot + 1) % OF_SOLVE_RING;
  // 'backslash': one residual replacement at ||r|| < sqrt(rtol) ||b||
  // (k_cg_update), x_hi beside the solve's x
  s.rtol = s.block ? P->exact_rtol : P->pcg_rtol;
  s.upd_rel = s.block && s.rtol > 0 ? std::sqrt(s.rtol) : 0.0;
  s.maxiter = s.block ? P->exact_maxiter : P->pcg_maxiter;
  if (s.block) s.xh = new_f2(c, H, W);
  return s;
}

// end of a CG arm: the 'backslash' finalisation, then the final state into
// the solve's ring slot (read at the next stream synchronisation, drain_solves)
SolveResult cg_queued(of_ctx *c, const CgSetup &s, const Img &coef, const F2 &b, const F2 &x, const char *name) {
  if (s.block) finish_backslash(c, coef, b, x, s.xh);
  HIPCHK(hipMemcpyAsync(&c->h_ring[s.slot], c->d_state, sizeof(PcgState), hipMemcpyDeviceToHost, c->stream));
  SolveResult res{0, 0, 0.0};
  res.slot = s.slot;
  res.px = (double)b.H * b.W;
  res.name = name;
  return res;
}

// coarse levels (<= CG_SMALL_PX pixels): the whole solve in one workgroup
// (k_cg_reg up to CG_REG_PX pixels, k_cg_small above)
SolveResult solve_cg_small(of_ctx *c, const CgSetup &s, const Img &coef, const F2 &b, const F2 &x) {
  const int H = b.H, W = b.W;
  CgSmallArgs a;
  a.coef = coef.p;
  a.ps = coef.ps();
  a.b = b.p;
  a.x = x.p;
  a.r = new_f2(c, H, W).p;
  a.p = new_f2(c, H, W).p;
  a.q = new_f2(c, H, W).p;
  a.y = new_f2(c, H, W).p;
  a.t = new_f2(c, H, W).p;
  a.H = H;
  a.W = W;
  a.P = b.P;
  a.rtol = s.rtol;
  a.maxiter = s.maxiter;
  for (int i = 0; i < 8; ++i) a.poly[i] = s.poly[i];
  a.st = c->d_state;
  a.xh = s.xh.p;
  a.upd_rel = s.upd_rel;
  if ((double)H * W <= CG_REG_PX)
    launch(c, "pcg_small", s.block ? k_cg_reg<CG_DEG, true> : k_cg_reg<0, false>, dim3(1), dim3(64, CGR_T / 64), 0,
           a);
  else
    launch(c, "pcg_small", s.block ? k_cg_small<CG_DEG, true> : k_cg_small<0, false>, dim3(1), dim3(CGW_BX, CGW_BY),
           0, a);
  return cg_queued(c, s, coef, b, x, nullptr);
}

// the fed CG: one launch per iteration, enqueued a few ahead of the progress
// the kernels report (run_fed).  'backslash': k_cgs (the degree-5 iteration
// with its stages split over a block's 4 waves); 'pcg': scipy's Jacobi CG in
// k_cg
SolveResult solve_cg(of_ctx *c, const CgSetup &s, const Img &coef, const F2 &b, const F2 &x) {
  const int H = b.H, W = b.W;
  const bool split = s.block;
  of_cg_geometry geo;
  const bool lanes_fine = c->big && (double)H * W >= c->big_px;  // a token-holding solve
  const int lanes_target = (double)H * W >= 1.5 * (1 << 20) ? CGS_LANES_BLOCKS : CGS_LANES_BLOCKS_S;
  const int gst = cg_geometry(H, W, split, &geo,
                              lanes_fine ? lanes_target : c->big ? CGS_LANES_COARSE_BLOCKS : CGS_TARGET_BLOCKS);
  REQUIRE(gst == OF_OK, gst, "level too wide for the fused CG kernels");
  REQUIRE(coef.ps() * 7 * 4 < 0x40000000ull, OF_ENOTSUP, "level too large for the CG kernels");
  const dim3 grid(geo.grid_x, geo.grid_y), blk(OF_BX, OF_BY);
  const int R = geo.rows, nbands = geo.bands;
  PcgArgs a;
  memset(&a, 0, sizeof(a));
  a.coef = coef.p;
  a.x = x.p;
  a.b = b.p;
  F2 rb[2] = {new_f2(c, H, W), new_f2(c, H, W)}, pb[2] = {new_f2(c, H, W), new_f2(c, H, W)};
  a.H = H;
  a.W = W;
  a.P = b.P;
  a.ps = coef.ps();
  a.nb = geo.blocks;
  a.st = c->d_state;
  a.rtol = s.rtol;
  a.maxiter = s.maxiter;
  a.xh = s.xh.p;
  a.upd_rel = s.upd_rel;
  for (int i = 0; i < 8; ++i) a.poly[i] = s.poly[i];
  a.hflag = c->d_flag + s.slot;
  HIPCHK(hipMemsetAsync(c->d_state, 0, sizeof(PcgState), c->stream));
  auto args_k = [&](int k) {
    PcgArgs ak = a;
    const int cur = k & 1, prev = cur ^ 1;
    ak.r_in = rb[prev].p;
    ak.p_old = pb[prev].p;
    ak.r_out = rb[cur].p;
    ak.p_new = pb[cur].p;
    ak.part_rd = c->d_partials + (size_t)prev * 5 * PCG_MAX_BLOCKS;
    ak.part_wr = c->d_partials + (size_t)cur * 5 * PCG_MAX_BLOCKS;
    return ak;
  };
  volatile CgFlag *hf = c->h_flag + s.slot;
  const int enq = run_fed(c, hf, a.maxiter + 1, 3, [&](int k) {
    // the replacement is offered every CG_UPD_EVERY launches until the
    // host sees that it ran (it acts at most once; extra offers are no-ops)
    if (s.upd_rel > 0 && k >= CG_UPD_FIRST && (k - CG_UPD_FIRST) % CG_UPD_EVERY == 0 && !hf->upd)
      launch(c, "cg_update", k_cg_update, grid, blk, 0, args_k(k), k);
    const bool odd = W & 1;
    auto kern = split ? (k == 0 ? (odd ? k_cgs<true, true> : k_cgs<true, false>)
                                : (odd ? k_cgs<false, true> : k_cgs<false, false>))
                      : (k == 0 ? (odd ? k_cg<true, true> : k_cg<true, false>)
                                : (odd ? k_cg<false, true> : k_cg<false, false>));
    launch(c, "pcg_iter", kern, grid, blk, 0, args_k(k), k, R, nbands);
  });
  // the convergence test of the last enqueued iterate when the solve ran
  // out of launches (a no-op, skipped, once a prologue declared it done)
  if (!hf->done) launch(c, "pcg_check", k_pcg_check, dim3(1), blk, 0, args_k(enq), enq);
  return cg_queued(c, s, coef, b, x, "pcg_iter");
}

// ---- the SOR arms -------------------------------------------------------------
// lexicographic SOR (base.py:138-172): 64-row strips of the u half then of
// the v half (kernels_sor.hip); k_sor_wg and k_sor_pipe run many sweeps in
// flight in one persistent launch, k_sor_lex one launch per sweep
// (of_set_option OF_OPT_SOR_PIPELINE 0; the same iterate bitwise)
SolveResult sor_result(const PcgState &st) {
  return {st.iter, st.done, st.xnorm2 > 0 ? std::sqrt(st.rr / st.xnorm2) : 0.0};
}

// The read-back every SOR arm ends in (a stream synchronisation): the final
// state and the arm's fail word.  True: the arm decided the solve, *r is its
// result; false: one of its hand-off waits gave up.
bool sor_outcome(of_ctx *c, const int *fail, SolveResult *r) {
  HIPCHK(hipMemcpyAsync(&c->h_state[0], c->d_state, sizeof(PcgState), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_norm, fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*(const int *)c->h_norm != 0) return false;
  *r = sor_result(c->h_state[0]);
  return true;
}

// checks, the arguments the arms share, the hand-off words cleared and x = 0
SorArgs sor_begin(of_ctx *c, const of_params *P, const Img &coef, const F2 &b, const F2 &x) {
  const int H = b.H, W = b.W;
  const int nstrips = (H + 63) / 64;
  REQUIRE(nstrips <= SOR_MAXS, OF_ENOTSUP, "level too tall for the SOR kernel");
  REQUIRE(((double)P->sor_max_iters + 2.0) * (W + 64.0) < 2.0e9, OF_ENOTSUP, "sor_max_iters too large");
  SorArgs a;
  memset(&a, 0, sizeof(a));
  a.coef = coef.p;
  a.b = b.p;
  a.x = x.p;
  a.H = H;
  a.W = W;
  a.P = b.P;
  a.ps = coef.ps();
  a.nstrips = nstrips;
  a.stride = W + 64;
  a.ticket = c->d_sor_sync;
  a.prog = (int *)(c->d_sor_sync + 64);
  a.fail = (int *)(c->d_sor_sync + 32);
  a.st = c->d_state;
  a.omega = (float)P->sor_omega;
  a.tol = P->sor_tol;
  a.maxiter = P->sor_max_iters;
  HIPCHK(hipMemsetAsync(c->d_sor_sync, 0, OF_SOR_SYNC_BYTES, c->stream));
  launch(c, "sor_init", k_sor_init, dim3(std::min(1024, (H * b.P + 63) / 64)), dim3(64), 0, a);
  return a;
}

// sweeps that k_sor_wg's LDS ring holds for an H x W level of one strip
int sor_wg_ring(int H, int W) {
  return (int)std::min<size_t>(SORW_MAXW, OF_SORW_RING_BYTES / (sizeof(float2) * (size_t)H * W));
}

// levels of <= 64 rows whose ring of S sweeps fits in LDS (OF_OPT_SOR_PIPELINE
// 2): the pipelined solve in one workgroup, hand-offs through LDS (k_sor_wg).
// False: a wait gave up; x and the state are k_sor_init's.
bool solve_sor_wg(of_ctx *c, const SorArgs &a, int S, SolveResult *r) {
  SorWgArgs w;
  memset(&w, 0, sizeof(w));
  w.coef = a.coef;
  w.b = a.b;
  w.x = a.x;
  w.H = a.H;
  w.W = a.W;
  w.P = a.P;
  w.ps = a.ps;
  w.S = S;
  w.nw = std::min(SORW_MAXW, 2 * S);
  w.omega = a.omega;
  w.tol = a.tol;
  w.maxiter = a.maxiter;
  w.st = a.st;
  w.fail = a.fail;
  const size_t buf = sizeof(float2) * (size_t)a.H * a.W;
  launch(c, "sor_wg", k_sor_wg, dim3(1), dim3(64 * w.nw), buf * S + sizeof(SorWgShared), w);
  if (!sor_outcome(c, a.fail, r)) return false;
  REQUIRE(r->done != 0, OF_EHIP, "SOR workgroup solve ended without a decided sweep");
  note_active(c, "sor_wg", r->iters, (double)a.H * a.W);
  return true;
}

// k_sor_pipe: a persistent grid, hand-offs through HBM.  False: a hand-off
// wait timed out (e.g. the grid could not stay resident beside other lanes'
// work); k_sor_pipe_final left x = 0 and the state as k_sor_init set it.
bool solve_sor_pipe(of_ctx *c, const SorArgs &a, SolveResult *r) {
  const int H = a.H, W = a.W, nstrips = a.nstrips;
  // ring of S sweep buffers: enough for the sweeps the persistent grid (one
  // wave per CU) can hold in flight, 2 * nstrips units per sweep
  const int S = std::max(4, std::min(SOR_RING_MAX, OF_SOR_PIPE_WAVES / (2 * nstrips) + 2));
  if (!c->d_sorp) HIPCHK(hipMalloc(&c->d_sorp, OF_SORP_BYTES));
  SorPipeArgs q;
  memset(&q, 0, sizeof(q));
  q.coef = a.coef;
  q.b = a.b;
  q.x0 = a.x;
  q.bstride = (size_t)H * a.P;
  const size_t ring_bytes = sizeof(float2) * q.bstride * S;
  if (ring_bytes > c->sor_ring_cap) {
    if (c->d_sor_ring) HIPCHK(hipFree(c->d_sor_ring));
    c->d_sor_ring = nullptr;
    c->sor_ring_cap = 0;
    HIPCHK(hipMalloc(&c->d_sor_ring, ring_bytes));
    c->sor_ring_cap = ring_bytes;
  }
  q.ring = c->d_sor_ring;
  q.H = H;
  q.W = W;
  q.P = a.P;
  q.ps = a.ps;
  q.nstrips = nstrips;
  q.S = S;
  q.stride = a.stride;
  char *z = c->d_sorp;
  q.ticket = (unsigned *)z;
  q.fail = (int *)(z + 64);
  q.stop = (int *)(z + 128);
  q.cnt = (int *)(z + 256);
  q.dec = (int *)(z + 512);
  q.prog = (int *)(z + 1024);
  q.part = (double *)(z + OF_SORP_SYNC_BYTES);
  q.res = q.part + (size_t)SOR_RING_MAX * 2 * SOR_MAXS * 2;
  q.omega = a.omega;
  q.tol = a.tol;
  q.maxiter = a.maxiter;
  HIPCHK(hipMemsetAsync(z, 0, OF_SORP_SYNC_BYTES, c->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)q.stop, 0x7fffffff, 1, c->stream));
  // enough waves for S sweeps in flight (more would only poll)
  const int nwaves =
      (int)std::min<int64_t>(std::min(OF_SOR_PIPE_WAVES, 2 * nstrips * S), (int64_t)a.maxiter * 2 * nstrips);
  launch(c, "sor_pipe", k_sor_pipe, dim3(nwaves), dim3(64), OF_SOR_PIPE_SHM, q);
  Grid2 g = grid2(H, W);
  launch(c, "sor_final", k_sor_pipe_final, g.grid, g.block, 0, q, a.x, c->d_state);
  if (!sor_outcome(c, q.fail, r)) return false;
  REQUIRE(r->done != 0, OF_EHIP, "SOR pipeline ended without a decided sweep");
  note_active(c, "sor_pipe", r->iters, (double)H * W);
  return true;
}

// k_sor_lex: one launch per sweep, in chunks (run_chunked)
SolveResult solve_sor_lex(of_ctx *c, const SorArgs &a) {
  double *sor_part = c->d_partials + 10 * PCG_MAX_BLOCKS;  // 2 x [2 * nstrips][2]
  auto args_k = [&](int k) {
    SorArgs ak = a;
    ak.part_rd = sor_part + (size_t)((k + 1) & 1) * 2 * PCG_MAX_BLOCKS;
    ak.part_wr = sor_part + (size_t)(k & 1) * 2 * PCG_MAX_BLOCKS;
    return ak;
  };
  int &hint = iter_hint(c, a.H, a.W, OF_SOLVER_SOR);
  const int enq = run_chunked(c, a.maxiter, hint > 0 ? std::max(16, hint * 3 / 4) : 16, 64, [&](int k) {
    launch(c, "sor_sweep", k_sor_lex, dim3(2 * a.nstrips), dim3(64), OF_SOR_SHM, args_k(k), k);
  });
  launch(c, "sor_final", k_sor_final, dim3(1), dim3(64), 0, args_k(enq), enq);
  SolveResult r;
  REQUIRE(sor_outcome(c, a.fail, &r), OF_EHIP, "SOR strip hand-off timed out");
  hint = r.iters;
  return r;
}

// the solver of P on an assembled level: CG in one workgroup or fed, SOR with
// its fallback chain k_sor_wg -> k_sor_pipe -> k_sor_lex (each redoes the
// solve from the start: the same iterate and sweep count bitwise)
SolveResult solve_impl(of_ctx *c, const of_params *P, const Img &coef, const F2 &b, const F2 &x) {
  const int H = b.H, W = b.W;
  c->cur_px = (double)H * W;
  if (P->solver == OF_SOLVER_PCG || P->solver == OF_SOLVER_BACKSLASH) {
    const CgSetup s = cg_setup(c, P, H, W);
    return (double)H * W <= CG_SMALL_PX ? solve_cg_small(c, s, coef, b, x) : solve_cg(c, s, coef, b, x);
  }
  REQUIRE(P->solver == OF_SOLVER_SOR, OF_EINVAL, "Unknown solver");
  const SorArgs a = sor_begin(c, P, coef, b, x);
  SolveResult r;
  const int wg_ring = c->opt_sor_pipe == 2 && a.maxiter > 0 && H <= 64 ? sor_wg_ring(H, W) : 0;
  if (wg_ring >= OF_SORW_MIN_RING) {
    if (solve_sor_wg(c, a, wg_ring, &r)) return r;
    ++c->sor_fallbacks;
    HIPCHK(hipMemsetAsync(c->d_sor_sync, 0, OF_SOR_SYNC_BYTES, c->stream));
  }
  if (c->opt_sor_pipe >= 1 && a.maxiter > 0) {
    if (solve_sor_pipe(c, a, &r)) return r;
    ++c->sor_fallbacks;
  }
  return solve_sor_lex(c, a);
}

// _solve_linear_system; with the solve log on, followed by the fp64 true
// residual of the final x (diagnostic, off by default)
SolveResult solve(of_ctx *c, const of_params *P, const Img &coef, const F2 &b, const F2 &x) {
  const int idx = c->slog && c->slog_rec.size() < OF_SLOG_MAX ? (int)c->slog_rec.size() : -1;
  c->slog_idx = idx;
  c->slog_iter = false;
  const SolveResult r = solve_impl(c, P, coef, b, x);
  c->slog_idx = -1;
  if (idx >= 0) {
    // residual of the returned fp32 x; also the iterate's unless the solver
    // logged that itself (finish_backslash)
    log_resid(c, coef, b, x, nullptr, c->d_rlog + 4 * idx + 2);
    if (!c->slog_iter) log_resid(c, coef, b, x, nullptr, c->d_rlog + 4 * idx);
    c->slog_rec.push_back({b.H, b.W, P->solver, r.slot, r.iters, r.done, r.rel});
  }
  return r;
}

// ||x||^2 on the host: a stream synchronisation, so it drains the deferred
// statistics too
double norm2(of_ctx *c, const F2 &x) {
  Grid2 g = grid2(x.H, x.W, PCG_MAX_BLOCKS);
  launch(c, "norm2", k_norm2_part, g.grid, g.block, 0, (const float2 *)x.p, x.H, x.W, x.P, c->d_partials);
  launch(c, "norm2", k_norm2_final, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)c->d_partials, g.nblocks,
         c->d_norm);
  HIPCHK(hipMemcpyAsync(c->h_norm, c->d_norm, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  drain_solves(c);
  return *c->h_norm;
}

// ---- general spatial_filters (kernels_gen.hip) ------------------------------
// radius of the DIA offset grid: filters of fh x fw taps couple pixels up to
// (fh - 1, fw - 1) apart
int gen_radius(const of_params *P) {
  int D = 0;
  for (int q = 0; q < P->filters.n; ++q) D = std::max(D, std::max(P->filters.fh[q], P->filters.fw[q]) - 1);
  return D;
}
int gen_nplanes(int D) { return 2 * (2 * D + 1) * (2 * D + 1) + 1; }

GenFilters gen_filters(const of_params *P) {
  GenFilters f;
  memset(&f, 0, sizeof(f));
  f.n = P->filters.n;
  f.D = gen_radius(P);
  for (int q = 0; q < f.n; ++q) {
    f.fh[q] = P->filters.fh[q];
    f.fw[q] = P->filters.fw[q];
    for (int t = 0; t < f.fh[q] * f.fw[q]; ++t) f.taps[q][t] = (float)P->filters.taps[q][t];
    f.ru[q] = to_penf(P->filters.rho_u[q]);
    f.rv[q] = to_penf(P->filters.rho_v[q]);
    f.qu[q] = to_penf(P->filters.qua_u[q]);
    f.qv[q] = to_penf(P->filters.qua_v[q]);
  }
  return f;
}

// per-level buffers of the general path: filter weights, DIA planes, CG vectors
struct GenLevel {
  int D = 0;
  Img w, pl;
  F2 r, p, z, q, t, e;
};
// the solver's part of a level of radius D: the DIA planes and the CG vectors
GenLevel gen_solver_level(of_ctx *c, int D, int H, int W) {
  GenLevel L;
  L.D = D;
  L.pl = new_img(c, H, W, gen_nplanes(D));
  for (F2 *f : {&L.r, &L.p, &L.z, &L.q, &L.t, &L.e}) *f = new_f2(c, H, W);
  return L;
}
GenLevel gen_level(of_ctx *c, const of_params *P, int H, int W) {
  const Img w = new_img(c, H, W, std::max(1, 2 * P->filters.n));
  GenLevel L = gen_solver_level(c, gen_radius(P), H, W);
  L.w = w;
  return L;
}

void gen_flow_operator(of_ctx *c, const of_params *P, const OpArgs &o, const F2 &uv, const F2 *duv, const Img &It,
                       const Img &Ix, const Img &Iy, const F2 *uvhat, const GenLevel &L, const F2 &rhs) {
  const GenFilters f = gen_filters(P);
  Grid2 g = grid2(uv.H, uv.W);
  if (f.n)
    launch(c, "gen_weights", k_gen_weights, g.grid, g.block, 0, f, o, (const float2 *)uv.p,
           (const float2 *)(duv ? duv->p : nullptr), uv.H, uv.W, uv.P, L.w.ps(), L.w.p);
  launch(c, "gen_dia", k_gen_dia, g.grid, g.block, 0, f, o, (const float *)L.w.p, (const float2 *)uv.p,
         (const float2 *)(duv ? duv->p : nullptr), (const float *)It.p, (const float *)Ix.p, (const float *)Iy.p, It.C,
         (const float2 *)(uvhat ? uvhat->p : nullptr), uv.H, uv.W, uv.P, L.pl.ps(), L.pl.p, rhs.p);
}

// CG on the DIA operator with the scipy control flow from x = 0; returns
// (iterations, done)
std::pair<int, int> dia_cg(of_ctx *c, DiaArgs a, int nb, Grid2 g) {
  HIPCHK(hipMemsetAsync(a.st, 0, sizeof(PcgState), c->stream));
  launch(c, "dia_init", k_dia_init, g.grid, g.block, 0, a);
  int it = 0;
  for (;;) {
    const int n = std::min(32, a.maxiter + 1 - it);
    for (int t = 0; t < n; ++t, ++it) {
      launch(c, "dia_dir", k_dia_dir, g.grid, g.block, 0, a, it, nb);
      launch(c, "dia_q", k_dia_q, g.grid, g.block, 0, a, it);
      launch(c, "dia_upd", k_dia_upd, g.grid, g.block, 0, a, it, nb);
    }
    HIPCHK(hipMemcpyAsync(&c->h_state[0], a.st, sizeof(PcgState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->h_state[0].done || it > a.maxiter) break;
  }
  return {c->h_state[0].iter, c->h_state[0].done};
}

// _solve_linear_system (base.py:87-172) on a DIA operator
DiaArgs dia_args(of_ctx *c, const GenLevel &L, const F2 &b, const F2 &x) {
  DiaArgs a;
  memset(&a, 0, sizeof(a));
  a.pl = L.pl.p;
  a.ps = L.pl.ps();
  a.D = L.D;
  a.H = b.H;
  a.W = b.W;
  a.P = b.P;
  a.b = b.p;
  a.x = x.p;
  a.r = L.r.p;
  a.p = L.p.p;
  a.z = L.z.p;
  a.q = L.q.p;
  a.part = c->d_partials;
  a.st = c->d_state;
  return a;
}

SolveResult gen_solve(of_ctx *c, const of_params *P, const GenLevel &L, const F2 &b, const F2 &x) {
  const int H = b.H, W = b.W;
  DiaArgs a = dia_args(c, L, b, x);
  const size_t vbytes = sizeof(float2) * (size_t)H * b.P;
  if (P->solver == OF_SOLVER_SOR) {
    HIPCHK(hipMemsetAsync(x.p, 0, vbytes, c->stream));
    HIPCHK(hipMemsetAsync(a.st, 0, sizeof(PcgState), c->stream));
    const int nt = std::min(1024, (W + 63) / 64 * 64);
    launch(c, "dia_sor", k_dia_sor, dim3(1), dim3(nt), 0, a, (float)P->sor_omega, P->sor_max_iters, P->sor_tol);
    HIPCHK(hipMemcpyAsync(&c->h_state[0], a.st, sizeof(PcgState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return {c->h_state[0].iter, c->h_state[0].done, 0.0};
  }
  REQUIRE(P->solver == OF_SOLVER_PCG || P->solver == OF_SOLVER_BACKSLASH, OF_EINVAL, "Unknown solver");
  const bool bs = P->solver == OF_SOLVER_BACKSLASH;
  a.block = bs;
  Grid2 g = grid2(H, W, PCG_MAX_BLOCKS);
  const int nb = g.nblocks;
  // ||b||
  {
    launch(c, "norm2", k_norm2_part, g.grid, g.block, 0, (const float2 *)b.p, H, W, b.P, c->d_partials);
    launch(c, "norm2", k_norm2_final, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)c->d_partials, nb, c->d_norm);
    HIPCHK(hipMemcpyAsync(c->h_norm, c->d_norm, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  const double bnorm = std::sqrt(*c->h_norm);
  if (!bs) {
    // scipy cg (base.py:116-136): Jacobi, rtol pcg_rtol, maxiter pcg_maxiter
    a.atol = P->pcg_rtol * bnorm;
    a.maxiter = P->pcg_maxiter;
    const auto r = dia_cg(c, a, nb, g);
    return {r.first, r.second, bnorm > 0 ? std::sqrt(c->h_state[0].rr) / bnorm : 0.0};
  }
  // 'backslash' surrogate: 2x2 block-Jacobi CG to exact_rtol, then iterative
  // refinement x += CG(A, b - A x) on the fp64 true residual until it meets
  // exact_rtol ||b|| (at most 4 corrections)
  const double goal = P->exact_rtol * bnorm;
  a.atol = 0.5 * goal;
  a.maxiter = P->exact_maxiter;
  auto r = dia_cg(c, a, nb, g);
  int iters = r.first, done = r.second;
  double rel = 0.0;
  for (int ref = 0;; ++ref) {
    DiaArgs t = a;
    t.x = x.p;
    launch(c, "dia_resid", k_dia_resid, g.grid, g.block, 0, t, L.t.p);
    launch(c, "dia_sum", k_dia_sum, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)(c->d_partials + 8 * PCG_MAX_BLOCKS),
           nb, c->d_norm);
    HIPCHK(hipMemcpyAsync(c->h_norm, c->d_norm, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double tn = std::sqrt(*c->h_norm);
    rel = bnorm > 0 ? tn / bnorm : 0.0;
    if (tn <= goal || ref >= 4 || iters >= P->exact_maxiter) break;
    DiaArgs e = a;
    e.b = L.t.p;
    e.x = L.e.p;
    e.maxiter = P->exact_maxiter - iters;
    r = dia_cg(c, e, nb, g);
    iters += r.first;
    done = r.second;
    launch(c, "dia_acc", k_dia_acc, g.grid, g.block, 0, x.p, (const float2 *)L.e.p, H, W, b.P);
  }
  return {iters, rel <= P->exact_rtol ? 1 : done, rel};
}

// gen_solve with the solve log (of_set_solve_log): the fp64 true residual
// ||b - A x|| / ||b|| of the DIA operator (k_dia_resid) for the iterate and
// the returned x (the same fp32 field here)
SolveResult gen_solve_logged(of_ctx *c, const of_params *P, const GenLevel &L, const F2 &b, const F2 &x) {
  const SolveResult r = gen_solve(c, P, L, b, x);
  if (c->slog && c->slog_rec.size() < OF_SLOG_MAX) {
    const int idx = (int)c->slog_rec.size();
    double *out = c->d_rlog + 4 * idx;
    Grid2 g = grid2(b.H, b.W, PCG_MAX_BLOCKS);
    launch(c, "dia_resid", k_dia_resid, g.grid, g.block, 0, dia_args(c, L, b, x), L.t.p);
    launch(c, "dia_sum", k_dia_sum, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)(c->d_partials + 8 * PCG_MAX_BLOCKS),
           g.nblocks, out);
    launch(c, "norm2", k_norm2_part, g.grid, g.block, 0, (const float2 *)b.p, b.H, b.W, b.P, c->d_rpart);
    launch(c, "norm2", k_norm2_final, dim3(1), dim3(OF_BX, OF_BY), 0, (const double *)c->d_rpart, g.nblocks, out + 1);
    HIPCHK(hipMemcpyAsync(out + 2, out, 2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->slog_rec.push_back({b.H, b.W, P->solver, -1, r.iters, r.done, r.rel});
  }
  return r;
}

}  // namespace
