// host_poisson.hip — host side of the multilevel Poisson solver
// (kernels_poisson.hip): option checks, the levels and their nested windows
// around a bounding box that the caller takes on the host, the setup of the
// operators, the fixed W-cycle schedule and the stage entry of_poisson_solve.
// The blended fill that runs it twice is host_inpaint.hip's.
namespace {

static_assert(PSN_MAX_SWEEPS == OF_BLEND_MAX_SWEEPS && PSN_FIXED == OF_PSN_FIXED && PSN_UNKNOWN == OF_PSN_UNKNOWN &&
                  PSN_EXCLUDED == OF_PSN_EXCLUDED,
              "the kernels' constants are the header's");

void check_blend_opts(const of_blend_opts *o) {
  REQUIRE(o, OF_EINVAL, "no blending options");
  REQUIRE(o->cycles >= 1 && o->cycles <= OF_BLEND_MAX_CYCLES, OF_EINVAL, "cycles must be 1..64");
  REQUIRE(o->sweeps >= 1 && o->sweeps <= PSN_MAX_SWEEPS, OF_EINVAL, "sweeps must be 1..2");
  REQUIRE(o->coarse_sweeps >= 1 && o->coarse_sweeps <= OF_BLEND_MAX_COARSE_SWEEPS, OF_EINVAL,
          "coarse_sweeps must be 1..64");
}

// the box of the nonzero (or == `value` when value >= 0) bytes of an H x W plane, grown by g and clipped
PsnBox psn_box(const uint8_t *m, int H, int W, int value, int g) {
  PsnBox b;
  b.ilo = H;
  b.jlo = W;
  for (int i = 0; i < H; ++i) {
    const uint8_t *row = m + (size_t)i * W;
    int lo = 0, hi = W - 1;
    auto hit = [&](int j) { return value < 0 ? row[j] != 0 : row[j] == value; };
    while (lo < W && !hit(lo)) ++lo;
    if (lo == W) continue;
    while (!hit(hi)) --hi;
    b.ilo = std::min(b.ilo, i);
    b.ihi = i;
    b.jlo = std::min(b.jlo, lo);
    b.jhi = std::max(b.jhi, hi);
  }
  if (b.empty()) return PsnBox();
  b.ilo = std::max(b.ilo - g, 0);
  b.jlo = std::max(b.jlo - g, 0);
  b.ihi = std::min(b.ihi + g, H - 1);
  b.jhi = std::min(b.jhi + g, W - 1);
  return b;
}

// L of an H x W frame: the first level whose grid, ceil(H / 2^L) x
// ceil(W / 2^L), has at most PSN_CMAX cells with a one-cell apron
int psn_levels(int H, int W) {
  int L = 0;
  while (((size_t)((H + (1 << L) - 1) >> L) + 2) * (size_t)(((W + (1 << L) - 1) >> L) + 2) > PSN_CMAX) ++L;
  return L;
}

struct PsnLevel {
  PsnWin win;
  int *d = nullptr;
  ushort4 *wt = nullptr;
  double *x[2] = {nullptr, nullptr}, *b = nullptr;  // x[cur] is the iterate (k_psn_smooth goes from one to the other)
  int cur = 0;
  size_t cells() const { return (size_t)win.h * win.w; }
};
struct PsnPlan {
  int C = 0, L = 0;
  std::vector<PsnLevel> lv;  // 0 .. L
};

// The levels around `box` (not empty), their buffers from the arena: the
// coarsest window is the box's cells of level L and one more on every side,
// the finer ones are its children.
PsnPlan psn_plan(of_ctx *c, int H, int W, int C, const PsnBox &box) {
  PsnPlan p;
  p.C = C;
  p.L = psn_levels(H, W);
  const int L = p.L;
  const int a_i = (box.ilo >> L) - 1, b_i = (box.ihi >> L) + 1, a_j = (box.jlo >> L) - 1, b_j = (box.jhi >> L) + 1;
  p.lv.resize(L + 1);
  for (int l = 0; l <= L; ++l) {
    PsnLevel &v = p.lv[l];
    const int sh = L - l;
    v.win = PsnWin{a_i * (1 << sh), a_j * (1 << sh), (b_i - a_i + 1) << sh, (b_j - a_j + 1) << sh};
    const size_t n = v.cells();
    v.d = new_dense<int>(c, n);
    v.wt = new_dense<ushort4>(c, n);
    v.b = new_dense<double>(c, n * C);
    v.x[0] = new_dense<double>(c, n * C);
    v.x[1] = l < L ? new_dense<double>(c, n * C) : nullptr;
  }
  REQUIRE(p.lv[L].cells() <= PSN_CMAX, OF_ENOTSUP, "the coarsest level does not fit one workgroup");
  return p;
}

// a kernel template's instance for C channels
#define PSN_FOR_C(C, call)      \
  do {                          \
    if ((C) == 1) call(1);      \
    else if ((C) == 2) call(2); \
    else if ((C) == 3) call(3); \
    else call(4);               \
  } while (0)

// The operators and the right-hand side of a solve from the frame-sized device
// planes (k_psn_setup); with `keep` the plan holds a previous solve, whose
// values stay where lab is not unknown.
void psn_setup(of_ctx *c, PsnPlan &p, const uint8_t *lab, const float *vf, const float *vu, const float *s,
               const uint8_t *hs, int H, int W, bool keep) {
  PsnLevel &f = p.lv[0];
  const Grid2 g = grid2(f.win.h, f.win.w);
  c->cur_px = (double)f.cells();
#define PSN_CALL(CT)                                                                                             \
  launch(c, "psn_setup", k_psn_setup<CT>, g.grid, g.block, 0, lab, vf, vu, s, hs, H, W, f.win, keep ? 1 : 0, f.d, \
         f.wt, f.x[f.cur], f.b)
  PSN_FOR_C(p.C, PSN_CALL);
#undef PSN_CALL
  for (int l = 1; l <= p.L; ++l) {
    PsnLevel &a = p.lv[l - 1], &b = p.lv[l];
    const Grid2 gc = grid2(b.win.h, b.win.w);
    c->cur_px = (double)b.cells();
    launch(c, "psn_coarsen", k_psn_coarsen, gc.grid, gc.block, 0, (const int *)a.d, (const ushort4 *)a.wt, a.win.w,
           b.win, b.d, b.wt);
  }
}

void psn_smooth(of_ctx *c, PsnPlan &p, int l, int sweeps) {
  PsnLevel &v = p.lv[l];
  const int gx = (v.win.w + PSN_T - 1) / PSN_T, gy = (v.win.h + PSN_T - 1) / PSN_T;
  c->cur_px = (double)v.cells();
#define PSN_CALL(CT)                                                                                               \
  launch(c, "psn_smooth", k_psn_smooth<CT>, dim3((unsigned)gx * (unsigned)gy), dim3(PSN_THREADS), 0, (const int *)v.d, \
         (const ushort4 *)v.wt, (const double *)v.b, (const double *)v.x[v.cur], v.x[v.cur ^ 1], v.win, gx, sweeps)
  PSN_FOR_C(p.C, PSN_CALL);
#undef PSN_CALL
  v.cur ^= 1;
}

// one W-cycle from level l down: every level but the coarsest is visited twice
// from the level above it
void psn_cycle(of_ctx *c, PsnPlan &p, int l, const of_blend_opts &o) {
  PsnLevel &v = p.lv[l];
  if (l == p.L) {
    c->cur_px = (double)v.cells();
    launch(c, "psn_coarsest", k_psn_coarsest, dim3(p.C), dim3(PSN_THREADS), 0, (const int *)v.d, (const ushort4 *)v.wt,
           (const double *)v.b, v.x[v.cur], v.win, o.coarse_sweeps);
    return;
  }
  psn_smooth(c, p, l, o.sweeps);
  PsnLevel &n = p.lv[l + 1];
  const Grid2 gc = grid2(n.win.h, n.win.w);
  c->cur_px = (double)n.cells();
#define PSN_CALL(CT)                                                                                                \
  launch(c, "psn_restrict", k_psn_restrict<CT>, gc.grid, gc.block, 0, (const int *)v.d, (const ushort4 *)v.wt,      \
         (const double *)v.b, (const double *)v.x[v.cur], v.win.h, v.win.w, (const int *)n.d, n.win, n.b, n.x[n.cur])
  PSN_FOR_C(p.C, PSN_CALL);
#undef PSN_CALL
  psn_cycle(c, p, l + 1, o);
  if (l + 1 < p.L) psn_cycle(c, p, l + 1, o);
  const Grid2 g = grid2(v.win.h, v.win.w);
  c->cur_px = (double)v.cells();
#define PSN_CALL(CT)                                                                                        \
  launch(c, "psn_prolong", k_psn_prolong<CT>, g.grid, g.block, 0, (const int *)v.d, v.win, v.x[v.cur],      \
         (const double *)n.x[n.cur], n.win.w)
  PSN_FOR_C(p.C, PSN_CALL);
#undef PSN_CALL
  psn_smooth(c, p, l, o.sweeps);
}

void psn_run(of_ctx *c, PsnPlan &p, const of_blend_opts &o) {
  for (int k = 0; k < o.cycles; ++k) psn_cycle(c, p, 0, o);
}

}  // namespace

extern "C" {

int of_poisson_solve(of_ctx *c, const uint8_t *label, const float *values, const float *source,
                     const uint8_t *has_source, int H, int W, int C, const of_blend_opts *o, double *out) {
  API_BEGIN(c)
  REQUIRE(label && values && out && (source != nullptr) == (has_source != nullptr), OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= PSN_MAX_C, OF_EINVAL, "values must have 1..4 channels");
  check_blend_opts(o);
  check_frame(H, W, "the Poisson solver");
  const size_t px = (size_t)H * W;
  for (size_t k = 0; k < px; ++k) REQUIRE(label[k] <= PSN_EXCLUDED, OF_EINVAL, "labels must be 0, 1 or 2");
  const PsnBox box = psn_box(label, H, W, PSN_UNKNOWN, 0);
  const float *dv = upload_dense(c, values, px * C);
  double *dout = new_dense<double>(c, px * C);
  PsnPlan p;
  PsnWin win = {0, 0, 0, 0};
  const double *x = nullptr;
  if (!box.empty()) {
    const uint8_t *dl = upload_dense(c, label, px), *dh = upload_dense(c, has_source, px);
    const float *ds = upload_dense(c, source, px * C);
    p = psn_plan(c, H, W, C, box);
    psn_setup(c, p, dl, dv, nullptr, ds, dh, H, W, false);
    psn_run(c, p, *o);
    win = p.lv[0].win;
    x = p.lv[0].x[p.lv[0].cur];
  }
  const Grid2 g = grid2(H, W);
  c->cur_px = (double)px;
#define PSN_CALL(CT) launch(c, "psn_store", k_psn_store<CT>, g.grid, g.block, 0, dv, x, win, H, W, dout)
  PSN_FOR_C(C, PSN_CALL);
#undef PSN_CALL
  download_dense(c, out, dout, px * C);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

}  // extern "C"
