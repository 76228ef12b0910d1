// host_track.hip — host side of the point tracker (kernels_track.hip): option
// checks, the advance and seed steps on device-resident flows and tables, the
// two stage entries on host buffers and the per-context tracker session.
namespace {

void check_track_opts(const of_track_opts *o) {
  REQUIRE(o, OF_EINVAL, "no track options");
  REQUIRE(o->step >= 1 && o->step <= 64, OF_EINVAL, "track step must be 1..64");
  REQUIRE(o->max_tracks >= 1 && o->max_tracks <= (1 << 24), OF_EINVAL, "max_tracks must be 1..2^24");
  for (double v : {o->alpha1, o->alpha2, o->beta1, o->beta2, o->min_eig})
    REQUIRE(std::isfinite(v) && v >= 0, OF_EINVAL, "alpha1, alpha2, beta1, beta2 and min_eig must be finite and >= 0");
}

inline dim3 track_grid(int n) { return dim3((unsigned)((n + TRK_BLOCK - 1) / TRK_BLOCK)); }

// one step of n device-resident tracks along two device-resident flows
void track_advance_dev(of_ctx *c, const F2 &fw, const F2 &bw, const of_track_opts &o, int n, const float2 *xy_in,
                       const uint8_t *st_in, float2 *xy_out, uint8_t *st_out) {
  REQUIRE(fw.H == bw.H && fw.W == bw.W && fw.P == bw.P, OF_EINVAL, "flows of different sizes");
  c->cur_px = (double)n;
  launch(c, "track_advance", k_track_advance, track_grid(n), dim3(TRK_BLOCK), 0, (const float2 *)fw.p,
         (const float2 *)bw.p, fw.H, fw.W, fw.P, o.alpha1, o.alpha2, o.beta1, o.beta2, n, xy_in, st_in, xy_out, st_out);
}

// the seeding grid of a frame
struct SeedGrid {
  int nci, ncj, ncells, nb;
};
SeedGrid seed_grid(int H, int W, int step) {
  SeedGrid g;
  g.nci = (H + step - 1) / step;
  g.ncj = (W + step - 1) / step;
  g.ncells = g.nci * g.ncj;
  g.nb = (g.ncells + TRK_BLOCK - 1) / TRK_BLOCK;
  return g;
}

// Seed on the pitched gray plane for a device-resident table of n tracks:
// occupancy, accept flags with block counts, their scan, scatter of the first
// `room` accepted cells into xy_new / st_new / start_new (new track r at index
// r).  occ / flags: one byte per cell; bcnt: nb + 1 ints.  Returns the number
// of accepted cells (one stream synchronisation).
int track_seed_dev(of_ctx *c, const Img &gray, const of_track_opts &o, int frame, int n, const float2 *xy,
                   const uint8_t *st, uint8_t *occ, uint8_t *flags, int *bcnt, int room, float2 *xy_new,
                   uint8_t *st_new, int32_t *start_new) {
  const SeedGrid g = seed_grid(gray.H, gray.W, o.step);
  HIPCHK(hipMemsetAsync(occ, 0, (size_t)g.ncells, c->stream));
  c->cur_px = (double)n;
  if (n > 0)
    launch(c, "track_mark", k_track_mark, track_grid(n), dim3(TRK_BLOCK), 0, n, xy, st, gray.H, gray.W, o.step, g.ncj,
           occ);
  c->cur_px = (double)g.ncells;
  launch(c, "track_flags", k_track_flags, dim3(g.nb), dim3(TRK_BLOCK), 0, (const float *)gray.p, gray.H, gray.W,
         gray.P, o.step, g.nci, g.ncj, o.min_eig, (const uint8_t *)occ, flags, bcnt);
  launch(c, "track_scan", k_track_scan, dim3(1), dim3(TRK_BLOCK), 0, bcnt, g.nb, bcnt + g.nb);
  launch(c, "track_scatter", k_track_scatter, dim3(g.nb), dim3(TRK_BLOCK), 0, (const uint8_t *)flags,
         (const int *)bcnt, o.step, g.ncells, g.ncj, room, frame, xy_new, st_new, start_new);
  int total = 0;
  HIPCHK(hipMemcpyAsync(&total, bcnt + g.nb, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return total;
}

// the gray plane the tracker seeds on: the frame itself (C == 1) or its
// _rgb2gray plane (C == 3), as k_rgb_prep writes it (plane 0 of the pair)
Img track_gray(of_ctx *c, const float *frame, int H, int W, int C) {
  Img gray = new_img(c, H, W, 2);
  uint32_t *mm = c->d_mm + 2 * 8;
  launch(c, "mm_init", k_mm_init, dim3(1), dim3(64), 0, mm, 1);
  Grid2 g = grid2(H, W);
  c->cur_px = (double)H * W;
  launch(c, "rgb_prep", k_rgb_prep<float>, g.grid, g.block, 0, frame, frame, H, W, C, gray.p, gray.P, gray.ps(),
         (float *)nullptr, (const uint32_t *)mm);
  return view(gray, 0, 1);
}

}  // namespace

extern "C" {

int of_track_advance(of_ctx *c, const float *fw, const float *bw, int H, int W, const of_track_opts *o, int n,
                     const float *xy_in, const uint8_t *status_in, float *xy_out, uint8_t *status_out) {
  API_BEGIN(c)
  REQUIRE(fw && bw && xy_in && status_in && xy_out && status_out && n >= 1, OF_EINVAL, "bad arguments");
  check_frame(H, W, "point tracking");
  check_track_opts(o);
  REQUIRE(n <= (1 << 24), OF_EINVAL, "at most 2^24 tracks");
  F2 f = upload_f2(c, fw, H, W), b = upload_f2(c, bw, H, W);
  float2 *dxy = upload_dense(c, (const float2 *)xy_in, n);
  uint8_t *dst = upload_dense(c, status_in, n);
  track_advance_dev(c, f, b, *o, n, dxy, dst, dxy, dst);
  download_dense(c, (float2 *)xy_out, dxy, n);
  download_dense(c, status_out, dst, n);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

int of_track_seed(of_ctx *c, const float *gray, int H, int W, const of_track_opts *o, int frame, int n,
                  const float *xy, const uint8_t *status, int32_t *n_new, int32_t *n_dropped, float *xy_new) {
  API_BEGIN(c)
  REQUIRE(gray && n_new && n_dropped && xy_new && frame >= 0, OF_EINVAL, "bad arguments");
  check_frame(H, W, "point tracking");
  check_track_opts(o);
  REQUIRE(n >= 0 && n <= o->max_tracks && (n == 0 || (xy && status)), OF_EINVAL,
          "the table must hold 0..max_tracks tracks");
  const SeedGrid g = seed_grid(H, W, o->step);
  const int room = std::min(o->max_tracks - n, g.ncells);
  Img G = upload_new_img(c, gray, H, W, 1);
  float2 *dxy = upload_dense(c, n > 0 ? (const float2 *)xy : nullptr, n);
  uint8_t *dst = upload_dense(c, n > 0 ? status : nullptr, n);
  uint8_t *occ = new_dense<uint8_t>(c, g.ncells), *flags = new_dense<uint8_t>(c, g.ncells);
  int *bcnt = new_dense<int>(c, g.nb + 1);
  float2 *dnew = new_dense<float2>(c, std::max(room, 1));
  const int total = track_seed_dev(c, G, *o, frame, n, dxy, dst, occ, flags, bcnt, room, dnew, nullptr, nullptr);
  *n_new = std::min(total, room);
  *n_dropped = total - *n_new;
  if (*n_new > 0) HIPCHK(hipMemcpy(xy_new, dnew, sizeof(float2) * *n_new, hipMemcpyDeviceToHost));
  API_END(c)
}

int of_tracks_open(of_ctx *c, const of_params *P, int H, int W, int C, const of_track_opts *o) {
  API_BEGIN(c)
  session_open<Tracker>(c, SES_TRACK, P, H, W, C, o, check_track_opts, [&](Tracker *t) {
    const SeedGrid g = seed_grid(H, W, o->step);
    t->alloc_frames(2);
    t->xy = t->alloc<float2>((size_t)o->max_tracks);
    t->status = t->alloc<uint8_t>((size_t)o->max_tracks);
    t->start = t->alloc<int32_t>((size_t)o->max_tracks);
    t->occ = t->alloc<uint8_t>((size_t)g.ncells);
    t->flags = t->alloc<uint8_t>((size_t)g.ncells);
    t->bcnt = t->alloc<int>((size_t)g.nb + 1);
  });
  API_END(c)
}

int of_tracks_push(of_ctx *c, const float *frame, float *out_fw, float *out_bw, uint8_t *state_fw, uint8_t *state_bw,
                   int32_t *n_tracks, int32_t *n_new, int32_t *n_dropped, of_stats *sf, of_stats *sb) {
  API_BEGIN(c)
  Tracker *t = session_get<Tracker>(c, SES_TRACK);
  REQUIRE(frame, OF_EINVAL, "bad arguments");
  const int H = t->H, W = t->W, C = t->C;
  const size_t px = (size_t)H * W;
  uint8_t *dsf = new_dense<uint8_t>(c, px, state_fw && t->frames > 0);
  uint8_t *dsb = new_dense<uint8_t>(c, px, state_bw && t->frames > 0);
  const PushPair p = session_push(c, t, frame, t->opt.alpha1, t->opt.alpha2, dsf, dsb, sf, sb);
  if (t->frames > 0) {
    if (t->n > 0) track_advance_dev(c, p.fw, p.bw, t->opt, t->n, t->xy, t->status, t->xy, t->status);
    if (out_fw) download_f2(c, p.fw, out_fw);
    if (out_bw) download_f2(c, p.bw, out_bw);
    download_dense(c, state_fw, dsf, px);
    download_dense(c, state_bw, dsb, px);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (sf) sf->total_ms = p.wall.ms();
  }
  const Img gray = track_gray(c, p.cur, H, W, C);
  const int room = t->opt.max_tracks - t->n;
  const int total = track_seed_dev(c, gray, t->opt, t->frames, t->n, t->xy, t->status, t->occ, t->flags, t->bcnt, room,
                                   t->xy + t->n, t->status + t->n, t->start + t->n);
  const int added = std::min(total, room);
  t->n += added;
  t->frames += 1;
  if (n_tracks) *n_tracks = t->n;
  if (n_new) *n_new = added;
  if (n_dropped) *n_dropped = total - added;
  API_END(c)
}

int of_tracks_read(of_ctx *c, int first, int n, float *xy, uint8_t *status, int32_t *start) {
  if (!c) return OF_EINVAL;
  try {
    Tracker *t = session_get<Tracker>(c, SES_TRACK);
    REQUIRE(first >= 0 && n >= 0 && first <= t->n && n <= t->n - first, OF_EINVAL, "tracks out of range");
    if (n == 0) return OF_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (xy) HIPCHK(hipMemcpy(xy, t->xy + first, sizeof(float2) * n, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, t->status + first, (size_t)n, hipMemcpyDeviceToHost));
    if (start) HIPCHK(hipMemcpy(start, t->start + first, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return OF_OK;
  }
  API_CATCH(c)
}

int of_tracks_close(of_ctx *c) { return session_close(c, SES_TRACK); }

}  // extern "C"
