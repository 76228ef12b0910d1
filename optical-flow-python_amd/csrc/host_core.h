// host_core.h — what every host part of the unity build (driver.hip) stands
// on: errors, the device arena, the context and its per-lane state, the
// tunables with their measurements, profiling, launch() and the API_* entry
// macros.  Included once, from driver.hip, after the kernel files.
namespace {

struct OfError {
  int code;
  std::string msg;
};

#define HIPCHK(x)                                                                                    \
  do {                                                                                               \
    hipError_t e_ = (x);                                                                             \
    if (e_ != hipSuccess) throw OfError{OF_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)
#define REQUIRE(cond, code, msg) \
  do {                           \
    if (!(cond)) throw OfError{code, msg}; \
  } while (0)

// the lanes' token for fine CG solves (BigPhase, host_flow.hip):
// OF_TOKEN_SLOTS solves may hold it at once
#ifndef OF_TOKEN_SLOTS
#define OF_TOKEN_SLOTS 2
#endif
struct Token {
  std::mutex m;
  std::condition_variable cv;
  int free = OF_TOKEN_SLOTS;
  void lock() {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return free > 0; });
    --free;
  }
  void unlock() {
    {
      std::lock_guard<std::mutex> l(m);
      ++free;
    }
    cv.notify_one();
  }
};

// grow-only device arena: chunks are kept across calls, offsets reset per call
struct Arena {
  struct Chunk {
    char *p;
    size_t cap, off;
  };
  std::vector<Chunk> chunks;
  void reset() {
    for (auto &c : chunks) c.off = 0;
  }
  void *alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    for (auto &c : chunks)
      if (c.cap - c.off >= bytes) {
        void *r = c.p + c.off;
        c.off += bytes;
        return r;
      }
    size_t cap = bytes > ((size_t)64 << 20) ? bytes : ((size_t)64 << 20);
    char *p = nullptr;
    HIPCHK(hipMalloc(&p, cap));
    chunks.push_back({p, cap, bytes});
    return p;
  }
  // offsets of the chunks now; rewind(mark) frees what was allocated since
  // (the caller has synchronised the stream that used it)
  std::vector<size_t> mark() const {
    std::vector<size_t> m;
    for (const auto &c : chunks) m.push_back(c.off);
    return m;
  }
  void rewind(const std::vector<size_t> &m) {
    for (size_t k = 0; k < chunks.size(); ++k) chunks[k].off = k < m.size() ? m[k] : 0;
  }
  void release() {
    for (auto &c : chunks) hipFree(c.p);
    chunks.clear();
  }
  size_t reserved() const {
    size_t n = 0;
    for (const auto &c : chunks) n += c.cap;
    return n;
  }
};

struct Img {  // C planar pitched fp32 planes
  float *p = nullptr;
  int H = 0, W = 0, P = 0, C = 0;
  size_t ps() const { return (size_t)H * P; }
  float *plane(int c) const { return p + (size_t)c * ps(); }
};
struct F2 {  // pitched float2 field
  float2 *p = nullptr;
  int H = 0, W = 0, P = 0;
};

struct ProfRec {
  const char *name;
  hipEvent_t e0, e1;
  double px;
};
struct KTime {
  double ms = 0, px = 0;
  int64_t n = 0;
};

struct Slot {
  void *rgb1 = nullptr, *rgb2 = nullptr;  // (H, W, C) fp32, or bytes when u8
  float *uv = nullptr;                    // dense planar 2 x H x W
  int H = 0, W = 0, C = 0;
  bool u8 = false;
  size_t cap_rgb = 0, cap_uv = 0;         // bytes of one frame, floats of uv
};

// of_pairs_run_host staging of one lane: two pinned input/output buffers and
// two device frame buffers, so pair j+1's bytes go up on the copy stream and
// pair j-1's flow comes down while pair j computes.  All lanes share the
// parent context's copy stream (`copy`, owned when own_copy): lanes + 1
// streams in all.  That fits GPU_MAX_HW_QUEUES (4) for lanes <= 3; the
// default 4 lanes oversubscribe it (5 streams, so two share a hardware queue
// and that lane's kernels and the copies queue behind each other), which was
// measured as a net gain all the same: 45.3 vs 44.4 pairs/s at 3 lanes
// (profiles/r3z_ab.log).  No copy waits on a lane's kernels inside the copy
// stream (the helper threads wait on the host).
struct HostStage {
  hipStream_t copy = nullptr;
  bool own_copy = false;
  uint8_t *pin_in[2] = {nullptr, nullptr}, *d_in[2] = {nullptr, nullptr};
  float *pin_out[2] = {nullptr, nullptr};
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_conv[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  size_t cap_in = 0, cap_out = 0;
};

// the streaming batch (of_pairs_open, batch.hip): a queued pair, and the pool
// of lanes that takes pairs from the queue
struct PairJob {
  const uint8_t *im1 = nullptr, *im2 = nullptr;  // host frames (of_pairs_submit) ...
  float *out = nullptr;
  int64_t ticket = 0;
  Slot dev;                  // ... or a device-resident slot (of_pairs_submit_slots)
  bool on_dev = false;
  int slot = -1;             // that slot's index
};

struct PairPool {
  int H = 0, W = 0, C = 0;
  of_params P;
  std::vector<of_ctx *> lanes;  // the ctx and its lane children (of_pairs_run's lanes), not owned
  of_progress_fn prog_fn = nullptr;  // the ctx's progress callback, off while the pool runs
  std::vector<float *> d_uv;  // 2 device flow buffers per lane
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  std::deque<PairJob> q;
  bool closing = false;
  int64_t next_ticket = 0;
  std::vector<uint8_t> done;  // by ticket
  std::map<int, int> busy;    // device slot -> its queued or running jobs (of_pairs_submit_slots)
  OfError err{OF_OK, ""};
};

// What the frame-sequence sessions of a context share (host_session.hip): the
// frame size, the parameters, a ring of the last frames, the delayed-emission
// state and the device allocations, which are the session's own and outlive
// the arena's per-call reset.  A context holds at most one of each kind.
// of_session_set_flow_scale names the first SES_SCALE_KINDS of them.
enum { SES_TRACK, SES_DENOISE, SES_STAB, SES_SR, SES_INPAINT, SES_MASKS, SES_CONSIST, SES_KINDS, SES_SCALE_KINDS = SES_SR };
struct Session {
  int H = 0, W = 0, C = 0;
  of_params P;        // as given at open; every push starts from a copy
  int frames = 0;     // frames pushed
  int next_out = 0;   // the next frame to emit (delayed emitters)
  bool flushed = false;
  std::vector<float *> frame;  // frame k at k % frame.size(): H x W x C dense
  std::vector<void *> owned;   // every device allocation of the session
  size_t bytes = 0;            // of all of them
  of_upsample_opts up = {1, 0, 0.0};  // of_session_set_flow_scale: scale > 1 estimates the pairs reduced
  virtual ~Session() = default;
  template <typename T>
  T *alloc(size_t count) {
    T *p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(T) * count));
    owned.push_back(p);
    bytes += sizeof(T) * count;
    return p;
  }
  void alloc_frames(int n) {
    for (int k = 0; k < n; ++k) frame.push_back(alloc<float>((size_t)H * W * C));
  }
};

// the point tracker (of_tracks_open, host_track.hip): a ring of 2 frames
struct Tracker : Session {
  of_track_opts opt;
  int n = 0;                     // tracks in the table
  float2 *xy = nullptr;          // the table: max_tracks entries each
  uint8_t *status = nullptr;
  int32_t *start = nullptr;
  uint8_t *occ = nullptr, *flags = nullptr;  // per cell
  int *bcnt = nullptr;                       // the cell kernels' block counts, then the total
};

// What the temporal denoiser and the super-resolver keep (host_fuse.hip): a
// ring of 2R+1 frames and rings of the last 2R adjacent pairs' flows and
// forward-backward states
struct PairRing : Session {
  int pitch = 0;
  float2 *fw[4] = {}, *bw[4] = {};         // pair (j, j+1) at j % 2R: pitched flows j -> j+1 and j+1 -> j
  uint8_t *sf[4] = {}, *sb[4] = {};        // their forward-backward states, H x W dense
};

// the temporal denoiser (of_denoise_open, host_fuse.hip)
struct Denoiser : PairRing {
  of_fuse_opts opt;
  // of_denoise_open_auto: sigma per emitted frame from the pair estimates
  // (host_noise.hip), kept on the host in the pairs' ring order
  bool auto_sigma = false;
  double floor = 0;                        // the smallest sigma a frame is fused with
  of_noise_estimate est[4] = {};           // pair (j, j+1) at j % 2R
  double last_sigma = 0;                   // what the last emitted frame was fused with
  bool emitted = false;
};

// the super-resolver (of_sr_open, host_sr.hip)
struct SuperResolver : PairRing {
  of_sr_opts opt;
};

// rows ilo .. ihi and columns jlo .. jhi of a frame, inclusive; empty when ihi < ilo
// (the bounding box the Poisson solver's window is built around, host_poisson.hip)
struct PsnBox {
  int ilo = 0, ihi = -1, jlo = 0, jhi = -1;
  bool empty() const { return ihi < ilo || jhi < jlo; }
};

// the inpainter (of_inpaint_open, host_inpaint.hip): rings of 2R+1 frames and
// grown masks and of the last 2R adjacent pairs' flows, R up to 16
struct Inpainter : Session {
  of_inpaint_opts opt;
  int pitch = 0;
  std::vector<uint8_t *> mask;     // the grown mask of frame k at k % (2R+1): H x W dense
  std::vector<float2 *> fw, bw;    // pair (j, j+1) at j % 2R: pitched flows j -> j+1 and j+1 -> j
  // of_inpaint_set_blend: every emitted frame is the blended fill
  bool blend = false;
  of_blend_opts bopt = {};
  std::vector<uint8_t *> mask1;    // the masks grown by one more, like `mask`
  std::vector<PsnBox> box;         // the grown mask's bounding box, taken on the host at the push, like `mask`
};

// the mask propagator (of_masks_open, host_mask.hip): a ring of 2 frames and
// the mask of the frame pushed last
struct MaskPropagator : Session {
  of_mask_opts opt;
  uint8_t *mask = nullptr;         // H x W dense, 0 / 1
};

// the temporal consistency session (of_consist_open, host_screen.hip): a ring
// of 2 frames and the output of the frame pushed last
struct Consistency : Session {
  of_consist_opts opt;
  int Cp = 0;                      // channels of the processed frames and the outputs
  float *out = nullptr;            // H x W x Cp dense
};

// the stabiliser (of_stab_open, host_motion.hip): a ring of R+1 frames; the
// motions between adjacent frames live on the host
struct Mat6 {
  double a[6];
};
struct Stabilizer : Session {
  of_stab_opts opt;
  std::deque<Mat6> motion;     // M_k at k - motion0, as kept (the identity where the fit's could not be inverted)
  int motion0 = 0;
};

}  // namespace

#define OF_SOLVE_RING 256
#define OF_SLOG_MAX 4096  // solve-log entries kept per context
// lanes mode: phases on levels of at least this many pixels hold the token
#define OF_BIG_PX (double)(1 << 20)
// SOR hand-off words: a ticket counter, then [2][SOR_MAXS] progress stamps
#define OF_SOR_SYNC_BYTES (256 + 2 * SOR_MAXS * sizeof(int))
// dynamic LDS of a k_sor_lex block: unused, it keeps one block per CU (the
// measured configuration of the sc1 hand-off, MI355X_MICROARCH.md)
#define OF_SOR_SHM (96 * 1024)
// k_sor_pipe: persistent grid of one wave per CU; sync words (ticket, fail,
// stop, counters, decisions, progress stamps) then per-strip partials and the
// decided sweeps' sums
// Round-4 A/B on config 2 (tools/ab/r4_sor_ab.sh, the same flow bitwise):
// publication interval / LDS per wave (waves per CU) / grid cap: 32 / 96 KB
// (1 per CU) / 256: 7.24 pairs/s; 8 / 96 KB / 256: 9.47; 8 / 32 KB / 512:
// 12.04; 16 / 32 KB / 512: 10.23; 32 / 32 KB / 512: 7.38.  Several waves per
// CU let the batch lanes' SOR grids run side by side; a short publication
// interval lets more sweeps overlap on the 1-2-strip coarse levels.
#ifndef OF_SOR_PIPE_WAVES
#define OF_SOR_PIPE_WAVES 512
#endif
// dynamic LDS of a k_sor_pipe wave (unused): bounds the waves per CU
// k_sor_wg only where its ring holds >= OF_SORW_MIN_RING sweeps: at 60x80
// (a ring of 3) it was slower than k_sor_pipe (37 vs 32 us per sweep), at
// 30x40 (ring 8) faster (11 vs 26 us; profiles/r6e)
#ifndef OF_SORW_MIN_RING
#define OF_SORW_MIN_RING 8
#endif
// k_sor_wg's sweep ring in LDS (the rest of the 160 KB holds its stamps)
#ifndef OF_SORW_RING_BYTES
#define OF_SORW_RING_BYTES (144 * 1024)
#endif
#ifndef OF_SOR_PIPE_SHM
#define OF_SOR_PIPE_SHM (32 * 1024)
#endif
#define OF_SORP_SYNC_BYTES (1024 + SOR_RING_MAX * 2 * SOR_MAXS * sizeof(int))
#define OF_SORP_BYTES (OF_SORP_SYNC_BYTES + (SOR_RING_MAX * 2 * SOR_MAXS * 2 + SOR_RING_MAX * 2) * sizeof(double))

// Streams are plain non-blocking streams, which the runtime maps onto its
// GPU_MAX_HW_QUEUES (4 on the box) hardware queues by creation order: batch
// lanes created after other streams of the same process came and went can
// share a queue with a busy lane and serialise (8 1080p pairs x 4 lanes:
// 47.0 pairs/s with a context's lanes created first, 43.1 with them created
// after a pair pool's lanes were destroyed on that context;
// tools/order_probe.py, profiles/r5_order_probe.log).  Streams created with a
// full CU mask behaved the same (the runtime pools them too).  Keep long-lived
// lanes: a context creates its of_pairs_run lanes once and keeps them.
static void create_stream(hipStream_t *s) { HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking)); }

// batch lanes created together on first use (ensure_lanes): the default 4
#ifndef OF_LANES_MIN
#define OF_LANES_MIN 4
#endif
#ifndef OF_FUSED_WARP_DEFAULT
#define OF_FUSED_WARP_DEFAULT 1
#endif
struct of_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  Arena arena;
  PcgState *d_state = nullptr, *h_state = nullptr;  // h_state: 2 pinned slots
  hipEvent_t ev_state[2] = {nullptr, nullptr};
  // CG solves: per-solve progress flags (mapped coherent host memory) and
  // copies of the final state (pinned), a ring of OF_SOLVE_RING; a solve's
  // statistics are read at the next stream synchronisation, so a CG solve
  // does not end in one
  CgFlag *h_flag = nullptr, *d_flag = nullptr;
  PcgState *h_ring = nullptr;
  int ring_next = 0;
  struct PendingSolve {
    int slot;
    double px;
    of_stats *st;
    const char *name;
  };
  std::vector<PendingSolve> pend;
  double *d_partials = nullptr;
  unsigned *d_sor_sync = nullptr;
  char *d_sorp = nullptr;  // k_sor_pipe sync words, partials (lazily allocated)
  // k_sor_pipe's ring of sweep buffers: one per context, grown to the largest
  // level seen (every SOR solve ends in a stream synchronisation, so the
  // ring is free again when the next solve starts)
  float2 *d_sor_ring = nullptr;
  size_t sor_ring_cap = 0;  // bytes
  int sor_fallbacks = 0;    // pipelined solves rerun per sweep (hand-off timeout)
  float *d_gather = nullptr;  // rank 0's RCCL gather receive buffer (grow-only)
  hipStream_t gstream = nullptr;  // the gather's own stream (of_rccl_gather_slots)
  size_t gather_cap = 0;
  // of_set_progress: display / per-stage report callback (never on batch lanes)
  of_progress_fn prog_fn = nullptr;
  void *prog_user = nullptr;
  int prog_flags = 0;
  int prog_stage = 0, prog_level = -1;
  std::chrono::steady_clock::time_point prog_t0;
  std::vector<float> prog_uv;  // host copy of a stage's flow (OF_PROGRESS_FLOW)
  // of_set_option(OF_OPT_SOR_PIPELINE): 2 (default) = k_sor_pipe, and
  // k_sor_wg where its LDS ring holds >= OF_SORW_MIN_RING sweeps
  int opt_sor_pipe = 2;
  int opt_fused_warp = OF_FUSED_WARP_DEFAULT;  // of_set_option(OF_OPT_FUSED_WARP)
  // solve log (of_set_solve_log): fp64 true residual of every solve
  int slog = 0;
  struct SolveLog {
    int h, w, solver, slot, iters, done;
    double est;
  };
  std::vector<SolveLog> slog_rec;
  int slog_idx = -1;       // log entry of the solve being issued (-1: none)
  bool slog_iter = false;  // ... whose iterate residual the solver logged itself
  double *d_rpart = nullptr, *d_rlog = nullptr;
  uint32_t *d_mm = nullptr;  // 32 min/max pairs
  NoiseSel *d_noise = nullptr;  // the noise estimators' selection words (lazily allocated)
  double *d_norm = nullptr, *h_norm = nullptr;
  int prof = 0;  // 0 off, 1 per kernel, 2 per kernel and level ("name@pixels")
  std::vector<hipEvent_t> ev_pool;  // profiling events
  size_t ev_used = 0;
  std::vector<hipEvent_t> tev_pool;  // level timing events, recycled per API call
  size_t tev_used = 0;
  std::vector<ProfRec> pending;
  std::map<std::string, KTime> ktimes;
  // profiling mode 3: every launch's [start, end] in ms after `epoch` (an
  // event on the parent context's stream; lanes share it)
  struct TlRec {
    const char *name;
    double px, t0, t1;
  };
  std::vector<TlRec> tl;
  hipEvent_t epoch = nullptr;
  bool own_epoch = false;
  std::map<int64_t, int> iter_hints;  // (H, W, solver) -> last iteration count
  double cur_px = 0;  // pixels processed by the launches being issued (profiling)
  std::vector<Slot> slots;
  HostStage *hs = nullptr;      // of_pairs_run_host staging (lazily created)
  PairPool *pool = nullptr;     // of_pairs_open streaming batch (lanes of its own)
  Session *session[SES_KINDS] = {};  // of_tracks_open, of_denoise_open, of_stab_open, of_sr_open, of_inpaint_open, of_masks_open, of_consist_open: one of each
  std::vector<of_ctx *> lanes;  // of_pairs_run pipelines: own stream, arena and solver state
  Token big_own;                // (parent) the big-phase token its lanes share
  Token *big = nullptr;         // (lane) token held through phases of >= big_px pixels
  double big_px = 0;
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
};

namespace {

// the next event of a grow-only pool that is recycled by resetting `used`
hipEvent_t next_event(std::vector<hipEvent_t> &pool, size_t &used) {
  if (used == pool.size()) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    pool.push_back(e);
  }
  return pool[used++];
}
hipEvent_t pool_event(of_ctx *c) { return next_event(c->ev_pool, c->ev_used); }
hipEvent_t timing_event(of_ctx *c) { return next_event(c->tev_pool, c->tev_used); }

void flush_prof(of_ctx *c) {
  if (c->pending.empty()) return;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto &r : c->pending) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
    auto &s = c->prof >= 2 ? c->ktimes[std::string(r.name) + "@" + std::to_string((long long)r.px)]
                           : c->ktimes[r.name];
    s.ms += ms;
    s.px += r.px;
    s.n += 1;
    if (c->prof == 3 && c->epoch) {
      float a = 0, b = 0;
      HIPCHK(hipEventElapsedTime(&a, c->epoch, r.e0));
      HIPCHK(hipEventElapsedTime(&b, c->epoch, r.e1));
      c->tl.push_back({r.name, r.px, a, b});
    }
  }
  c->pending.clear();
  c->ev_used = 0;
}

template <typename K, typename... A>
void launch(of_ctx *c, const char *name, K kernel, dim3 g, dim3 b, size_t shm, A... args) {
  if (g.x == 0 || g.y == 0 || g.z == 0) return;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->prof) {
    if (c->ev_used + 2 > 8192) flush_prof(c);
    e0 = pool_event(c);
    e1 = pool_event(c);
    HIPCHK(hipEventRecord(e0, c->stream));
  }
  hipLaunchKernelGGL(kernel, g, b, shm, c->stream, args...);
  HIPCHK(hipGetLastError());
  if (c->prof) {
    HIPCHK(hipEventRecord(e1, c->stream));
    c->pending.push_back({name, e0, e1, c->cur_px});
  }
}

inline dim3 gz(const Grid2 &g, int z) { return dim3(g.grid.x, g.grid.y, z); }

// host wall clock of a call, for of_stats::total_ms
struct WallClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

// ---- what the C entries return: the code, with the text kept for
// of_last_error (g_err: calls that have no context) ----
int fail(of_ctx *c, const OfError &e) {
  if (c) c->err = e.msg;
  return e.code;
}

thread_local std::string g_err;

// ---- argument checks several parts share ----
// the forward-backward thresholds
void check_alphas(double alpha1, double alpha2) {
  REQUIRE(std::isfinite(alpha1) && std::isfinite(alpha2) && alpha1 >= 0 && alpha2 >= 0, OF_EINVAL,
          "alpha1 and alpha2 must be finite and >= 0");
}
// a frame size whose pixel index fits 31 bits; `what` names who needs that
void check_frame(int H, int W, const char *what) {
  REQUIRE(H > 0 && W > 0, OF_EINVAL, "bad arguments");
  REQUIRE((size_t)H * W < ((size_t)1 << 31), OF_ENOTSUP, std::string(what) + " takes H * W < 2^31");
}

}  // namespace

// Entries that compute on the context refuse while a pair stream is open on
// it: the pool's lane 0 is the context itself, and these reset its arena and
// drain its pending solves (before the try: the error path clears them too)
#define API_BEGIN(ctx)            \
  if (!ctx) return OF_EINVAL;     \
  if (ctx->pool) return fail(ctx, OfError{OF_EINVAL, "a pair stream is open on this context (of_pairs_close first)"}); \
  try {                           \
    HIPCHK(hipSetDevice(ctx->device)); \
    ctx->arena.reset();            \
    ctx->tev_used = 0;
#define API_END(ctx)                         \
  if (!ctx->pend.empty()) {                  \
    HIPCHK(hipStreamSynchronize(ctx->stream)); \
    drain_solves(ctx);                       \
  }                                          \
  flush_prof(ctx);                           \
  return OF_OK;                              \
  }                                          \
  catch (const OfError &e) {                 \
    ctx->pending.clear();                    \
    ctx->pend.clear();                       \
    ctx->ev_used = 0;                        \
    return fail(ctx, e);                     \
  }                                          \
  catch (const std::exception &e) {          \
    return fail(ctx, OfError{OF_ENOMEM, e.what()}); \
  }
// the catch arms of an entry that leaves the context's pending work alone
#define API_CATCH(ctx)                              \
  catch (const OfError &e) {                        \
    return fail(ctx, e);                            \
  }                                                 \
  catch (const std::exception &e) {                 \
    return fail(ctx, OfError{OF_ENOMEM, e.what()}); \
  }
