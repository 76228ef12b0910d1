// host_session.hip — what the frame-sequence sessions of a context (point
// tracker, temporal denoiser, stabiliser, super-resolver, inpainter, mask
// propagator, temporal consistency: Session, host_core.h) share: the
// words of their messages, lookup and free, the open and push prologues, the
// bookkeeping of the delayed emitters and the switch to reduced-resolution
// pairs (of_session_set_flow_scale).
namespace {

// the words that differ between the sessions' messages
struct SessionKind {
  const char *name, *prefix, *topic;
};
const SessionKind SESSION_KIND[SES_KINDS] = {{"point tracker", "of_tracks_", "point tracking"},
                                             {"temporal denoiser", "of_denoise_", "temporal fusion"},
                                             {"stabiliser", "of_stab_", "global motion"},
                                             {"super-resolver", "of_sr_", "super-resolution"},
                                             {"inpainter", "of_inpaint_", "video inpainting"},
                                             {"mask propagator", "of_masks_", "mask propagation"},
                                             {"temporal consistency session", "of_consist_", "temporal consistency"}};

std::string session_not_open(int kind) {
  const SessionKind &K = SESSION_KIND[kind];
  return std::string("no ") + K.name + " is open on this context (" + K.prefix + "open first)";
}

// the open session of a kind
template <typename S>
S *session_get(of_ctx *c, int kind) {
  REQUIRE(c->session[kind], OF_EINVAL, session_not_open(kind));
  return static_cast<S *>(c->session[kind]);
}

void session_free(of_ctx *c, int kind) {
  Session *s = c->session[kind];
  if (!s) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (void *p : s->owned) hipFree(p);
  delete s;
  c->session[kind] = nullptr;
}

int session_close(of_ctx *c, int kind) {
  if (!c) return OF_EINVAL;
  if (!c->session[kind]) return fail(c, OfError{OF_EINVAL, session_not_open(kind)});
  session_free(c, kind);
  return OF_OK;
}

// Open a session of type S on frames H x W x C: the checks every open shares
// (`check` is the kind's own, of its options), then `alloc(S *)` makes the
// kind's device allocations; the session is freed again if that throws.
template <typename S, typename O, typename Alloc>
void session_open(of_ctx *c, int kind, const of_params *P, int H, int W, int C, const O *o, void (*check)(const O *),
                  Alloc alloc) {
  const SessionKind &K = SESSION_KIND[kind];
  REQUIRE(!c->session[kind], OF_EINVAL,
          std::string("a ") + K.name + " is open on this context (" + K.prefix + "close first)");
  REQUIRE(P, OF_EINVAL, "bad arguments");
  REQUIRE(C == 1 || C == 3, OF_EINVAL, "frames must be (H,W) or (H,W,3)");
  check_frame(H, W, K.topic);
  check(o);
  check_params(P);
  S *s = new S();
  c->session[kind] = s;
  try {
    s->H = H;
    s->W = W;
    s->C = C;
    s->P = *P;
    s->opt = *o;
    alloc(s);
  } catch (...) {
    session_free(c, kind);
    throw;
  }
}

// a push after a flush is refused
void session_not_flushed(const Session *s, int kind) {
  const SessionKind &K = SESSION_KIND[kind];
  REQUIRE(!s->flushed, OF_EINVAL,
          std::string("the ") + K.name + " has been flushed (" + K.prefix + "close, then open again)");
}

// The first half of a push: the caller's frame goes into its ring slot, and
// when there is a previous frame the pair (previous, this) is estimated in
// both directions from zero flows, at full resolution or, after
// of_session_set_flow_scale, reduced and upsampled (either way r.fw / r.bw and
// the states are full-resolution).  st_fw / st_bw: dense H x W device bytes
// for the forward-backward states, or nullptr; sf / sb: the passes' statistics
// (zeroed here), or nullptr.  fw.p is nullptr on the first frame.
struct PushPair {
  float *cur = nullptr;  // this frame on the device
  F2 fw, bw;             // previous -> this and back
  WallClock wall;        // started with the pair, for of_stats::total_ms
};
PushPair session_push(of_ctx *c, Session *s, const float *frame, double alpha1, double alpha2, uint8_t *st_fw,
                      uint8_t *st_bw, of_stats *sf, of_stats *sb) {
  const int H = s->H, W = s->W, C = s->C, k = s->frames, nf = (int)s->frame.size();
  PushPair r;
  r.cur = s->frame[k % nf];
  HIPCHK(hipMemcpyAsync(r.cur, frame, sizeof(float) * (size_t)H * W * C, hipMemcpyHostToDevice, c->stream));
  if (k == 0) return r;
  if (sf) memset(sf, 0, sizeof(*sf));
  if (sb) memset(sb, 0, sizeof(*sb));
  r.wall = WallClock();
  of_params P = s->P;
  if (s->up.scale > 1) {
    r.fw = new_f2(c, H, W);
    r.bw = new_f2(c, H, W);
    estimate_bidir_scaled_dev(c, &P, s->frame[(k - 1) % nf], r.cur, H, W, C, s->up, r.fw, r.bw, alpha1, alpha2, st_fw,
                              st_bw, sf, sb);
    return r;
  }
  r.fw = init_flow(c, nullptr, H, W);
  r.bw = init_flow(c, nullptr, H, W);
  estimate_bidir_dev(c, &P, s->frame[(k - 1) % nf], r.cur, H, W, C, r.fw, r.bw, alpha1, alpha2, st_fw, st_bw, sf, sb);
  return r;
}

// The frame a delayed emitter of radius R emits now, or -1: in a push (frame
// s->frames has just been stored) frame s->frames - R once it exists, in a
// flush step the next pending one.  Advances frames, next_out and flushed.
int session_next_emit(Session *s, int R, bool flush) {
  if (flush) {
    s->flushed = true;
    return s->next_out < s->frames ? s->next_out++ : -1;
  }
  const int k = s->frames++;
  if (k < R) return -1;
  s->next_out = k - R + 1;
  return k - R;
}

}  // namespace

extern "C" {

int of_session_set_flow_scale(of_ctx *c, int kinds, const of_upsample_opts *o) {
  if (!c) return OF_EINVAL;
  try {
    check_upsample_opts(o, true);
    REQUIRE(kinds > 0 && kinds < (1 << SES_SCALE_KINDS), OF_EINVAL, "kinds must name one or more of OF_SESSION_*");
    // every named session is checked before any is changed
    for (int kind = 0; kind < SES_SCALE_KINDS; ++kind) {
      if (!(kinds >> kind & 1)) continue;
      const Session *s = c->session[kind];
      REQUIRE(s, OF_EINVAL, session_not_open(kind));
      REQUIRE(s->frames < 2 && !s->flushed, OF_EINVAL,
              std::string("the ") + SESSION_KIND[kind].name +
                  " has estimated a pair already (set the flow scale before the second push)");
    }
    for (int kind = 0; kind < SES_SCALE_KINDS; ++kind)
      if (kinds >> kind & 1) c->session[kind]->up = o->scale == 1 ? of_upsample_opts{1, 0, 0.0} : *o;
    return OF_OK;
  }
  API_CATCH(c)
}

}  // extern "C"
