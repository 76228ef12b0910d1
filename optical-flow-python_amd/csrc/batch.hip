// batch.hip — many pairs on one context: the device-resident slots, the
// lanes (concurrent pipelines), of_pairs_run, of_pairs_run_host and its
// staging, the streaming pair pool, the slot copies and the RCCL gather.
namespace {

// ---- lanes ------------------------------------------------------------------
// The batch lanes (of_pairs_run, of_pairs_run_host, the pair pool) are the
// context itself (lane 0) and its child contexts (lanes 1..), created once,
// in one consecutive batch, and kept.  The runtime binds each stream to one of
// its GPU_MAX_HW_QUEUES (4) hardware queues when the stream is created: the
// first four streams of a process get four queues, later ones share them, so
// two busy lanes can end up on one queue and serialise (43 vs 47 pairs/s).
// rocprofv3's Queue_Id per lane thread (tools/queue_map.py,
// profiles/r5_queue_map_*.txt) showed it: lanes created and destroyed per
// pool, or a fifth lane stream, collided; the context's stream plus three
// children created right after it did not.  n = child lanes wanted.
void ensure_lanes(of_ctx *c, int n) {
  const int want = std::max(n, OF_LANES_MIN - 1);
  while ((int)c->lanes.size() < want) {
    of_ctx *l = nullptr;
    const int rc = of_ctx_create(c->device, &l);
    REQUIRE(rc == OF_OK, rc, "lane context: " + g_err);
    c->lanes.push_back(l);
  }
  // the gather / slot-copy stream (of_rccl_gather_slots, io_stream) right
  // after the lanes, for every run that has lanes: N = 1 and N > 1 map their
  // streams to hardware queues the same way (one created lazily at the first
  // gather, after the copy stream, would land on a busy lane's queue)
  if (!c->gstream) create_stream(&c->gstream);
}

of_ctx *lane_ctx(of_ctx *c, int li) { return li ? c->lanes[li - 1] : c; }

// A lane computes with its parent's options.  prof: a child lane's profiling
// mode (the parent's in the batch calls, which end in merge_lane_prof; 0 in
// the pool, whose children's tables nobody reads).  token_on: the lane's
// solves on levels of >= OF_BIG_PX pixels hold the parent's token (BigPhase).
// 8 1080p pairs, 2 lanes: 22.5 pairs/s with the token in three runs (16-18
// without; 20.5 with one lane) -- two lanes' fine-level CG kernels otherwise
// stall each other.
void configure_lane(of_ctx *parent, of_ctx *lane, int prof, bool token_on) {
  if (lane != parent) {
    lane->prof = prof;
    lane->epoch = parent->epoch;  // borrowed; read only when profiling (flush_prof)
  }
  lane->opt_sor_pipe = parent->opt_sor_pipe;
  lane->opt_fused_warp = parent->opt_fused_warp;
  lane->big = token_on && OF_BIG_PX > 0 ? &parent->big_own : nullptr;
  lane->big_px = OF_BIG_PX;
}

// profiling: the child lanes' timings into the ctx's table (lane 0, the ctx,
// records its own)
void merge_lane_prof(of_ctx *c, int lanes) {
  c->big = nullptr;
  for (int li = 1; li < lanes; ++li) {
    of_ctx *l = c->lanes[li - 1];
    for (auto &kv : l->ktimes) {
      KTime &d = c->ktimes[kv.first];
      d.ms += kv.second.ms;
      d.px += kv.second.px;
      d.n += kv.second.n;
    }
    l->ktimes.clear();
    c->tl.insert(c->tl.end(), l->tl.begin(), l->tl.end());
    l->tl.clear();
  }
}

// body(lane, li) on one host thread per configured lane; joins them, merges
// the children's profiles and rethrows the first lane's error.  A failed
// lane's stream (and, with sync_copy, its staging copy stream) is drained
// before its thread ends.
template <typename Body>
void run_lanes(of_ctx *c, int lanes, bool sync_copy, Body body) {
  std::vector<std::thread> th;
  std::vector<OfError> errs(lanes, OfError{OF_OK, ""});
  for (int li = 0; li < lanes; ++li) {
    of_ctx *l = lane_ctx(c, li);
    th.emplace_back([=, &errs] {
      try {
        HIPCHK(hipSetDevice(l->device));
        body(l, li);
        if (l != c) flush_prof(l);
      } catch (const OfError &e) {
        errs[li] = e;
        hipStreamSynchronize(l->stream);
        if (sync_copy && l->hs) hipStreamSynchronize(l->hs->copy);
        l->pending.clear();
        l->ev_used = 0;
      } catch (const std::exception &e) {
        errs[li] = OfError{OF_ENOMEM, e.what()};
      }
    });
  }
  for (auto &t : th) t.join();
  merge_lane_prof(c, lanes);
  for (auto &e : errs)
    if (e.code != OF_OK) throw e;
}

// ---- device-resident slots ---------------------------------------------------
void slot_reserve_uv(Slot &s, size_t nu) {
  if (s.cap_uv >= nu) return;
  hipFree(s.uv);
  HIPCHK(hipMalloc(&s.uv, sizeof(float) * nu));
  s.cap_uv = nu;
}

// ---- of_pairs_run_host and its staging --------------------------------------
void stage_alloc(of_ctx *l, of_ctx *parent, size_t in_bytes, size_t out_floats) {
  if (!l->hs) {
    l->hs = new HostStage();
    if (l == parent) {
      create_stream(&l->hs->copy);
      l->hs->own_copy = true;
    }
    for (int b = 0; b < 2; ++b) {
      HIPCHK(hipEventCreateWithFlags(&l->hs->ev_in[b], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&l->hs->ev_conv[b], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&l->hs->ev_out[b], hipEventDisableTiming));
    }
  }
  HostStage &h = *l->hs;
  if (!h.own_copy) h.copy = parent->hs->copy;
  if (h.cap_in < in_bytes) {
    for (int b = 0; b < 2; ++b) {
      HIPCHK(hipEventSynchronize(h.ev_in[b]));
      HIPCHK(hipEventSynchronize(h.ev_conv[b]));
      if (h.pin_in[b]) hipHostFree(h.pin_in[b]);
      hipFree(h.d_in[b]);
      HIPCHK(hipHostMalloc((void **)&h.pin_in[b], in_bytes, hipHostMallocDefault));
      HIPCHK(hipMalloc((void **)&h.d_in[b], in_bytes));
    }
    h.cap_in = in_bytes;
  }
  if (h.cap_out < out_floats) {
    for (int b = 0; b < 2; ++b) {
      HIPCHK(hipEventSynchronize(h.ev_out[b]));
      if (h.pin_out[b]) hipHostFree(h.pin_out[b]);
      HIPCHK(hipHostMalloc((void **)&h.pin_out[b], sizeof(float) * out_floats, hipHostMallocDefault));
    }
    h.cap_out = out_floats;
  }
}

void stage_free(of_ctx *l) {
  if (!l->hs) return;
  HostStage &h = *l->hs;
  for (int b = 0; b < 2; ++b)
    for (hipEvent_t e : {h.ev_in[b], h.ev_out[b]})
      if (e) hipEventSynchronize(e);
  for (int b = 0; b < 2; ++b) {
    if (h.pin_in[b]) hipHostFree(h.pin_in[b]);
    if (h.pin_out[b]) hipHostFree(h.pin_out[b]);
    hipFree(h.d_in[b]);
    for (hipEvent_t e : {h.ev_in[b], h.ev_conv[b], h.ev_out[b]})
      if (e) hipEventDestroy(e);
  }
  if (h.own_copy && h.copy) {
    hipStreamSynchronize(h.copy);
    hipStreamDestroy(h.copy);
  }
  delete l->hs;
  l->hs = nullptr;
}

// a pair's uint8 frames: host -> pinned buffer b -> device buffer b on the
// copy stream
void stage_in(HostStage &h, int b, const uint8_t *im1, const uint8_t *im2, size_t nb) {
  HIPCHK(hipEventSynchronize(h.ev_in[b]));  // pinned buffer b free (its last H2D done)
  memcpy(h.pin_in[b], im1, nb);
  memcpy(h.pin_in[b] + nb, im2, nb);
  HIPCHK(hipEventSynchronize(h.ev_conv[b]));  // device buffer b no longer read (its last pair done)
  HIPCHK(hipMemcpyAsync(h.d_in[b], h.pin_in[b], 2 * nb, hipMemcpyHostToDevice, h.copy));
  HIPCHK(hipEventRecord(h.ev_in[b], h.copy));
}
// the flow of buffer b's pair: wait for its kernels on the host, then D2H on
// the shared copy stream into pinned buffer b and out to the caller
void stage_out(HostStage &h, int b, const float *src_dev, float *dst_host, size_t nu) {
  HIPCHK(hipEventSynchronize(h.ev_conv[b]));
  HIPCHK(hipMemcpyAsync(h.pin_out[b], src_dev, sizeof(float) * nu, hipMemcpyDeviceToHost, h.copy));
  HIPCHK(hipEventRecord(h.ev_out[b], h.copy));
  HIPCHK(hipEventSynchronize(h.ev_out[b]));
  memcpy(dst_host, h.pin_out[b], sizeof(float) * nu);
}
// the pair staged in device buffer b as a slot whose flow goes to `uv`
Slot staged_slot(const HostStage &h, int b, size_t nb, float *uv, int H, int W, int C) {
  Slot s;
  s.rgb1 = h.d_in[b];
  s.rgb2 = h.d_in[b] + nb;
  s.u8 = true;
  s.uv = uv;
  s.H = H;
  s.W = W;
  s.C = C;
  return s;
}

// One lane's share of of_pairs_run_host: pairs k = first, first + step, ...
// Per pair j (buffer b = j & 1): host bytes -> pinned -> device on the copy
// stream (issued while pair j-1 computes), estimate_flow on the lane stream
// straight from the bytes, flow -> slot k's device buffer (kept for the RCCL
// gather) -> pinned on the copy stream -> caller's buffer (while pair j+1
// computes).
void run_host_lane(of_ctx *c, of_ctx *l, int first, int step, int npairs, const uint8_t *const *im1,
                   const uint8_t *const *im2, int H, int W, int C, const of_params *P, float *const *out_uv,
                   of_stats *st) {
  HostStage &h = *l->hs;
  const size_t nb = (size_t)H * W * C, nu = 2 * (size_t)H * W;
  std::vector<int> ks;
  for (int k = first; k < npairs; k += step) ks.push_back(k);
  auto prefetch = [&](int j) { stage_in(h, j & 1, im1[ks[j]], im2[ks[j]], nb); };
  auto finish = [&](int j) { stage_out(h, j & 1, c->slots[ks[j]].uv, out_uv[ks[j]], nu); };
  // the host copies of pair j+1 (in) and pair j-1 (out) run on a helper
  // thread while this thread drives pair j's kernels
  std::thread io;
  OfError io_err{OF_OK, ""};
  auto join_io = [&] {
    if (io.joinable()) io.join();
    if (io_err.code != OF_OK) throw io_err;
  };
  if (!ks.empty()) prefetch(0);
  for (int j = 0; j < (int)ks.size(); ++j) {
    const int b = j & 1, k = ks[j];
    join_io();
    l->arena.reset();
    l->tev_used = 0;
    HIPCHK(hipStreamWaitEvent(l->stream, h.ev_in[b], 0));
    const Slot s = staged_slot(h, b, nb, c->slots[k].uv, H, W, C);
    io = std::thread([&, j] {
      try {
        HIPCHK(hipSetDevice(l->device));
        if (j + 1 < (int)ks.size()) prefetch(j + 1);
        if (j) finish(j - 1);
      } catch (const OfError &e) {
        io_err = e;
      }
    });
    try {
      of_params Pc = *P;
      run_slot(l, s, &Pc, k == 0 ? st : nullptr);
    } catch (...) {
      if (io.joinable()) io.join();
      throw;
    }
    HIPCHK(hipEventRecord(h.ev_conv[b], l->stream));  // frames of buffer b consumed, flow k complete
  }
  join_io();
  if (!ks.empty()) finish((int)ks.size() - 1);
}
}  // namespace

extern "C" {

int of_pair_run(of_ctx *c, int slot, of_params *P, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(slot >= 0 && slot < (int)c->slots.size() && c->slots[slot].rgb1, OF_EINVAL, "slot not uploaded");
  run_slot(c, c->slots[slot], P, st);
  API_END(c)
}

// Slots 0..nslots-1 on `lanes` concurrent pipelines.  Each lane is a child
// context (own non-blocking stream, arena, CG state and host progress flag)
// driven by its own host thread; slot s runs on lane s % lanes, so while one
// pair is in a latency-bound phase (coarse levels, solver feed, host syncs)
// another pair's kernels fill the CUs.  Every kernel is deterministic, so a
// slot's flow does not depend on the lane count.  lanes == 1 runs the slots
// in order on the ctx's own stream.
int of_pairs_run(of_ctx *c, int nslots, const of_params *P, int lanes, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(P && nslots >= 1 && nslots <= (int)c->slots.size() && lanes >= 1 && lanes <= 16, OF_EINVAL,
          "bad arguments");
  for (int s = 0; s < nslots; ++s) REQUIRE(c->slots[s].rgb1 && c->slots[s].uv, OF_EINVAL, "slot not uploaded");
  REQUIRE(!c->pool, OF_EINVAL, "a pair stream is open on this context (of_pairs_close first)");
  ProgressOff quiet(c);  // batch entries never report
  lanes = std::min(lanes, nslots);
  if (lanes == 1) {
    for (int s = 0; s < nslots; ++s) {
      if (s) {
        c->arena.reset();
        c->tev_used = 0;
      }
      of_params Pc = *P;
      run_slot(c, c->slots[s], &Pc, s == 0 ? st : nullptr);
    }
  } else {
    // lane 0 is the ctx itself, lanes 1.. its long-lived children (ensure_lanes)
    ensure_lanes(c, lanes - 1);
    for (int li = 0; li < lanes; ++li) configure_lane(c, lane_ctx(c, li), c->prof, true);
    run_lanes(c, lanes, false, [=](of_ctx *l, int li) {
      for (int s = li; s < nslots; s += lanes) {
        l->arena.reset();
        l->tev_used = 0;
        of_params Pc = *P;
        run_slot(l, c->slots[s], &Pc, s == 0 ? st : nullptr);
      }
    });
  }
  API_END(c)
}

// Host-to-host batch (SURVEY.md §8d headline: wall clock including the H2D of
// the uint8 pair and the D2H of uv): pairs are read from caller-owned (H, W, C)
// uint8 frames and the flows written to caller-owned planar 2 x H x W fp32
// buffers, `lanes` pairs in flight as in of_pairs_run.  Slots 0..npairs-1 keep
// each pair's flow on the device afterwards (of_rccl_gather_flows,
// of_pair_download).
int of_pairs_run_host(of_ctx *c, int npairs, const uint8_t *const *im1, const uint8_t *const *im2, int H, int W,
                      int C, const of_params *P, int lanes, float *const *out_uv, of_stats *st) {
  API_BEGIN(c)
  REQUIRE(P && im1 && im2 && out_uv && npairs >= 1 && npairs <= 4096 && H > 0 && W > 0 && (C == 1 || C == 3) &&
              lanes >= 1 && lanes <= 16,
          OF_EINVAL, "bad arguments");
  for (int k = 0; k < npairs; ++k) REQUIRE(im1[k] && im2[k] && out_uv[k], OF_EINVAL, "null pair buffer");
  REQUIRE(!c->pool, OF_EINVAL, "a pair stream is open on this context (of_pairs_close first)");
  ProgressOff quiet(c);  // batch entries never report
  if ((int)c->slots.size() < npairs) c->slots.resize(npairs);
  const size_t nu = 2 * (size_t)H * W;
  for (int k = 0; k < npairs; ++k) {
    Slot &s = c->slots[k];
    slot_reserve_uv(s, nu);
    // the slot now holds this batch's flow; frames of an earlier
    // of_pair_upload (possibly of another size) are dropped so that
    // of_pair_run / of_pairs_run refuse the slot until it is re-uploaded
    if (s.rgb1 || s.rgb2) {
      HIPCHK(hipStreamSynchronize(c->stream));
      hipFree(s.rgb1);
      hipFree(s.rgb2);
      s.rgb1 = s.rgb2 = nullptr;
      s.cap_rgb = 0;
    }
    s.H = H;
    s.W = W;
    s.C = C;
  }
  lanes = std::min(lanes, npairs);
  if (lanes > 1) ensure_lanes(c, lanes - 1);  // lane streams before the copy stream (ensure_lanes)
  for (int li = 0; li < lanes; ++li) stage_alloc(lane_ctx(c, li), c, 2 * (size_t)H * W * C, nu);
  if (lanes == 1) {
    run_host_lane(c, c, 0, 1, npairs, im1, im2, H, W, C, P, out_uv, st);
  } else {
    for (int li = 0; li < lanes; ++li) configure_lane(c, lane_ctx(c, li), c->prof, true);
    run_lanes(c, lanes, true, [=](of_ctx *l, int li) {
      run_host_lane(c, l, li, lanes, npairs, im1, im2, H, W, C, P, out_uv, st);
    });
  }
  API_END(c)
}

}  // extern "C"

// ---- streaming batch: a persistent pool of lanes fed from a queue --------
namespace {
// a slot queued to the pair pool and not yet finished
bool pool_slot_busy(of_ctx *c, int slot) {
  PairPool *pp = c->pool;
  if (!pp) return false;
  std::lock_guard<std::mutex> lk(pp->m);
  auto it = pp->busy.find(slot);
  return it != pp->busy.end() && it->second > 0;
}

void pool_set_progress(PairPool *pp, of_progress_fn fn) { pp->prog_fn = fn; }

// with pp->m held: the code a submission is refused with (OF_OK: accepted)
int pool_refuses(of_ctx *c, PairPool *pp) {
  if (pp->err.code != OF_OK) {
    c->err = pp->err.msg;
    return pp->err.code;
  }
  if (pp->closing) c->err = "pair stream closing";
  return pp->closing ? OF_EINVAL : OF_OK;
}

// One lane of the pool: the per-pair pipeline of run_host_lane (pinned and
// device double buffers, H2D of the next pair and D2H of the previous one on
// a helper thread while this thread drives a pair's kernels), but pairs come
// from the pool's queue as they are submitted, so a lane never drains between
// the caller's chunks.  A pair's flow is written out as soon as no next pair
// is waiting, so of_pairs_wait never waits for a later submission.
void pool_lane(of_ctx *c, PairPool *pp, int li) {
  of_ctx *l = pp->lanes[li];
  HostStage &h = *l->hs;
  const int H = pp->H, W = pp->W, C = pp->C;
  const size_t nb = (size_t)H * W * C, nu = 2 * (size_t)H * W;
  float *duv[2] = {pp->d_uv[2 * li], pp->d_uv[2 * li + 1]};
  auto pop = [&](PairJob &j, const bool *stop) {
    std::unique_lock<std::mutex> lk(pp->m);
    pp->cv_job.wait(lk, [&] { return !pp->q.empty() || pp->closing || (stop && *stop); });
    if (pp->q.empty()) return false;
    j = pp->q.front();
    pp->q.pop_front();
    return true;
  };
  auto prefetch = [&](int b, const PairJob &j) {
    if (!j.on_dev) stage_in(h, b, j.im1, j.im2, nb);  // else: frames already in HBM
  };
  auto finish = [&](int b, const PairJob &j) {
    if (j.on_dev) HIPCHK(hipEventSynchronize(h.ev_conv[b]));  // a device slot's flow stays in its slot
    else stage_out(h, b, duv[b], j.out, nu);
    {
      std::lock_guard<std::mutex> lk(pp->m);
      if (j.on_dev) --pp->busy[j.slot];
      pp->done[j.ticket] = 1;
    }
    pp->cv_done.notify_all();
  };
  PairJob jobs[2];
  if (!pop(jobs[0], nullptr)) return;
  prefetch(0, jobs[0]);
  int b = 0, pending = -1;  // pending: buffer of a computed pair not yet written out
  for (;;) {
    l->arena.reset();
    l->tev_used = 0;
    Slot s;
    if (jobs[b].on_dev) {
      s = jobs[b].dev;
    } else {
      HIPCHK(hipStreamWaitEvent(l->stream, h.ev_in[b], 0));
      s = staged_slot(h, b, nb, duv[b], H, W, C);
    }
    bool computed = false, got = false;
    OfError io_err{OF_OK, ""};
    std::thread io([&, b, pending] {
      try {
        HIPCHK(hipSetDevice(l->device));
        if (pending >= 0) finish(pending, jobs[pending]);
        got = pop(jobs[b ^ 1], &computed);
        if (got) prefetch(b ^ 1, jobs[b ^ 1]);
      } catch (const OfError &e) {
        io_err = e;
      }
    });
    auto release_io = [&] {
      {
        std::lock_guard<std::mutex> lk(pp->m);
        computed = true;
      }
      pp->cv_job.notify_all();
      io.join();
    };
    try {
      of_params Pc = pp->P;
      run_slot(l, s, &Pc, nullptr);
      HIPCHK(hipEventRecord(h.ev_conv[b], l->stream));
    } catch (...) {
      release_io();
      throw;
    }
    release_io();
    if (io_err.code != OF_OK) throw io_err;
    pending = b;
    if (!got) {
      finish(b, jobs[b]);
      pending = -1;
      if (!pop(jobs[b ^ 1], nullptr)) return;
      prefetch(b ^ 1, jobs[b ^ 1]);
    }
    b ^= 1;
  }
}

// ---- slot copies ----------------------------------------------------------------
// of_pair_upload / of_pair_download may run while the pair pool computes on
// the context: no arena, no pending solves, and a stream of their own when a
// pool is open (the gather's, which exists whenever a pool is open:
// of_pairs_open creates it with the lanes, ensure_lanes)
hipStream_t io_stream(of_ctx *c) { return c->pool ? c->gstream : c->stream; }
}  // namespace

extern "C" {

// Streaming batch (host I/O overlapped with the GPU):
// of_pairs_open starts `lanes` pipelines (child contexts, one host thread
// each) that take (H, W, C) uint8 pairs from a queue; of_pairs_submit queues
// pairs and returns at once; of_pairs_wait blocks until a pair's flow is in
// the caller's buffer.  Flows equal of_pairs_run_host's with the same lanes
// (bitwise): lanes == 1 keeps estimate_flow's geometry, lanes >= 2 share the
// fine-solve token (two pairs' fine CG solves side by side).
int of_pairs_open(of_ctx *c, int H, int W, int C, const of_params *P, int lanes) {
  API_BEGIN(c)
  REQUIRE(!c->pool, OF_EINVAL, "a pair stream is already open on this context");
  REQUIRE(P && H > 0 && W > 0 && (C == 1 || C == 3) && lanes >= 1 && lanes <= 16, OF_EINVAL, "bad arguments");
  check_params(P);
  std::unique_ptr<PairPool> pp(new PairPool());
  pp->H = H;
  pp->W = W;
  pp->C = C;
  pp->P = *P;
  const size_t nu = 2 * (size_t)H * W;
  ensure_lanes(c, lanes - 1);  // lane streams before the copy stream (ensure_lanes)
  try {
    // the pool runs on the context's long-lived lane children (the ones
    // of_pairs_run / of_pairs_run_host use): lanes created and destroyed per
    // pool would shift the runtime's stream -> hardware-queue mapping for
    // the lanes created after them (create_stream)
    for (int li = 0; li < lanes; ++li) {
      of_ctx *l = lane_ctx(c, li);
      pp->lanes.push_back(l);
      configure_lane(c, l, 0, lanes > 1);
      stage_alloc(l, c, 2 * (size_t)H * W * C, nu);
      for (int b = 0; b < 2; ++b) {
        float *d = nullptr;
        HIPCHK(hipMalloc(&d, sizeof(float) * nu));
        pp->d_uv.push_back(d);
      }
    }
  } catch (...) {
    for (float *d : pp->d_uv) hipFree(d);
    throw;
  }
  PairPool *raw = pp.release();
  c->pool = raw;
  raw->prog_fn = c->prog_fn;  // lane 0 is the ctx: batch lanes never report
  c->prog_fn = nullptr;
  for (int li = 0; li < lanes; ++li)
    raw->th.emplace_back([c, raw, li] {
      try {
        HIPCHK(hipSetDevice(raw->lanes[li]->device));
        pool_lane(c, raw, li);
      } catch (const OfError &e) {
        std::lock_guard<std::mutex> lk(raw->m);
        if (raw->err.code == OF_OK) raw->err = e;
        raw->closing = true;
      } catch (const std::exception &e) {
        std::lock_guard<std::mutex> lk(raw->m);
        if (raw->err.code == OF_OK) raw->err = OfError{OF_ENOMEM, e.what()};
        raw->closing = true;
      }
      raw->cv_done.notify_all();
      raw->cv_job.notify_all();
    });
  API_END(c)
}

// queue n pairs (caller-owned (H, W, C) uint8 frames and planar 2 x H x W fp32
// outputs, all kept alive until waited for); tickets first .. first + n - 1
int of_pairs_submit(of_ctx *c, int n, const uint8_t *const *im1, const uint8_t *const *im2, float *const *out_uv,
                    int64_t *first_ticket) {
  if (!c) return OF_EINVAL;
  PairPool *pp = c->pool;
  if (!pp || n < 1 || !im1 || !im2 || !out_uv) {
    c->err = pp ? "bad arguments" : "no pair stream open (of_pairs_open)";
    return OF_EINVAL;
  }
  for (int k = 0; k < n; ++k)
    if (!im1[k] || !im2[k] || !out_uv[k]) {
      c->err = "null pair buffer";
      return OF_EINVAL;
    }
  {
    std::lock_guard<std::mutex> lk(pp->m);
    if (const int rc = pool_refuses(c, pp)) return rc;
    if (first_ticket) *first_ticket = pp->next_ticket;
    for (int k = 0; k < n; ++k) {
      PairJob j;
      j.im1 = im1[k];
      j.im2 = im2[k];
      j.out = out_uv[k];
      j.ticket = pp->next_ticket++;
      pp->q.push_back(j);
      pp->done.push_back(0);
    }
  }
  pp->cv_job.notify_all();
  return OF_OK;
}

// queue n device-resident pairs (slots of this context, of_pair_upload); each
// flow stays in its slot.  A slot is read and written by the lane that takes
// it, so it must not be submitted again (or re-uploaded) before its ticket is
// waited for.
int of_pairs_submit_slots(of_ctx *c, int n, const int *slots, int64_t *first_ticket) {
  if (!c) return OF_EINVAL;
  PairPool *pp = c->pool;
  if (!pp || n < 1 || !slots) {
    c->err = pp ? "bad arguments" : "no pair stream open (of_pairs_open)";
    return OF_EINVAL;
  }
  for (int k = 0; k < n; ++k) {
    const int sl = slots[k];
    if (sl < 0 || sl >= (int)c->slots.size() || !c->slots[sl].rgb1 || !c->slots[sl].uv) {
      c->err = "slot not uploaded";
      return OF_EINVAL;
    }
    if (c->slots[sl].H != pp->H || c->slots[sl].W != pp->W) {
      c->err = "slot frame size differs from the stream's";
      return OF_EINVAL;
    }
  }
  {
    std::lock_guard<std::mutex> lk(pp->m);
    if (const int rc = pool_refuses(c, pp)) return rc;
    for (int k = 0; k < n; ++k) {
      auto it = pp->busy.find(slots[k]);
      int dup = 0;
      for (int q = 0; q < k; ++q) dup += slots[q] == slots[k];
      if ((it != pp->busy.end() && it->second > 0) || dup) {
        c->err = "slot already queued in the pair stream (of_pairs_wait its ticket first)";
        return OF_EINVAL;
      }
    }
    if (first_ticket) *first_ticket = pp->next_ticket;
    for (int k = 0; k < n; ++k) {
      PairJob j;
      j.ticket = pp->next_ticket++;
      j.dev = c->slots[slots[k]];
      j.on_dev = true;
      j.slot = slots[k];
      ++pp->busy[slots[k]];
      pp->q.push_back(j);
      pp->done.push_back(0);
    }
  }
  pp->cv_job.notify_all();
  return OF_OK;
}

// block until pair `ticket`'s flow has been written (a lane's error is
// returned here, and by every later call)
int of_pairs_wait(of_ctx *c, int64_t ticket) {
  if (!c) return OF_EINVAL;
  PairPool *pp = c->pool;
  if (!pp) {
    c->err = "no pair stream open (of_pairs_open)";
    return OF_EINVAL;
  }
  std::unique_lock<std::mutex> lk(pp->m);
  if (ticket < 0 || ticket >= pp->next_ticket) {
    c->err = "unknown ticket";
    return OF_EINVAL;
  }
  pp->cv_done.wait(lk, [&] { return pp->done[ticket] || pp->err.code != OF_OK; });
  if (!pp->done[ticket]) {
    c->err = pp->err.msg;
    return pp->err.code;
  }
  return OF_OK;
}

// finish every queued pair, stop the lanes and release them
int of_pairs_close(of_ctx *c) {
  if (!c) return OF_EINVAL;
  PairPool *pp = c->pool;
  if (!pp) return OF_OK;
  {
    std::lock_guard<std::mutex> lk(pp->m);
    pp->closing = true;
  }
  pp->cv_job.notify_all();
  for (auto &t : pp->th) t.join();
  for (of_ctx *l : pp->lanes) {  // the lanes stay with the context
    l->big = nullptr;
    l->arena.reset();
  }
  c->prog_fn = pp->prog_fn;
  hipSetDevice(c->device);
  for (float *d : pp->d_uv) hipFree(d);
  const OfError e = pp->err;
  delete pp;
  c->pool = nullptr;
  if (e.code != OF_OK) {
    c->err = e.msg;
    return e.code;
  }
  return OF_OK;
}

#define API_BEGIN_IO(ctx)               \
  if (!ctx) return OF_EINVAL;           \
  try {                                 \
    HIPCHK(hipSetDevice(ctx->device));  \
    hipStream_t ios = io_stream(ctx);
#define API_END_IO(ctx) \
  return OF_OK;         \
  }                     \
  API_CATCH(ctx)

int of_pair_upload(of_ctx *c, int slot, const float *im1, const float *im2, int H, int W, int C) {
  API_BEGIN_IO(c)
  REQUIRE(slot >= 0 && slot < 4096 && im1 && im2 && (C == 1 || C == 3), OF_EINVAL, "bad arguments");
  REQUIRE(!pool_slot_busy(c, slot), OF_EINVAL, "slot is queued in the pair stream (of_pairs_wait its ticket first)");
  if ((int)c->slots.size() <= slot) c->slots.resize(slot + 1);
  Slot &s = c->slots[slot];
  const size_t n = (size_t)H * W * C * sizeof(float);
  if (s.cap_rgb < n) {
    hipFree(s.rgb1);
    hipFree(s.rgb2);
    HIPCHK(hipMalloc(&s.rgb1, n));
    HIPCHK(hipMalloc(&s.rgb2, n));
    s.cap_rgb = n;
  }
  slot_reserve_uv(s, 2 * (size_t)H * W);
  s.H = H;
  s.W = W;
  s.C = C;
  s.u8 = false;
  HIPCHK(hipMemcpyAsync(s.rgb1, im1, n, hipMemcpyHostToDevice, ios));
  HIPCHK(hipMemcpyAsync(s.rgb2, im2, n, hipMemcpyHostToDevice, ios));
  HIPCHK(hipStreamSynchronize(ios));
  API_END_IO(c)
}

int of_pair_download(of_ctx *c, int slot, float *out_uv) {
  API_BEGIN_IO(c)
  REQUIRE(slot >= 0 && slot < (int)c->slots.size() && c->slots[slot].uv && out_uv, OF_EINVAL, "bad slot");
  REQUIRE(!pool_slot_busy(c, slot), OF_EINVAL, "slot is queued in the pair stream (of_pairs_wait its ticket first)");
  Slot &s = c->slots[slot];
  HIPCHK(hipMemcpyAsync(out_uv, s.uv, sizeof(float) * 2 * (size_t)s.H * s.W, hipMemcpyDeviceToHost, ios));
  HIPCHK(hipStreamSynchronize(ios));
  API_END_IO(c)
}

// ---- RCCL gather: one process per GPU ----
int of_rccl_unique_id(char *out128) {
  if (!out128) return OF_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return OF_ERCCL;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(out128, &id, 128);
  return OF_OK;
}

int of_rccl_init(of_ctx *c, const char *id128, int nranks, int rank) {
  API_BEGIN(c)
  REQUIRE(id128 && nranks >= 1 && rank >= 0 && rank < nranks, OF_EINVAL, "bad arguments");
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ensure_lanes(c, 0);  // the lanes and the gather stream, in the order a pool would create them
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
  REQUIRE(r == ncclSuccess, OF_ERCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  c->nranks = nranks;
  c->rank = rank;
  API_END(c)
}

int of_rccl_gather_flows(of_ctx *c, int nslots, float *out_uv_rank0) {
  return of_rccl_gather_slots(c, 0, nslots, out_uv_rank0);
}

// May run while a pair stream is open on this context, whose lane 0 is the
// context itself (bench.py gathers step s's slots while step s + 1 computes):
// so no API_BEGIN / API_END here -- they reset the context's arena and drain
// its pending solves under the lane thread -- and the gather's copies and
// RCCL calls go to a stream of its own (the slots' flows are complete: a
// ticket is done only after its lane's stream reached the end of the pair).
int of_rccl_gather_slots(of_ctx *c, int first, int nslots, float *out_uv_rank0) {
  if (!c) return OF_EINVAL;
  try {
  HIPCHK(hipSetDevice(c->device));
  REQUIRE(c->comm, OF_EINVAL, "of_rccl_init first");
  if (!c->gstream) ensure_lanes(c, 0);  // (never while a pool is open: of_pairs_open made it)
  REQUIRE(first >= 0 && nslots >= 1 && first + nslots <= (int)c->slots.size(), OF_EINVAL, "bad slot range");
  Slot *sl = c->slots.data() + first;
  const int H = sl[0].H, W = sl[0].W;
  for (int s = 0; s < nslots; ++s)
    REQUIRE(sl[s].uv && sl[s].H == H && sl[s].W == W, OF_EINVAL, "slots must share one size");
  const size_t per = 2 * (size_t)H * W;
  float *recv = nullptr;
  if (c->rank == 0) {  // one grow-only receive buffer per context (the call ends in a sync)
    const size_t need = sizeof(float) * per * nslots * c->nranks;
    if (need > c->gather_cap) {
      if (c->d_gather) HIPCHK(hipFree(c->d_gather));
      c->d_gather = nullptr;
      c->gather_cap = 0;
      HIPCHK(hipMalloc(&c->d_gather, need));
      c->gather_cap = need;
    }
    recv = c->d_gather;
  }
  // rank 0's own slots first: nothing that can throw runs between
  // ncclGroupStart and ncclGroupEnd, so a failed copy cannot leave a group open
  if (c->rank == 0)
    for (int s = 0; s < nslots; ++s)
      HIPCHK(hipMemcpyAsync(recv + per * s, sl[s].uv, sizeof(float) * per, hipMemcpyDeviceToDevice, c->gstream));
  ncclResult_t r = ncclGroupStart();
  for (int s = 0; s < nslots && r == ncclSuccess; ++s) {
    if (c->rank == 0) {
      for (int src = 1; src < c->nranks && r == ncclSuccess; ++src)
        r = ncclRecv(recv + per * ((size_t)src * nslots + s), per, ncclFloat, src, c->comm, c->gstream);
    } else {
      r = ncclSend(sl[s].uv, per, ncclFloat, 0, c->comm, c->gstream);
    }
  }
  ncclResult_t r2 = ncclGroupEnd();
  REQUIRE(r == ncclSuccess && r2 == ncclSuccess, OF_ERCCL,
          std::string("rccl gather: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
  if (c->rank == 0 && out_uv_rank0)
    HIPCHK(hipMemcpyAsync(out_uv_rank0, recv, sizeof(float) * per * nslots * c->nranks, hipMemcpyDeviceToHost,
                          c->gstream));
  HIPCHK(hipStreamSynchronize(c->gstream));
  return OF_OK;
  }
  API_CATCH(c)
}

int of_rccl_finalize(of_ctx *c) {
  if (!c) return OF_EINVAL;
  if (c->comm) ncclCommDestroy(c->comm);
  c->comm = nullptr;
  return OF_OK;
}

}  // extern "C"
