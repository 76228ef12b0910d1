// host_layers.hip — host side of the layered motion segmentation
// (kernels_layers.hip): option checks, the segmentation as two chains of
// launches on a device-resident flow, and the stage entry on host buffers.
// The passes are host_motion.hip's (motion_pass), with the removed set or a
// layer's label mask as the state plane.
namespace {

void check_layers_opts(const of_layers_opts *o) {
  REQUIRE(o, OF_EINVAL, "no layer options");
  REQUIRE(o->model >= OF_MOTION_TRANSLATION && o->model <= OF_MOTION_AFFINE, OF_EINVAL,
          "motion model must be 0 (translation), 1 (similarity) or 2 (affine)");
  REQUIRE(o->max_layers >= 1 && o->max_layers <= LAY_MAXK, OF_EINVAL, "max_layers must be 1..8");
  REQUIRE(o->grid >= 1 && o->grid <= 16, OF_EINVAL, "grid must be 1..16");
  REQUIRE(o->passes >= 0 && o->passes <= 16, OF_EINVAL, "passes must be 0..16");
  REQUIRE(o->rounds >= 0 && o->rounds <= 16, OF_EINVAL, "rounds must be 0..16");
  REQUIRE(o->smooth >= 0 && o->smooth <= LAY_MAXR, OF_EINVAL, "smooth must be 0..3");
  REQUIRE(std::isfinite(o->cutoff) && o->cutoff > 0, OF_EINVAL, "cutoff must be finite and > 0");
  REQUIRE(std::isfinite(o->min_support) && o->min_support > 0 && o->min_support <= 1, OF_EINVAL,
          "min_support must be in (0, 1]");
}

// The segmentation of the device-resident flow f; dw (dense H x W weights) and
// ds (dense H x W states) may be nullptr, d_raw (dense H x W) too.  The
// hypotheses and all o.max_layers extractions are queued as one chain: the
// device picks every seed and decides every stop, and what is queued behind a
// stop does nothing.  One read-back of the layer count sizes the second chain
// (the joint rounds, the closing passes, the mode filter); a second read-back
// fetches the layers.  Two stream synchronisations in here; the entry's
// download of the label planes ends in a third.
void segment_motion_dev(of_ctx *c, const F2 &f, const float *dw, const uint8_t *ds, const of_layers_opts &o,
                        of_motion_layer *layers, int32_t *n_layers, uint8_t *d_labels, uint8_t *d_raw) {
  const int H = f.H, W = f.W, K = o.max_layers, nh = o.grid * o.grid;
  const size_t px = (size_t)H * W;
  const MotionPasses p = motion_passes(c, H, W);
  const MotionFrame &fr = p.fr;
  const float2 *uv = (const float2 *)f.p;
  const dim3 tb(p.tile_blocks()), tt(MOT_WAVES * 64);
  const double c2 = o.cutoff * o.cutoff;
  LayerCtl *ctl = (LayerCtl *)c->arena.alloc(sizeof(LayerCtl));
  LayerHyp *hyp = (LayerHyp *)c->arena.alloc(sizeof(LayerHyp) * nh);
  MotionState *ms0 = (MotionState *)c->arena.alloc(sizeof(MotionState));
  MotionState *lay = (MotionState *)c->arena.alloc(sizeof(MotionState) * K);
  uint8_t *cst = new_dense<uint8_t>(c, px);
  if (!d_raw) d_raw = new_dense<uint8_t>(c, px);
  c->cur_px = (double)px;
  HIPCHK(hipMemsetAsync(ctl, 0, sizeof(LayerCtl), c->stream));
  launch(c, "layers_usable", k_layers_usable, tb, tt, 0, uv, H, W, f.P, dw, ds, p.ntx, p.nt, cst, ctl);
  // hypotheses: pass 0 of the fit per tile, then a solve per cell
  launch(c, "motion_init", k_motion_init, dim3(1), dim3(64), 0, ms0, c2);
  motion_part(c, p, f, dw, ds, ms0, MOT_PASS_FIRST, nullptr);
  launch(c, "layers_cells", k_layers_cells, dim3((unsigned)((nh + MOT_WAVES - 1) / MOT_WAVES)), tt, 0,
         (const double *)p.rec[0], p.stride[0], p.nty, p.ntx, o.grid, o.model, hyp);
  // extraction
  for (int l = 0; l < K; ++l) {
    launch(c, "layers_score", k_layers_score, tb, tt, 0, uv, H, W, f.P, (const uint8_t *)cst, (const LayerHyp *)hyp, nh,
           c2, fr, p.ntx, p.nt, ctl);
    launch(c, "layers_pick", k_layers_pick, dim3(1), dim3(64), 0, (const LayerHyp *)hyp, nh, l, o.min_support, c2,
           lay + l, ctl);
    for (int k = 0; k < o.passes; ++k)
      motion_pass(c, p, f, dw, cst, lay + l, MOT_PASS_ROBUST, o.model, 0.0, 1.0, c2, nullptr);
    launch(c, "layers_remove", k_layers_remove, tb, tt, 0, uv, H, W, f.P, cst, (const MotionState *)(lay + l), l, c2, fr,
           p.ntx, p.nt, ctl);
    launch(c, "layers_commit", k_layers_commit, dim3(1), dim3(64), 0, l, o.min_support, ctl);
  }
  LayerCtl h;
  HIPCHK(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int n = h.n;
  // joint rounds, the closing assignment and its passes, the mode filter
  uint8_t *mask = new_dense<uint8_t>(c, px * n, n > 0);
  for (int k = 0; k <= o.rounds; ++k) {
    launch(c, "layers_assign", k_layers_assign, tb, tt, 0, uv, H, W, f.P, (const uint8_t *)cst, lay, n, c2, fr, p.ntx,
           p.nt, d_raw, mask);
    for (int l = 0; l < n; ++l)
      motion_pass(c, p, f, dw, mask + px * l, lay + l, k < o.rounds ? MOT_PASS_ROBUST : MOT_PASS_LAST, o.model, 0.0, 1.0,
                  c2, nullptr);
  }
  const int nbx = (W + LAY_FW - 1) / LAY_FW, nby = (H + LAY_FH - 1) / LAY_FH;  // nbx * nby < 2^31 / 128
  launch(c, "layers_mode", k_layers_mode, dim3((unsigned)(nbx * nby)), dim3(LAY_FW * LAY_FH), 0, (const uint8_t *)d_raw,
         H, W, n, o.smooth, nbx, d_labels, ctl);
  std::vector<MotionState> hl(n);
  if (n > 0) HIPCHK(hipMemcpyAsync(hl.data(), lay, sizeof(MotionState) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n_layers = n;
  for (int l = 0; l < n; ++l) {
    of_motion_layer &out = layers[l];
    for (int k = 0; k < 6; ++k) out.theta[k] = hl[l].th[k];
    motion_matrix(hl[l].th, fr, out.matrix);
    out.support = hl[l].sums[0];
    out.rms = std::sqrt(hl[l].sums[12] / hl[l].sums[0]);
    out.pixels = h.pixels[l];
    out.degenerate = (hl[l].degenerate & 1) | h.lost[l];
    out.pad_ = 0;
  }
}

}  // namespace

extern "C" {

int of_segment_motion(of_ctx *c, const float *uv, int H, int W, const float *weight, const uint8_t *state,
                      const of_layers_opts *o, of_motion_layer *layers, int32_t *n_layers, uint8_t *labels,
                      uint8_t *labels_raw) {
  API_BEGIN(c)
  REQUIRE(uv && layers && n_layers && labels, OF_EINVAL, "bad arguments");
  check_frame(H, W, "motion segmentation");
  check_layers_opts(o);
  const size_t px = (size_t)H * W;
  if (weight)
    for (size_t k = 0; k < px; ++k)
      REQUIRE(std::isfinite(weight[k]) && weight[k] >= 0, OF_EINVAL, "weight must be finite and >= 0 everywhere");
  const F2 f = upload_f2(c, uv, H, W);
  float *dw = upload_dense(c, weight, px);
  uint8_t *ds = upload_dense(c, state, px);
  uint8_t *dlab = new_dense<uint8_t>(c, px);
  uint8_t *draw = new_dense<uint8_t>(c, px, labels_raw);
  segment_motion_dev(c, f, dw, ds, *o, layers, n_layers, dlab, draw);
  download_dense(c, labels, dlab, px);
  download_dense(c, labels_raw, draw, px);
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END(c)
}

}  // extern "C"
