// host_noise.hip — host side of the noise-level estimation (kernels_noise.hip):
// the two estimators on device-resident frames (keys, the three-pass radix
// selection, one read-back) and their stage entries on host buffers.  The
// denoiser session's automatic sigma (host_fuse.hip) runs the device forms.
namespace {

unsigned noise_grid(size_t n) { return (unsigned)std::min<size_t>((n + NOISE_BLOCK - 1) / NOISE_BLOCK, 1024); }

// the context's selection words, zeroed: sizeof(NoiseSel) device bytes kept
// with the context (the arena holds the keys only)
NoiseSel *noise_sel(of_ctx *c) {
  if (!c->d_noise) HIPCHK(hipMalloc(&c->d_noise, sizeof(NoiseSel)));
  HIPCHK(hipMemsetAsync(c->d_noise, 0, sizeof(NoiseSel), c->stream));
  return c->d_noise;
}

// The lower median of each channel's N key slots, selected on the device
// after the key kernel has counted the first pass, and the estimate from it:
// five launches, no host synchronisation between them, then one read-back of
// n and the C keys (a stream synchronisation).
void noise_select(of_ctx *c, const uint32_t *keys, size_t N, int C, NoiseSel *sel, of_noise_estimate *out) {
  auto count = [&](int shift, int bits) {
    launch(c, "noise_count", k_noise_count, dim3(noise_grid(N), C), dim3(NOISE_BLOCK), 0, keys, (unsigned)N, shift, bits,
           sel);
  };
  launch(c, "noise_pick", k_noise_pick<11>, dim3(1), dim3(NOISE_BLOCK), 0, sel, C, 1);  // bits 31..21
  count(10, 11);
  launch(c, "noise_pick", k_noise_pick<11>, dim3(1), dim3(NOISE_BLOCK), 0, sel, C, 0);  // bits 20..10
  count(0, 10);
  launch(c, "noise_pick", k_noise_pick<10>, dim3(1), dim3(NOISE_BLOCK), 0, sel, C, 0);  // bits 9..0
  uint32_t h[1 + NOISE_MAX_C];  // n, then the prefixes: after the last pass the whole keys
  HIPCHK(hipMemcpyAsync(h, sel, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const double nan = std::nan("");
  out->n = (int64_t)h[0];
  double s = 0.0;
  for (int ch = 0; ch < NOISE_MAX_C; ++ch) {
    out->sigma_c[ch] = nan;
    if (ch >= C || h[0] == 0) continue;
    float m;
    memcpy(&m, &h[1 + ch], sizeof(m));
    out->sigma_c[ch] = std::sqrt((double)m) / 0.6744897501960817;
    s = s + out->sigma_c[ch] * out->sigma_c[ch];
  }
  out->sigma = h[0] == 0 ? nan : std::sqrt(s / (double)C);
}

// the pair estimator on device-resident frames (dense H x W x C), the flow
// im1 -> im2 of pitch P and its state (dense H x W, or nullptr: all 0)
void noise_pair_dev(of_ctx *c, const float *im1, const float *im2, int H, int W, int C, const float2 *flow, int P,
                    const uint8_t *state, of_noise_estimate *out) {
  const size_t px = (size_t)H * W;
  uint32_t *keys = new_dense<uint32_t>(c, px * C);
  NoiseSel *sel = noise_sel(c);
  c->cur_px = (double)px;
  launch(c, "noise_keys_pair", k_noise_keys_pair, dim3(noise_grid(px)), dim3(NOISE_BLOCK), 0, im1, im2, flow, state, H,
         W, P, C, keys, sel);
  noise_select(c, keys, px, C, sel, out);
}

// the single-frame estimator on a device-resident frame; H, W >= 2
void noise_single_dev(of_ctx *c, const float *im, int H, int W, int C, of_noise_estimate *out) {
  const size_t nb = (size_t)(H / 2) * (W / 2);
  uint32_t *keys = new_dense<uint32_t>(c, nb * C);
  NoiseSel *sel = noise_sel(c);
  c->cur_px = (double)H * W;
  launch(c, "noise_keys_single", k_noise_keys_single, dim3(noise_grid(nb)), dim3(NOISE_BLOCK), 0, im, H, W, C, keys,
         sel);
  noise_select(c, keys, nb, C, sel, out);
}

}  // namespace

extern "C" {

int of_estimate_noise_pair(of_ctx *c, const float *im1, const float *im2, int H, int W, int C, const float *fw,
                           const uint8_t *state, of_noise_estimate *out) {
  API_BEGIN(c)
  REQUIRE(im1 && im2 && fw && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= NOISE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_frame(H, W, "noise estimation");
  const size_t px = (size_t)H * W;
  float *d1, *d2;
  upload_frames(c, im1, im2, px * C, &d1, &d2);
  const F2 f = upload_f2(c, fw, H, W);
  noise_pair_dev(c, d1, d2, H, W, C, f.p, f.P, upload_dense(c, state, px), out);
  API_END(c)
}

int of_estimate_noise(of_ctx *c, const float *im, int H, int W, int C, of_noise_estimate *out) {
  API_BEGIN(c)
  REQUIRE(im && out, OF_EINVAL, "bad arguments");
  REQUIRE(C >= 1 && C <= NOISE_MAX_C, OF_EINVAL, "frames must have 1..4 channels");
  check_frame(H, W, "noise estimation");
  REQUIRE(H >= 2 && W >= 2, OF_EINVAL, "the single-frame noise estimate takes H and W >= 2");
  noise_single_dev(c, upload_dense(c, im, (size_t)H * W * C), H, W, C, out);
  API_END(c)
}

}  // extern "C"
