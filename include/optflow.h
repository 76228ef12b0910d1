/*
 * optflow.h — C ABI of the MI355X-native variational optical-flow solver.
 *
 * One shared library (liboptflow.so, HIP for gfx950) runs the reference's
 * coarse-to-fine IRLS inner loop on the GPU.  The Python package
 * `optical_flow` (same API as jordanshivers/optical-flow-python) binds these
 * symbols with ctypes; any other host language binds the same symbols (see
 * INTEGRATION.md).  No torch / CUDA types appear here: plain pointers, sizes
 * and POD structs only.
 *
 * Conventions
 *   - Host buffers are caller-owned, C-contiguous float32.  "planar" means
 *     channel-major: plane c of an HxW image starts at c*H*W.  Flow fields
 *     (uv) are planar too: u plane then v plane.
 *   - Every function returns 0 on success and a negative OF_E* code on error;
 *     of_last_error() returns a message for the calling thread's context.
 *   - A context binds one HIP device and one stream; one context per host
 *     thread.  Calls are synchronous with respect to host buffers.
 *   - Non-convergence of an iterative solve is reported (of_stats), never an
 *     error — matching the reference, which ignores cg's `info`
 *     (optical_flow/methods/base.py:134-136).
 */
#ifndef OPTFLOW_H
#define OPTFLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OF_ABI_VERSION 3

/* status codes */
#define OF_OK 0
#define OF_EINVAL (-1)   /* bad argument (ValueError in the Python mirror) */
#define OF_EHIP (-2)     /* HIP runtime error */
#define OF_ENOMEM (-3)
#define OF_ENOTSUP (-4)  /* valid in the reference but not supported here */
#define OF_ERCCL (-5)

/* method kinds: optical_flow/methods/{hs,ba,classic_nl,alt_ba}.py */
enum of_method { OF_METHOD_HS = 0, OF_METHOD_BA = 1, OF_METHOD_CLASSIC_NL = 2, OF_METHOD_ALT_BA = 3 };

/* interpolation_method (optical_flow/utils/derivatives.py:148-294) */
enum of_interp { OF_INTERP_CUBIC = 0 /* 'cubic' = cubic B-spline */,
                 OF_INTERP_BICUBIC = 1 /* 'bi-cubic' = Hermite */,
                 OF_INTERP_BILINEAR = 2 /* 'bi-linear' */ };

/* solver (optical_flow/methods/base.py:87-114) */
enum of_solver { OF_SOLVER_BACKSLASH = 0, OF_SOLVER_PCG = 1, OF_SOLVER_SOR = 2 };

/* robust penalties (optical_flow/robust/penalties.py); OF_PEN_CONST is an
 * internal kind: rho'(x)/x == p0 everywhere (Horn-Schunck's 1/sigma^2). */
enum of_penalty_kind {
  OF_PEN_QUADRATIC = 0, OF_PEN_LORENTZIAN = 1, OF_PEN_CHARBONNIER = 2,
  OF_PEN_GEN_CHARBONNIER = 3, OF_PEN_GEMAN_MCCLURE = 4, OF_PEN_HUBER = 5,
  OF_PEN_TUKEY = 6, OF_PEN_GAUSSIAN = 7, OF_PEN_TDIST = 8, OF_PEN_TDIST_UNNORM = 9,
  OF_PEN_CONST = 100
};

typedef struct of_penalty {
  int32_t kind;
  int32_t pad_;
  double p0;   /* sigma, or r for t-dist */
  double p1;   /* a for generalized charbonnier, s for t-dist */
} of_penalty;

/*
 * A general spatial_filters list (classic_nl.py:301-322, ba.py:228-246,
 * alt_ba.py:298-316): filter i is fh[i] x fw[i] taps (row-major, at most
 * 5 x 5), applied as the reference's make_convn_mat(F, sz, 'valid',
 * 'sameswap') (utils/sparse_ops.py:59-109) with its own penalties.  general
 * = 0 means the default pair [[1, -1]], [[1], [-1]] with rho_spatial_* /
 * qua_spatial_* of of_params (the matrix-free 5-point hot path).
 */
#define OF_MAX_FILTERS 8
#define OF_MAX_FDIM 5
typedef struct of_filter_set {
  int32_t general;
  int32_t n;
  int32_t fh[OF_MAX_FILTERS], fw[OF_MAX_FILTERS];
  double taps[OF_MAX_FILTERS][OF_MAX_FDIM * OF_MAX_FDIM];
  of_penalty rho_u[OF_MAX_FILTERS], rho_v[OF_MAX_FILTERS];
  of_penalty qua_u[OF_MAX_FILTERS], qua_v[OF_MAX_FILTERS];
} of_filter_set;

/*
 * POD mirror of the method object's attribute bag
 * (optical_flow/methods/base.py:21-63, hs.py:23-47, ba.py:26-55,
 *  classic_nl.py:32-87, alt_ba.py:31-79).  The Python mirror fills it.
 */
typedef struct of_params {
  int32_t method;            /* enum of_method */
  int32_t solver;            /* enum of_solver */
  int32_t interp;            /* enum of_interp */
  int32_t texture;           /* ROF structure-texture pre-pass */
  int32_t fc;                /* high-pass pre-filter */
  int32_t auto_level;        /* BA/NL: pyramid_levels from image size */
  int32_t pyramid_levels;
  int32_t gnc_iters;
  int32_t gnc_pyramid_levels;
  int32_t max_iters;         /* IRLS warping iterations (BA, NL, AltBA) */
  int32_t max_warping_iters; /* HS */
  int32_t max_linear;
  int32_t pcg_maxiter;
  int32_t sor_max_iters;
  int32_t limit_update;
  int32_t median_filter_size;   /* 0 = None, else odd square size (5) */
  int32_t mf_iter;              /* HS */
  int32_t use_wmf;              /* Classic+NL non-local weighted median */
  int32_t area_hsz;
  int32_t itersLO;              /* AltBA */
  int32_t exact_maxiter;        /* 'backslash' surrogate: max PCG iterations */
  int32_t display;
  int32_t guide_mode;           /* estimate_flow builds a colour guide (color_images is not None) */
  int32_t pad_;
  double lambda_;
  double lambda_q;
  double alpha;                 /* initial GNC alpha */
  double pyramid_spacing;
  double gnc_pyramid_spacing;
  double pcg_rtol;
  double exact_rtol;            /* 'backslash' surrogate tolerance */
  double sor_omega;
  double sor_tol;
  double blend;
  double alp;
  double sigma_i;
  double sigmaD2, sigmaS2;      /* HS */
  double lambda2, lambda3;      /* AltBA */
  double deriv_filter[5];
  of_penalty rho_data, rho_spatial_u[2], rho_spatial_v[2];
  of_penalty qua_data, qua_spatial_u[2], qua_spatial_v[2];  /* quadratic relaxation */
  of_penalty rho_couple;        /* AltBA */
  of_filter_set filters;        /* ABI 3: general spatial_filters */
} of_params;

/* per-call statistics (may be NULL) */
#define OF_MAX_LEVELS 32
typedef struct of_stats {
  int32_t n_levels;                  /* levels processed (all GNC stages) */
  int32_t level_h[OF_MAX_LEVELS];
  int32_t level_w[OF_MAX_LEVELS];
  int32_t level_stage[OF_MAX_LEVELS];
  double level_ms[OF_MAX_LEVELS];    /* wall time of one compute_flow_base */
  int32_t solves;
  int32_t solver_iters_total;
  int32_t solver_iters_max;
  int32_t solves_not_converged;
  double total_ms;
  double preprocess_ms;
} of_stats;

typedef struct of_ctx of_ctx;

/* ---- context ---- */
int of_abi_version(void);
int of_device_count(int *count);
int of_ctx_create(int device, of_ctx **out);
int of_ctx_destroy(of_ctx *ctx);
const char *of_last_error(of_ctx *ctx);
int of_synchronize(of_ctx *ctx);
/* per-kernel HIP-event timing on the ctx stream: 0 = off, 1 = keyed by kernel
 * name, 2 = keyed by "name@pixels" (one entry per kernel and level size);
 * 3 = as 2, and every launch's start / end is also kept on a common time
 * axis across the batch lanes (of_kernel_timeline); see of_kernel_times */
int of_set_profiling(of_ctx *ctx, int enable);
/* solver options of a context (inherited by its batch lanes):
 *   OF_OPT_SOR_PIPELINE  2 (default): 'sor' runs its sweeps pipelined in one
 *                        persistent launch (k_sor_pipe), and a level of <= 64
 *                        rows whose LDS ring holds >= 8 sweeps in one
 *                        workgroup (k_sor_wg); 1: k_sor_pipe only; 0: one
 *                        launch per sweep
 *                        (k_sor_lex).  All give the same iterate and sweep
 *                        count bitwise. */
#define OF_OPT_SOR_PIPELINE 1
/*   OF_OPT_FUSED_WARP    1 (default): each warping iteration's partial_deriv
 *                        and flow_operator run as one kernel (no It / Ix /
 *                        Iy planes; 1 or 3 channels, one linearisation per
 *                        warp); 0: two kernels.  The same system bitwise
 *                        (no fma contraction in either form's warp, weight
 *                        and assembly arithmetic; tests/test_gpu_stages.py). */
#define OF_OPT_FUSED_WARP 3
int of_set_option(of_ctx *ctx, int option, int value);
/* read an option, or a read-only counter of the context and its batch lanes:
 *   OF_OPT_SOR_FALLBACKS  pipelined SOR solves whose sweep hand-off timed out
 *                         and were redone by the per-sweep kernel (the same
 *                         result; a sign of an oversubscribed GPU) */
#define OF_OPT_SOR_FALLBACKS 2
/*   OF_OPT_DEVICE_BYTES   device bytes the context and its batch lanes hold in
 *                         grow-only buffers (arena, SOR sweep ring, gather
 *                         buffer): flat across repeated pairs of one size; plus
 *                         an open point tracker's (of_tracks_open) and an open
 *                         temporal denoiser's (of_denoise_open), an open
 *                         stabiliser's (of_stab_open), an open
 *                         super-resolver's (of_sr_open), an open
 *                         inpainter's (of_inpaint_open) and an open mask
 *                         propagator's (of_masks_open) buffers, which leave
 *                         the count again at their close */
#define OF_OPT_DEVICE_BYTES 4
/*   OF_OPT_RCCL_NRANKS    ranks of the context's RCCL communicator as RCCL
 *                         reports them (ncclCommCount; 0 before of_rccl_init) */
#define OF_OPT_RCCL_NRANKS 5
int of_get_option(of_ctx *ctx, int option, int64_t *value);
/* progress of compute_flow / compute_flow_base: the reference's `display`
 * prints and its per-GNC-stage report (classic_nl.py:141-196, 255-256;
 * ba.py:101-133, 189-190; hs.py:80-81, 123-124; alt_ba.py:128-183, 249-250).
 * The callback runs on the calling thread, synchronously, between kernel
 * launches.  Events: a GNC stage starts; a pyramid level starts; a warping /
 * linear iteration's solve is done (with OF_PROGRESS_ITER: `norm` = the
 * reference's ||x - duv|| after the clip, or HS's ||x||, in fp64 on the
 * device -- one stream synchronisation per iteration); a GNC stage ends
 * (`elapsed_s` after a stream synchronisation; with OF_PROGRESS_FLOW `uv`
 * holds the stage's flow, planar 2 x h x w, valid during the call).  Batch
 * entries (of_pairs_*) never report.  fn = NULL turns it off. */
enum of_event { OF_EV_STAGE = 0, OF_EV_LEVEL = 1, OF_EV_ITER = 2, OF_EV_STAGE_END = 3 };
#define OF_PROGRESS_ITER 1
#define OF_PROGRESS_FLOW 2
typedef struct of_progress {
  int32_t event;           /* enum of_event */
  int32_t stage;           /* GNC stage, 0-based */
  int32_t level;           /* pyramid level index l (0 = finest; -1 for compute_flow_base) */
  int32_t h, w;            /* level size */
  int32_t iter, lin;       /* warping iteration i, linear iteration j (0-based) */
  int32_t pad_;
  double norm;             /* OF_EV_ITER */
  double elapsed_s;        /* OF_EV_STAGE_END: seconds since compute_flow started */
  const float *uv;         /* OF_EV_STAGE_END with OF_PROGRESS_FLOW, else NULL */
} of_progress;
typedef void (*of_progress_fn)(void *user, const of_progress *ev);
int of_set_progress(of_ctx *ctx, of_progress_fn fn, void *user, int flags);
/* kernel timing accumulated since enable: per kernel name total ms, launch
 * count and pixels processed (sum over launches of the level's H*W; ROF
 * counts H*W*channels); any output pointer may be NULL */
int of_kernel_times(of_ctx *ctx, int max, const char **names, double *ms, int64_t *count, double *pixels, int *n);
/* profiling mode 3: launches since enable, each with its kernel name, level
 * pixels and [start, end] in ms after the enable call (HIP events; lanes of a
 * batch share the time axis); *n = number of launches recorded */
int of_kernel_timeline(of_ctx *ctx, int max, const char **names, double *pixels, double *t0_ms, double *t1_ms,
                       int *n);

/*
 * Whole pair: estimate_flow (optical_flow/interface.py:11-71) without its
 * Python-side parameter handling.
 *   im1, im2 : H x W x C interleaved float32, C == 1 (gray) or C == 3 (RGB;
 *              converted on device with _rgb2gray / _rgb2lab semantics)
 *   init_uv  : planar 2 x H x W or NULL (zeros)
 *   out_uv   : planar 2 x H x W
 * The final GNC alpha is written back to params->alpha (Classic+NL keeps it,
 * classic_nl.py:180-184; BA restores it, ba.py:136).
 */
int of_estimate_flow(of_ctx *ctx, of_params *params, const float *im1, const float *im2,
                     int H, int W, int C, const float *init_uv, float *out_uv, of_stats *stats);

/*
 * compute_flow() on an already preprocessed pair (the method object's
 * `images`, `color_images`):
 *   images : planar (2*nc) x H x W   (frame-1 channels then frame-2 channels)
 *   guide  : planar gc x H x W Lab/gray guide for the weighted median, or NULL
 */
int of_compute_flow(of_ctx *ctx, of_params *params, const float *images, int H, int W, int nc,
                    const float *guide, int gc, const float *init_uv, float *out_uv, of_stats *stats);

/*
 * Per-pixel data-term weights (validity and confidence masks).  A weight
 * plane w is H x W float32, dense, every value finite and >= 0 (not limited
 * to <= 1); anything else: OF_EINVAL, checked on the host before any launch.
 * Where w is 0 the data term is gone and the smoothness term inpaints the
 * flow from its surroundings.  At pixel (i, j) of a level the assembled
 * system (of_flow_operator's planes) uses
 *   psi_w = psi * w[i][j]
 * in place of psi, the pixel's data weight: one fp32 product applied to the
 * finished psi (after the channel mean and the GNC blend of the quadratic and
 * the robust penalty), never contracted into an fma, in
 *   a_uu = psi_w*<Ix Ix> + (edge weights)      b_u = -(smoothness) - psi_w*<It Ix>
 *   a_uv = psi_w*<Ix Iy>                       b_v = -(smoothness) - psi_w*<It Iy>
 *   a_vv = psi_w*<Iy Iy> + (edge weights)
 * The smoothness weights, the clip and update, the occlusion detection and
 * both median filters do not see w.  The coarse levels use the weight's own
 * pyramid: the one-plane image w goes through the Gaussian and the bilinear
 * resize the frames get, with the levels and spacing of the image pyramid it
 * accompanies and again with those of the GNC pyramid.  Both steps are convex
 * combinations, so every level stays >= 0.
 * A NULL weight is the unweighted entry, bitwise (the same kernels).  A weight
 * with params->filters.general or with AltBA (classic-c-a): OF_ENOTSUP.  The
 * batch and stream entries (of_pairs_*), of_estimate_flow_bidir and
 * of_estimate_interp take no weight.
 * Known limitation: the content of a masked region still enters the global
 * minimum and maximum of the structure-texture split / scale_image, and the
 * blurred coarse frames around it; the weight pyramid only down-weights the
 * coarse pixels it pollutes.  Fill masked pixels with plausible values (their
 * surroundings, the other frame) rather than with extremes.
 *
 * Each entry is its unweighted sibling with `weight` added.
 * of_compute_flow_base_weighted uses the weight as given, for that one level;
 * of_flow_operator_weighted (a stage entry for the parity tests) likewise.
 */
int of_estimate_flow_weighted(of_ctx *ctx, of_params *params, const float *im1, const float *im2,
                              int H, int W, int C, const float *init_uv, const float *weight,
                              float *out_uv, of_stats *stats);
int of_compute_flow_weighted(of_ctx *ctx, of_params *params, const float *images, int H, int W, int nc,
                             const float *guide, int gc, const float *init_uv, const float *weight,
                             float *out_uv, of_stats *stats);
int of_compute_flow_base_weighted(of_ctx *ctx, of_params *params, const float *images, int H, int W, int nc,
                                  const float *guide, int gc, double alpha, const float *uv_in,
                                  const float *weight, float *out_uv);
int of_flow_operator_weighted(of_ctx *ctx, const of_params *params, double alpha, const float *uv,
                              const float *duv, const float *weight, const float *It, const float *Ix,
                              const float *Iy, int H, int W, int nc, float *coef, float *rhs);

/*
 * Forward-backward consistency of two flows (Sundaram et al. 2010): where can
 * `fw` (frame 1 -> 2) be trusted, given `bw` (frame 2 -> 1)?  fw, bw planar
 * 2 x H x W.  For pixel (i, j), 0-based, u = fw.x, v = fw.y, in double from
 * the fp32 flows, no fma contraction, in exactly this order (a numpy float64
 * restatement gives the same bits):
 *   q = j + u;  r = i + v
 *   inside = q >= 0 && q <= W-1 && r >= 0 && r <= H-1      (NaN / Inf: false)
 *   !inside: state = 2, err = +inf
 *   j0 = floor(q), i0 = floor(r); fc = q - j0; fr = r - i0
 *   j1 = min(j0+1, W-1); i1 = min(i0+1, H-1)
 *   bu = (1-fr)*((1-fc)*B[i0][j0].x + fc*B[i0][j1].x)
 *      + fr*((1-fc)*B[i1][j0].x + fc*B[i1][j1].x);   bv the same with .y
 *   du = u + bu; dv = v + bv;  err = du*du + dv*dv
 *   thr = alpha1*((u*u + v*v) + (bu*bu + bv*bv)) + alpha2
 *   state = err > thr ? 1 : 0
 *   state : H x W bytes: 0 consistent, 1 inconsistent / occluded, 2 the
 *           forward flow leaves the frame
 *   err   : H x W fp32 (float)err, or NULL
 * The usual thresholds are alpha1 = 0.01, alpha2 = 0.5.  The backward mask is
 * the same call with fw and bw exchanged.  alpha1 / alpha2 negative or not
 * finite: OF_EINVAL.
 */
int of_fb_consistency(of_ctx *ctx, const float *fw, const float *bw, int H, int W,
                      double alpha1, double alpha2, uint8_t *state, float *err);

/*
 * of_estimate_flow in both directions plus the forward-backward masks, one
 * call: out_fw equals of_estimate_flow(im1, im2), out_bw equals
 * of_estimate_flow(im2, im1) (bitwise), state_fw / state_bw (H x W bytes,
 * either may be NULL) equal of_fb_consistency(out_fw, out_bw) /
 * (out_bw, out_fw).  Gray conversion, the structure-texture split (or the
 * fc / plain scaling) and the image pyramids run once for both directions;
 * the weighted median's colour guide (Lab of each direction's first frame,
 * its /255 decision from that frame's own maximum) and its pyramids are
 * built per direction.  The two directions run one after the other on the
 * context's stream.  init_fw / init_bw: planar 2 x H x W or NULL (zeros).
 * params->alpha is written back once (both passes start from the caller's
 * value and end on the same one).  The progress callback reports the backward
 * pass as a second compute_flow.  stats_fw (may be NULL) is charged the shared
 * preprocessing and its total_ms is the whole call's wall time; stats_bw (may
 * be NULL) has preprocess_ms = 0 and the backward schedule's wall time.
 */
int of_estimate_flow_bidir(of_ctx *ctx, of_params *params, const float *im1, const float *im2,
                           int H, int W, int C, const float *init_fw, const float *init_bw,
                           float *out_fw, float *out_bw, double alpha1, double alpha2,
                           uint8_t *state_fw, uint8_t *state_bw, of_stats *stats_fw, of_stats *stats_bw);

/*
 * Using a flow on an image.  Common definitions, all in double from the fp32
 * inputs, no fma contraction, in exactly this order (a numpy float64
 * restatement gives the same bits); images are H x W x C interleaved:
 *   bil(A, r, q), r and q finite: the clamped bilinear sample of a plane
 *     qc = min(max(q, 0), W-1); j0 = floor(qc); fc = qc - j0; j1 = min(j0+1, W-1)
 *     rc, i0, fr, i1 the same with rows and H
 *     (1-fr)*((1-fc)*A[i0][j0] + fc*A[i0][j1]) + fr*((1-fc)*A[i1][j0] + fc*A[i1][j1])
 *   inside(r, q) = q >= 0 && q <= W-1 && r >= 0 && r <= H-1
 *   near(x, n)   = min(max(floor(x + 0.5), 0), n-1)
 *
 * of_warp_image: out(i, j, c) = (float)bil(im_c, i + v, j + u) with
 * (u, v) = uv(i, j) (planar 2 x H x W: u along columns, v along rows);
 * valid (H x W bytes or NULL) = inside(i + v, j + u).  A flow with a NaN or
 * Inf component gives valid 0 and out 0.  C is 1..4.
 */
int of_warp_image(of_ctx *ctx, const float *im, int H, int W, int C, const float *uv, float *out, uint8_t *valid);

/*
 * Occlusion-aware frame interpolation (Baker et al. 2011, sec. 3.3.2): the
 * frames at times t[0..n) strictly between im1 (time 0) and im2 (time 1) from
 * the flows F = fw (1 -> 2) and B = bw (2 -> 1), planar 2 x H x W.  Sf / Sb are
 * the states of of_fb_consistency(fw, bw) / (bw, fw) with alpha1, alpha2,
 * computed once per call.  Per t, with omt = 1.0 - t:
 *
 * 1. Splat.  Every source pixel (i, j), s = i*W + j, of frame f = 0
 *    ((u, v) = F[i][j], motion (a, b) = (u, v), tau = t) and of frame f = 1
 *    ((u, v) = B[i][j], (a, b) = (-u, -v), tau = omt) whose u and v are finite:
 *      q = j + tau*u; r = i + tau*v; jf = floor(q); i_f = floor(r)
 *      for di, dj in {0,1}^2: target (ti, tj) = (i_f + di, jf + dj), skipped
 *        when outside the frame (tested in double) or when its bilinear weight
 *        is zero (dj == 1 && q == jf, or di == 1 && r == i_f)
 *      cost = sum over c ascending of
 *             |bil(I1_c, ti - t*b, tj - t*a) - bil(I2_c, ti + omt*b, tj + omt*a)|
 *      K = (uint64)bits((float)cost) << 32 | f << 31 | s
 *    and the smallest K per target wins (a 64-bit atomic minimum: a
 *    non-negative float's bits order like its value, so the cheapest motion
 *    at the target wins, ties go to frame 1's flow, then to the lowest source
 *    index, whatever the order of arrival).  H*W >= 2^31: OF_ENOTSUP.
 * 2. Resolve.  A target nothing reached is a hole; otherwise its motion is
 *    ut = f ? -B[s] : F[s] (fp32, exact).
 * 3. Fill.  Jacobi passes: a hole with at least one non-hole among its 8
 *    neighbours as of the previous pass takes, per component, the double sum
 *    of those neighbours (row-major order) divided by their count, rounded to
 *    fp32, and is a non-hole from the next pass on; repeated until no hole is
 *    left.  A pass that fills nothing means no pixel has a motion: then
 *    ut = 0 everywhere and every pixel renders as the plain blend, info 3.
 * 4. Render pixel (i, j), (a, b) = ut:
 *      p1 = (i - t*b, j - t*a); p2 = (i + omt*b, j + omt*a)
 *      in1 = inside(p1); in2 = inside(p2)
 *      o1 = in1 && Sf[near(p1)] == 1   (frame 1's point is not visible in frame 2)
 *      o2 = in2 && Sb[near(p2)] == 1
 *      w1 = in1 && !o2;  w2 = in2 && !o1
 *      s1 = bil(I1_c, p1); s2 = bil(I2_c, p2)
 *      w1 && w2: omt*s1 + t*s2, info 0;  w1 only: s1, info 1;
 *      w2 only: s2, info 2;  neither: omt*s1 + t*s2, info 3
 *      out = (float) of that; info |= 4 where ut came from the hole filling
 *   out      : n x H x W x C
 *   out_ut   : n x 2 x H x W planar, the motion at time t, or NULL
 *   out_info : n x H x W bytes, or NULL
 * C is 1..4, n >= 1, every t[k] strictly inside (0, 1), alpha1 / alpha2 as
 * for of_fb_consistency; anything else: OF_EINVAL.
 * Known limitation: a surface that both frames see but that is hidden at time
 * t offers its motion at the same cost as the surface hiding it (the cost
 * compares the two frames only), so a thin occluder crossing in front of it
 * between the frames can lose its pixels at time t.
 */
int of_interp_frames(of_ctx *ctx, const float *im1, const float *im2, int H, int W, int C,
                     const float *fw, const float *bw, double alpha1, double alpha2,
                     int n, const double *t, float *out, float *out_ut, uint8_t *out_info);

/*
 * of_estimate_flow_bidir followed by of_interp_frames on the device-resident
 * frames, flows and states, one call: the flows never visit the host in
 * between, and out / out_info equal (bitwise) those of the two calls.  C is
 * 1 or 3 as for of_estimate_flow; out_fw / out_bw (planar 2 x H x W),
 * out_info and the stats (as for of_estimate_flow_bidir) may be NULL.
 */
int of_estimate_interp(of_ctx *ctx, of_params *params, const float *im1, const float *im2,
                       int H, int W, int C, double alpha1, double alpha2, int n, const double *t,
                       float *out, float *out_fw, float *out_bw, uint8_t *out_info,
                       of_stats *stats_fw, of_stats *stats_bw);

/*
 * Dense point trajectories across a frame sequence (Sundaram, Brox and
 * Keutzer, ECCV 2010).  A table of tracks: a point is carried from frame to
 * frame by the forward flow; its track ends where the forward-backward test
 * or a motion boundary says the flow cannot be trusted, or where it leaves
 * the frame; new tracks are seeded on a grid wherever the picture has
 * structure and no live track covers the cell.  A point is (x, y) = (column,
 * row) in fp32, pixel centres at integers, as for flows (u along columns); the
 * table stores it as n x 2 floats {x, y}.  Everything in double from the fp32
 * inputs, no fma contraction, in exactly the order written (a numpy float64
 * restatement gives the same bits); bil, inside and near as defined above
 * ("Using a flow on an image").  H * W >= 2^31: OF_ENOTSUP.
 *
 * Options.  Any value out of range or not finite: OF_EINVAL, checked on the
 * host before any launch (every entry checks the whole struct).
 */
#define OF_TRACK_ALIVE 0            /* still tracked */
#define OF_TRACK_OCCLUDED 1         /* the forward-backward test failed */
#define OF_TRACK_LEFT_FRAME 2       /* left the frame */
#define OF_TRACK_MOTION_BOUNDARY 3  /* ended at a motion boundary */
typedef struct of_track_opts {
  int32_t step;          /* seeding grid: one candidate per step x step cell, 1..64 */
  int32_t max_tracks;    /* capacity of the track table, 1..2^24 */
  double alpha1, alpha2; /* forward-backward test, as of_fb_consistency (0.01, 0.5); >= 0 */
  double beta1, beta2;   /* motion-boundary test (Sundaram et al.: 0.01, 0.002); >= 0 */
  double min_eig;        /* seeding: smallest eigenvalue threshold, >= 0; 0 accepts every free cell */
} of_track_opts;
/*
 * of_track_advance: one step of n tracks along F = fw (frame k -> k+1) with
 * B = bw (frame k+1 -> k), planar 2 x H x W.  A track whose status is not 0
 * comes back as it is.  For an alive track at (x, y):
 *   xd = x; yd = y
 *   !inside(yd, xd)                      -> status 2      (also NaN / Inf positions)
 *   u = bil(F.x, yd, xd); v = bil(F.y, yd, xd)
 *   x1 = xd + u; y1 = yd + v
 *   !inside(y1, x1)                      -> status 2      (a NaN flow sample lands here)
 *   bu = bil(B.x, y1, x1); bv = bil(B.y, y1, x1)
 *   du = u + bu; dv = v + bv; err = du*du + dv*dv
 *   thr = alpha1*((u*u + v*v) + (bu*bu + bv*bv)) + alpha2
 *   !(err <= thr)                        -> status 1
 *   i = near(yd, H); j = near(xd, W)
 *   jm = max(j-1, 0); jp = min(j+1, W-1); im = max(i-1, 0); ip = min(i+1, H-1)
 *   ux = F[i][jp].x - F[i][jm].x; uy = F[ip][j].x - F[im][j].x; vx, vy the same with .y
 *   g = 0.25*((ux*ux + uy*uy) + (vx*vx + vy*vy))
 *   !(g <= beta1*(u*u + v*v) + beta2)    -> status 3
 *   otherwise (x, y) <- ((float)x1, (float)y1), status 0
 * The tests run in that order, the first that fires decides; a track that ends
 * keeps its last position; the negated comparisons make NaN end a track.
 * (float)x1 <= W-1 follows from x1 <= W-1, so an alive track is always inside
 * the frame.  xy_in / xy_out: n x 2; status_in / status_out: n bytes; n >= 1.
 */
int of_track_advance(of_ctx *ctx, const float *fw, const float *bw, int H, int W, const of_track_opts *opts,
                     int n, const float *xy_in, const uint8_t *status_in, float *xy_out, uint8_t *status_out);
/*
 * of_track_seed: new tracks on the gray plane G (H x W fp32) for a table of n
 * tracks (n may be 0, then xy / status may be NULL; n <= max_tracks).  The
 * cells are ci < ceil(H/step), cj < ceil(W/step), in row-major order.
 *   - a cell's candidate pixel is (i, j) = (ci*step + step/2, cj*step + step/2)
 *     (integer division); a cell whose candidate is outside the frame has none
 *   - a cell is occupied when some alive track has
 *     (near(y, H) / step, near(x, W) / step) == (ci, cj)
 *   - a free cell's candidate is accepted when min_eig == 0, or when, summing
 *     over the 3 x 3 window (a, b) around (i, j) in row-major order, a and b
 *     clamped to the frame before use,
 *       gx = 0.5*(G[a][min(b+1, W-1)] - G[a][max(b-1, 0)]);  gy likewise along rows
 *       Jxx += gx*gx; Jxy += gx*gy; Jyy += gy*gy
 *     T = Jxx + Jyy; D = Jxx*Jyy - Jxy*Jxy satisfy
 *       T >= 2*min_eig && (D - min_eig*T) + min_eig*min_eig >= 0
 *     (lambda_min(J) >= min_eig without a square root)
 *   - accepted cells take the ids n, n+1, ... in row-major cell order while
 *     id < max_tracks (an exclusive prefix sum over the accept flags: the same
 *     ids whatever the launch geometry); the rest are dropped and counted
 *   - a new track is at ((float)j, (float)i), status 0, start = frame (>= 0)
 * *n_new = tracks added, *n_dropped = accepted cells the table had no room
 * for, xy_new = the n_new new points (room for min(max_tracks - n, cells)).
 */
int of_track_seed(of_ctx *ctx, const float *gray, int H, int W, const of_track_opts *opts, int frame,
                  int n, const float *xy, const uint8_t *status,
                  int32_t *n_new, int32_t *n_dropped, float *xy_new);
/*
 * The tracker session: one per context, its table and frames stay on the
 * device.  Ids are table indices and never move; dead tracks keep their slot.
 *   of_tracks_open   frames of H x W x C (C 1 or 3) with the given parameter
 *                    set; a second open on the context, or an open while a
 *                    pair stream is open: OF_EINVAL
 *   of_tracks_push   the next frame.  The first push only seeds (frame index
 *                    0; the out_* / state_* / stats buffers are untouched).
 *                    Every later push estimates both flows between the
 *                    previous frame and this one from a fresh copy of the
 *                    of_params given at open (out_fw, out_bw, state_fw,
 *                    state_bw, any of which may be NULL, are bitwise those of
 *                    of_estimate_flow_bidir on that pair with alpha1 / alpha2
 *                    of the options; the stats likewise; after
 *                    of_session_set_flow_scale they are bitwise those of
 *                    of_estimate_flow_bidir_scaled on that pair), advances the table
 *                    along them on the device, seeds on this frame's gray
 *                    plane with start = this frame's index, and keeps the
 *                    frame as the previous one.  The gray plane is the frame
 *                    itself for C = 1 and the _rgb2gray plane of
 *                    of_preprocess for C = 3.  *n_tracks = the table size
 *                    after the push; n_new / n_dropped as of_track_seed (all
 *                    three may be NULL).
 *   of_tracks_read   tracks first .. first+n-1 (xy n x 2, status, start: the
 *                    frame index a track was seeded in; any may be NULL)
 *   of_tracks_close  free the tracker (of_ctx_destroy does it too)
 * push, read and close without an open tracker: OF_EINVAL.  Other entries of
 * the context may be called between pushes.  The tracker's buffers are its
 * own allocations, not arena memory; their bytes are counted in
 * OF_OPT_DEVICE_BYTES from open to close.
 */
int of_tracks_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_track_opts *opts);
int of_tracks_push(of_ctx *ctx, const float *frame, float *out_fw, float *out_bw, uint8_t *state_fw,
                   uint8_t *state_bw, int32_t *n_tracks, int32_t *n_new, int32_t *n_dropped,
                   of_stats *stats_fw, of_stats *stats_bw);
int of_tracks_read(of_ctx *ctx, int first, int n, float *xy, uint8_t *status, int32_t *start);
int of_tracks_close(of_ctx *ctx);

/*
 * Motion-compensated temporal denoising of a frame sequence: a frame is
 * averaged with its neighbours in time, each warped onto it along a flow and
 * weighted per pixel by how well its warped patch matches the frame's.  Where
 * the forward-backward state, the frame border or the photometric difference
 * says a neighbour does not show the same surface, it is left out.
 * Everything in double from the fp32 inputs, no fma contraction, in exactly
 * the order written (a numpy float64 restatement gives the same bits); bil,
 * inside and near as defined above ("Using a flow on an image"); images
 * H x W x C interleaved, flows planar 2 x H x W, states H x W bytes in
 * of_fb_consistency's encoding.  H * W >= 2^31: OF_ENOTSUP.
 *
 * of_flow_compose: chain f (frame a -> b) and g (b -> c) into out (a -> c).
 * state_f / state_g may be NULL (all 0), out_state may be NULL.  For pixel
 * (i, j), (u, v) = f(i, j):
 *   u or v not finite, or !inside(i + v, j + u):
 *     out = f(i, j) unchanged, out_state = 2
 *   otherwise
 *     r = i + v; q = j + u
 *     gu = bil(g.x, r, q); gv = bil(g.y, r, q)
 *     out = ((float)(u + gu), (float)(v + gv))
 *     out_state = max(state_f[i][j], state_g[near(r, H)][near(q, W)])
 * so 2 (left the frame) dominates 1 (inconsistent) dominates 0; a NaN sampled
 * from g propagates into out.
 */
int of_flow_compose(of_ctx *ctx, const float *f, const float *g, int H, int W, const uint8_t *state_f,
                    const uint8_t *state_g, float *out, uint8_t *out_state);
/*
 * Options.  Any value out of range or not finite: OF_EINVAL, checked on the
 * host before any launch (every entry checks the whole struct).
 */
typedef struct of_fuse_opts {
  int32_t radius;   /* session only: neighbours on each side, 1..2 */
  int32_t patch;    /* half-size r of the comparison window, 0..3 (window (2r+1)^2) */
  double sigma;     /* noise standard deviation in image units, finite, > 0 */
  double strength;  /* rejection scale in units of sigma, finite, > 0 (4) */
  double alpha1, alpha2; /* session only: forward-backward test, as of_fb_consistency; >= 0 */
} of_fuse_opts;
/*
 * of_fuse_frames: the frame I = center fused with n neighbours N_k along
 * flows[k] (centre -> neighbour k), states[k] their forward-backward states
 * (NULL: all 0).  C is 1..4, n is 1..8.  With r = patch,
 *   two_s2 = 2.0*(sigma*sigma);  h2 = (strength*sigma)*(strength*sigma)
 * and for neighbour k, ascending, pixel (i, j), (u, v) = flows[k](i, j):
 *   vis_k(i,j) = u, v finite && inside(i + v, j + u) && state_k(i,j) == 0
 *   where vis_k:  Wk_c = bil(N_k,c, i + v, j + u)                   for each c
 *                 D_k(i,j) = sum over c ascending: dd = I_c(i,j) - Wk_c; += dd*dd
 *   window: S = 0, m = 0; for a = i-r..i+r, inside that b = j-r..j+r (row-major),
 *           positions outside the frame or with vis_k(a,b) == 0 skipped:
 *             S += D_k(a,b); m += 1
 *   !vis_k(i,j): w_k = 0
 *   otherwise:   d = S/(m*C); e = max(d - two_s2, 0); x = min(e/h2, 1)
 *                w_k = (1 - x)*(1 - x)
 * (a Tukey-type weight: exactly 1 while the patch difference is explained by
 * the noise, exactly 0 from e >= h2 on).  Per pixel
 *   acc_c = I_c(i,j); wsum = 1.0                    (the frame itself has weight 1)
 *   k ascending: acc_c += w_k*Wk_c; wsum += w_k
 *   out_c = (float)(acc_c/wsum); out_weight = (float)wsum
 * wsum is the effective number of frames averaged, 1..n+1.  The window sum
 * runs in that fixed order whatever the launch geometry.  The frames are taken
 * as finite.
 *   neigh      : n x H x W x C
 *   flows      : n x 2 x H x W
 *   states     : n x H x W bytes, or NULL
 *   out        : H x W x C
 *   out_weight : H x W, or NULL
 */
int of_fuse_frames(of_ctx *ctx, const float *center, int H, int W, int C, int n, const float *neigh,
                   const float *flows, const uint8_t *states, const of_fuse_opts *opts,
                   float *out, float *out_weight);
/*
 * of_fuse_weights: the neighbour weights of of_fuse_frames on their own, same
 * arguments, checks and order:  out_w[k](i,j) = (float)w_k, 0 where
 * !vis_k(i,j).
 *   out_w : n x H x W
 */
int of_fuse_weights(of_ctx *ctx, const float *center, int H, int W, int C, int n, const float *neigh,
                    const float *flows, const uint8_t *states, const of_fuse_opts *opts, float *out_w);
/*
 * The denoiser session: one per context; the last 2R+1 frames (R = radius)
 * and the last 2R adjacent pairs' flows and states stay on the device.
 *   of_denoise_open   frames of H x W x C (C 1 or 3) with the given parameter
 *                     set; a second open on the context, or an open while a
 *                     pair stream is open: OF_EINVAL
 *   of_denoise_push   frame k = 0, 1, ...  For k > 0 both flows between frame
 *                     k-1 and this one are estimated from a fresh copy of the
 *                     of_params given at open and zero initial flows; flows
 *                     and states are bitwise those of of_estimate_flow_bidir
 *                     on that pair with alpha1 / alpha2 of the options (of
 *                     of_estimate_flow_bidir_scaled after
 *                     of_session_set_flow_scale).  For
 *                     k >= R frame t = k - R is fused and written to out
 *                     (H x W x C) and out_weight (H x W or NULL), and
 *                     *out_index = t; otherwise *out_index = -1 and out is
 *                     untouched.
 *   of_denoise_flush  emits the next pending frame from the neighbours that
 *                     exist; *out_index = -1 when nothing is pending.  After
 *                     the first flush a push is refused (OF_EINVAL).
 *   of_denoise_close  free the session (of_ctx_destroy does it too)
 * push, flush and close without an open session: OF_EINVAL.  Frame t is fused
 * (of_fuse_frames) with the neighbours at offsets -1, +1, -2, +2, in that
 * order; offsets outside the clip so far, or beyond R, are skipped; with no
 * neighbour at all out is the frame itself and the weight 1.  With fw_j /
 * bw_j / sf_j / sb_j the flows j -> j+1, j+1 -> j and their states of pair
 * (j, j+1), the neighbours use
 *   +1: fw_t, sf_t                 -1: bw_{t-1}, sb_{t-1}
 *   +2: of_flow_compose(fw_t, fw_{t+1}; sf_t, sf_{t+1})
 *   -2: of_flow_compose(bw_{t-1}, bw_{t-2}; sb_{t-1}, sb_{t-2})
 * For C = 3 the fusion runs on the RGB frames as pushed.  Other entries of the
 * context may be called between pushes, and a point tracker may be open beside
 * the denoiser.  The session's buffers are its own allocations, not arena
 * memory; their bytes are counted in OF_OPT_DEVICE_BYTES from open to close.
 */
int of_denoise_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_fuse_opts *opts);
int of_denoise_push(of_ctx *ctx, const float *frame, float *out, float *out_weight, int32_t *out_index);
int of_denoise_flush(of_ctx *ctx, float *out, float *out_weight, int32_t *out_index);
int of_denoise_close(of_ctx *ctx);

/*
 * Noise-level estimation: the standard deviation sigma of additive Gaussian
 * noise, per channel and pooled, as the median absolute value of a residual
 * that holds noise of a known variance factor and little else.  The pair
 * estimator's residual is a pixel minus its motion-compensated partner in the
 * other frame (the median ignores the minority where the flow is wrong); the
 * single-frame estimator's is the diagonal Haar detail of 2 x 2 blocks.
 * Everything in double from the fp32 inputs, no fma contraction, in exactly
 * the order written; bil's taps and inside as defined above ("Using a flow on
 * an image"); images H x W x C interleaved, C 1..4, the flow planar 2 x H x W,
 * the state H x W bytes in of_fb_consistency's encoding.  H * W >= 2^31:
 * OF_ENOTSUP.
 *
 * of_estimate_noise_pair: fw is the flow im1 -> im2, state its forward-
 * backward state or NULL (all 0).  Pixel (i, j), (u, v) = fw(i, j), is usable
 * when u and v are finite, inside(i + v, j + u), state(i, j) == 0 and, with
 * the taps of bil at r = i + v, q = j + u (rows i0, i1, columns j0, j1,
 * fractions fr, fc), im1_c(i, j) and the four values im2_c(i0|i1, j0|j1) are
 * finite for every channel c.  Then
 *   w00 = (1 - fr)*(1 - fc); w01 = (1 - fr)*fc; w10 = fr*(1 - fc); w11 = fr*fc
 *   g = 1.0 + (((w00*w00 + w01*w01) + w10*w10) + w11*w11)
 *   e_c = im1_c(i, j) - bil(im2_c, r, q)
 *   key_c = (float)(e_c*e_c/g)
 * g is the variance factor of "own noise + interpolated noise" (2 at integer
 * flows, 1.25 at half-pixel ones), so the estimate does not depend on the
 * sub-pixel phase.  The bilinear sample interpolates the signal too: while
 * sigma is below the picture's interpolation error the estimate reads high.
 *
 * of_estimate_noise: the floor(H/2) x floor(W/2) non-overlapping 2 x 2 blocks
 * (an odd last row or column is left out); H or W below 2: OF_EINVAL.  Block
 * (bi, bj) with a = im_c(2bi, 2bj), b = im_c(2bi, 2bj+1), p = im_c(2bi+1, 2bj),
 * q = im_c(2bi+1, 2bj+1) is usable when all four are finite for every c; then
 *   d = ((a - b) - (p - q))/2.0;  key_c = (float)(d*d)
 *
 * Both: n = the usable pixels / blocks (every channel has n keys).  A key that
 * rounds to +Inf stays in as +Inf.  Per channel m_c = the lower median of the
 * n keys, the key of rank (n - 1)/2 (integer division, 0-based, ascending),
 * selected exactly (a radix selection over the keys' bit patterns with integer
 * counts: no dependence on launch geometry or arrival order), and on the host
 *   sigma_c = sqrt((double)m_c)/0.6744897501960817
 *   s = 0; c ascending: s += sigma_c*sigma_c;   sigma = sqrt(s/C)
 * sigma_c[C..3] are NaN.  n == 0: every sigma NaN, n = 0, OF_OK.  Device
 * scratch: the keys, 4*C*n_slots bytes of the arena (n_slots = H*W, or the
 * blocks), and 32 KB + 64 bytes of counters kept with the context.
 */
typedef struct of_noise_estimate {
  double sigma;       /* pooled over the channels */
  double sigma_c[4];  /* per channel */
  int64_t n;          /* samples per channel */
} of_noise_estimate;
int of_estimate_noise_pair(of_ctx *ctx, const float *im1, const float *im2, int H, int W, int C, const float *fw,
                           const uint8_t *state, of_noise_estimate *out);
int of_estimate_noise(of_ctx *ctx, const float *im, int H, int W, int C, of_noise_estimate *out);
/*
 * The denoiser session with an estimated sigma.  of_denoise_open_auto is
 * of_denoise_open except that opts->sigma is not read (the other options are
 * checked as there) and every emitted frame is fused with a sigma of its own;
 * `floor`, finite and > 0, in image units, is the smallest one used (clean
 * 8-bit material estimates 0, which the fusion refuses).  Every push that
 * completes a pair (k-1, k) runs of_estimate_noise_pair once on the two frames
 * as pushed, the pair's forward flow and its state, all still on the device,
 * and keeps the result E_{k-1} on the host.  For the emitted frame t
 *   s = 0; m = 0
 *   j = t-1, then t, where pair (j, j+1) exists among the frames pushed so
 *   far and 4*E_j.n >= H*W (a scene cut leaves few consistent pixels and must
 *   not set the level):  s += E_j.sigma*E_j.sigma; m += 1
 *   m > 0:                 sigma_t = sqrt(s/m)
 *   m == 0, H, W >= 2:     sigma_t = of_estimate_noise(frame t).sigma
 *   otherwise:             sigma_t = floor
 *   !(sigma_t >= floor):   sigma_t = floor          (a NaN estimate too)
 * and the fusion is of_fuse_frames with sigma = sigma_t, radius 2 included.
 * of_denoise_last_sigma: the sigma the last emitted frame was fused with (of a
 * session of either kind; opts->sigma for of_denoise_open); no session, or no
 * frame emitted yet: OF_EINVAL.
 */
int of_denoise_open_auto(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_fuse_opts *opts,
                         double floor);
int of_denoise_last_sigma(of_ctx *ctx, double *sigma);

/*
 * Global motion estimation and video stabilisation.  The dominant (camera)
 * motion of a flow field is fitted as a translation, a similarity or an
 * affine map by iteratively reweighted least squares with Tukey's biweight
 * and a decreasing cutoff (Odobez and Bouthemy 1995); a stabiliser smooths
 * the chain of those motions over a clip and warps every frame onto the
 * smoothed path.  Everything in double from the fp32 inputs, no fma
 * contraction, in exactly the order written (a numpy float64 restatement gives
 * the same bits); bil and inside as defined above ("Using a flow on an
 * image"); min(a, b) is a < b ? a : b and max(a, b) is b > a ? b : a, so a
 * NaN second operand gives the first.  H * W >= 2^31: OF_ENOTSUP.
 *
 * Coordinates and models.  s = 0.5*max(H, W), cx = 0.5*(W-1), cy = 0.5*(H-1);
 * pixel (i, j) has x = (j - cx)/s, y = (i - cy)/s, and the model flow is
 *   uh = th0 + th1*x + th2*y;  vh = th3 + th4*x + th5*y
 * with th1 = th2 = th4 = th5 = 0 (translation), th1 = th5 = a and
 * th4 = -th2 = b (similarity), or all six free (affine).
 *
 * Weight of pixel (i, j) in pass k.  w0 = weight[i][j] (NULL: 1.0), forced to
 * 0 where u or v is not finite or state[i][j] != 0 (NULL: all 0); there
 * u = v = 0 is used, so no NaN enters a sum.  With th of the previous pass
 * (zero for pass 0):
 *   ru = u - uh; rv = v - vh; r2 = ru*ru + rv*rv
 *   pass 0:      w = w0
 *   pass k >= 1: t = min(r2/c2, 1.0); w = w0*((1 - t)*(1 - t))
 * Sums of a pass, every product formed left to right as written:
 *   Sw = sum w;  Sx = sum w*x;  Sy = sum w*y
 *   Sxx = sum (w*x)*x;  Sxy = sum (w*x)*y;  Syy = sum (w*y)*y
 *   Su = sum w*u;  Sxu = sum (w*x)*u;  Syu = sum (w*y)*u;  Sv, Sxv, Syv with v
 *   Sr = sum w*r2
 * Order of every sum, whatever the launch geometry: tiles of 8 rows x 64
 * columns in row-major tile order, positions outside the frame contributing
 * +0.0; column l of a tile adds its 8 rows ascending into an accumulator
 * starting at +0.0; the 64 column values are combined by the halving tree
 *   for d = 32, 16, ..., 1: s[l] = s[l] + s[l+d] for l < d
 * the tile values, in tile order, are zero-padded to a multiple of 64 and each
 * group of 64 is reduced by the same tree, and so on until one value is left.
 *
 * Solve of a pass.  !(Sw > 0): th and c2 keep their values, no further pass
 * solves (the fit stops) and degenerate |= 2.  Otherwise
 *   translation: th0 = Su/Sw; th3 = Sv/Sw
 *   similarity:  q = Sxx + Syy; D = q - (Sx*Sx + Sy*Sy)/Sw
 *                a = ((Sxu + Syv) - (Sx*Su + Sy*Sv)/Sw)/D
 *                b = ((Sxv - Syu) - (Sx*Sv - Sy*Su)/Sw)/D
 *                th0 = (Su - a*Sx + b*Sy)/Sw; th3 = (Sv - b*Sx - a*Sy)/Sw
 *   affine:      m = Sx/Sw; n = Sy/Sw; A = Sxx - m*Sx; B = Sxy - m*Sy
 *                Cc = Syy - n*Sy; l = B/A; E = Cc - l*B
 *                per component f in {u, v}:
 *                  gx = Sxf - m*Sf; gy = Syf - n*Sf; p2 = (gy - l*gx)/E
 *                  p1 = (gx - B*p2)/A; p0 = (Sf - Sx*p1 - Sy*p2)/Sw
 *                (th0, th1, th2) = p of u; (th3, th4, th5) = p of v
 * Rank loss, !(D > 1e-9*Sw), or !(A > 1e-9*Sw) or !(E > 1e-9*Sw): that pass
 * solves the translation model instead and degenerate |= 1.
 * Cutoff, starting at c2 = c_min*c_min: after pass 0
 *   c2 = max(c_min*c_min, (kappa*kappa)*(Sr/Sw))
 * (th was zero: the weighted mean square of the flow itself), after each later
 * pass c2 = max(c_min*c_min, c2*decay).  Pass 0 and `iters` robust passes
 * solve; then one more pass weighs with the final th and c2 as a pass k >= 1,
 * writes the inlier plane (float)w and does not solve: its sums give
 * support = Sw and rms = sqrt(Sr/Sw).  passes = the solving passes run (the
 * one that stopped the fit included); cutoff = sqrt(c2).
 * The matrix (row-major 2 x 3) maps a point (column, row) of the flow's first
 * frame to the second:
 *   M = [1 + th1/s, th2/s, th0 - (th1*cx + th2*cy)/s;
 *        th4/s, 1 + th5/s, th3 - (th4*cx + th5*cy)/s]
 * Flows of +-1e30 are finite and enter the sums as they are.
 * Known limitation: the fit finds the dominant motion.  With the affine model
 * it breaks down when one coherent foreground region covers roughly 40 % or
 * more of the frame (it locks onto the wrong layer); the similarity model
 * held in the same scenes.
 */
#define OF_MOTION_TRANSLATION 0
#define OF_MOTION_SIMILARITY 1
#define OF_MOTION_AFFINE 2
/* Any value out of range or not finite: OF_EINVAL, checked on the host before
 * any launch. */
typedef struct of_motion_opts {
  int32_t model;   /* OF_MOTION_*, 0..2 */
  int32_t iters;   /* robust passes after pass 0, 0..64 (10) */
  double kappa;    /* first cutoff in units of the flow's rms, > 0 (2) */
  double decay;    /* factor on c2 per pass, 0 < decay <= 1 (0.5) */
  double c_min;    /* smallest cutoff in pixels, > 0 (0.5) */
} of_motion_opts;
typedef struct of_motion_fit {
  double theta[6];
  double matrix[6];
  double cutoff;    /* sqrt of the final c2, pixels */
  double support;   /* Sw of the last pass */
  double rms;       /* sqrt(Sr/Sw) of the last pass (NaN without support) */
  int32_t passes;
  int32_t degenerate;  /* 1 rank loss | 2 no support */
} of_motion_fit;
/*
 *   uv         : planar 2 x H x W
 *   weight     : H x W fp32, every value finite and >= 0 (else OF_EINVAL), or NULL
 *   state      : H x W bytes (of_fb_consistency's encoding; != 0 masks), or NULL
 *   out_inlier : H x W fp32, the last pass's w, or NULL
 */
int of_fit_motion(of_ctx *ctx, const float *uv, int H, int W, const float *weight, const uint8_t *state,
                  const of_motion_opts *opts, of_motion_fit *out, float *out_inlier);
/*
 * of_warp_affine: A (row-major 2 x 3) maps an output pixel to its source
 * position.  For output pixel (i, j):
 *   q = (A[0]*j + A[1]*i) + A[2];  r = (A[3]*j + A[4]*i) + A[5]
 *   q and r finite and inside(r, q): out(i, j, c) = (float)bil(im_c, r, q), valid 1
 *   otherwise: out 0, valid 0
 * im, out: H x W x C interleaved, C is 1..4; valid: H x W bytes or NULL.
 */
int of_warp_affine(of_ctx *ctx, const float *im, int H, int W, int C, const double A[6], float *out,
                   uint8_t *valid);
/*
 * The stabiliser session: one per context; the last radius + 1 frames stay on
 * the device, the motions (six doubles each) on the host.
 *   of_stab_open   frames of H x W x C (C 1 or 3) with the given parameter set;
 *                  a second open on the context, or an open while a pair
 *                  stream is open: OF_EINVAL
 *   of_stab_push   frame k = 0, 1, ...  For k > 0 both flows between frame k-1
 *                  and this one are estimated from a fresh copy of the
 *                  of_params given at open and zero initial flows (bitwise
 *                  of_estimate_flow_bidir with alpha1 / alpha2 of the options,
 *                  or of_estimate_flow_bidir_scaled after
 *                  of_session_set_flow_scale),
 *                  and M_{k-1} = the matrix of of_fit_motion on the
 *                  device-resident forward flow with the forward state as
 *                  `state`, no weight and `fit` of the options.  A motion
 *                  that cannot be inverted (below) is replaced by the identity.
 *                  out_motion (6 doubles or NULL) receives M_{k-1} as kept,
 *                  *degenerate the fit's flags | 4 for every replacement by
 *                  the identity in this call.  For k >= radius frame
 *                  t = k - radius is emitted: out (H x W x C), out_valid (H x W
 *                  bytes or NULL), out_transform (S_t, 6 doubles, or NULL) and
 *                  *out_index = t; otherwise *out_index = -1 and they are
 *                  untouched.
 *   of_stab_flush  emits the next pending frame from the neighbours that
 *                  exist; *out_index = -1 when nothing is pending.  After the
 *                  first flush a push is refused (OF_EINVAL).
 *   of_stab_close  free the session (of_ctx_destroy does it too)
 * push, flush and close without an open session: OF_EINVAL.  Other entries of
 * the context may be called between pushes, and a point tracker and a temporal
 * denoiser may be open beside the stabiliser.  The session's buffers are its
 * own allocations, not arena memory; their bytes are counted in
 * OF_OPT_DEVICE_BYTES from open to close.
 *
 * Path smoothing, on the host, in double, in the order written.
 *   inverse of [a b tx; c d ty]:
 *     det = a*d - b*c; ia = d/det; ib = -b/det; ic = -c/det; id = a/det
 *     itx = -(ia*tx + ib*ty); ity = -(ic*tx + id*ty)
 *     !(fabs(det) >= 1e-12) or an entry that is not finite: the matrix is
 *     replaced by the identity (and so is its inverse), degenerate |= 4
 *   composition X o Y (Y first), each entry left to right:
 *     [X0*Y0 + X1*Y3, X0*Y1 + X1*Y4, (X0*Y2 + X1*Y5) + X2;
 *      X3*Y0 + X4*Y3, X3*Y1 + X4*Y4, (X3*Y2 + X4*Y5) + X5]
 *   P(t->t) = I;  P(t->t+d) = M_{t+d-1} o P(t->t+d-1)
 *   P(t->t-d) = inv(M_{t-d}) o P(t->t-d+1)
 *   g_d = exp(-(d*d)/((2*sigma_t)*sigma_t))
 *   S_t = (sum g_d*P(t->t+d)) / (sum g_d), entrywise, both sums starting at 0
 *         and d running 0, -1, +1, -2, +2, ... over the offsets inside the
 *         clip so far and within the radius
 * The emitted frame is of_warp_affine(frame t, inv(S_t)): the frame as seen
 * from the smoothed camera path.
 */
typedef struct of_stab_opts {
  of_motion_opts fit;
  int32_t radius;        /* frames of the smoothing window on each side, 1..30 */
  int32_t pad_;
  double sigma_t;        /* standard deviation of the smoothing window in frames, finite, > 0 */
  double alpha1, alpha2; /* forward-backward test, as of_fb_consistency; >= 0 */
} of_stab_opts;
int of_stab_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_stab_opts *opts);
int of_stab_push(of_ctx *ctx, const float *frame, float *out, uint8_t *out_valid, double *out_transform,
                 double *out_motion, int32_t *degenerate, int32_t *out_index);
int of_stab_flush(of_ctx *ctx, float *out, uint8_t *out_valid, double *out_transform, int32_t *degenerate,
                  int32_t *out_index);
int of_stab_close(of_ctx *ctx);

/*
 * Reduced-resolution flow with edge-aware upsampling.  The flow is estimated
 * on frames reduced by an integer factor and brought back to full size by a
 * joint bilateral filter guided by the full-resolution frame, so that motion
 * boundaries land on the picture's edges instead of being smeared over s
 * pixels as a plain resize (of_resample_flow) would leave them.  Everything in
 * double from the fp32 inputs, no fma contraction, no transcendental, in
 * exactly the order written (a numpy float64 restatement gives the same bits).
 * s = scale, an integer 2..4; hs = ceil(H/s), ws = ceil(W/s).  Images are
 * H x W x C interleaved, C 1..4; flows planar.  H * W >= 2^31: OF_ENOTSUP.
 *
 * of_reduce_frame: the box reduction L (hs x ws x C) of im.
 *   L_c(a, b) = (float)(S/m)
 *   S = the sum of I_c(i, j) over rows i = a*s .. min(a*s + s, H) - 1 and,
 *       inside each row, columns j = b*s .. min(b*s + s, W) - 1, row-major,
 *       starting from +0.0;  m = the number of terms
 *
 * of_flow_upsample: the low flow f (planar 2 x hs x ws, in low-resolution
 * pixels) with its low guide L (hs x ws x C, the reduction of the frame the
 * flow starts in) onto the full guide G (H x W x C).  h2 = range*range.  For
 * output pixel (i, j):
 *   r = (i - 0.5*(s-1))/s;  q = (j - 0.5*(s-1))/s;  a0 = floor(r);  b0 = floor(q)
 *   U = V = Sw = 0;  Us = Vs = Ss = 0
 *   for a = a0-1 .. a0+2, inside that b = b0-1 .. b0+2 (row-major), skipped
 *   when a or b is outside the low frame or f(a,b).x or .y is not finite:
 *     wa = max(1 - |a - r|/2, 0);  wb = max(1 - |b - q|/2, 0);  wsp = wa*wb
 *     D = sum over c ascending: d = G_c(i,j) - L_c(a,b); += d*d
 *     z = D/(C*h2);  x = z < 1 ? z : 1;  wr = (1 - x)*(1 - x);  w = wsp*wr
 *     U += w*fx; V += w*fy; Sw += w;   Us += wsp*fx; Vs += wsp*fy; Ss += wsp
 *   Sw > 0:      out = ((float)(s*(U/Sw)),  (float)(s*(V/Sw))),  info 0
 *   else Ss > 0: out = ((float)(s*(Us/Ss)), (float)(s*(Vs/Ss))), info 1
 *   else:        out = (NaN, NaN),                               info 2
 * info 1: no neighbour looks like this pixel, the spatial weights alone
 * decide.  A G value that is not finite makes D not finite; x = z < 1 ? z : 1
 * then gives x = 1 and wr = 0, so such a pixel takes the spatial branch.  A
 * low flow of +-1e30 is finite and enters the sums as it is.
 *   f_lo     : planar 2 x hs x ws
 *   L        : hs x ws x C
 *   G        : H x W x C
 *   out_uv   : planar 2 x H x W, in full-resolution pixels
 *   out_info : H x W bytes, or NULL
 * Options: any value out of range or not finite: OF_EINVAL, checked on the
 * host before any launch.  The low size is not an argument: it is hs x ws of
 * (H, W, scale), and the buffers are taken to have it.
 */
typedef struct of_upsample_opts {
  int32_t scale;   /* s, 2..4 (of_session_set_flow_scale: 1 clears) */
  int32_t pad_;
  double range;    /* photometric cutoff in image units, finite, > 0 (20 for 0..255 frames) */
} of_upsample_opts;
int of_reduce_frame(of_ctx *ctx, const float *im, int H, int W, int C, int scale, float *out);
int of_flow_upsample(of_ctx *ctx, const float *f_lo, const float *L, const float *G, int H, int W, int C,
                     const of_upsample_opts *opts, float *out_uv, uint8_t *out_info);
/*
 * The one-call entries: both frames are reduced on the device, the existing
 * estimate runs unchanged on the reduced pair at hs x ws from zero initial
 * flows (with params->auto_level the pyramid depth follows from that size),
 * every low flow is upsampled with its own first frame as guide (frame 1 for
 * the forward flow, frame 2 for the backward one), and the states are the
 * forward-backward check of the full-resolution upsampled flows.  The result
 * is bitwise the composition of the stage entries through the host:
 *   L1 = of_reduce_frame(im1); L2 = of_reduce_frame(im2)
 *   f, b = of_estimate_flow_bidir(L1, L2 at hs x ws)      (of_estimate_flow for the one direction)
 *   out_fw = of_flow_upsample(f, L1, im1); out_bw = of_flow_upsample(b, L2, im2)
 *   state_fw = of_fb_consistency(out_fw, out_bw); state_bw = (out_bw, out_fw)
 * C is 1 or 3.  The stats are those of the reduced estimate, with the
 * reduction charged to preprocess_ms (of stats_fw) and total_ms of stats /
 * stats_fw the whole call's wall time.  No weight is accepted, as for
 * of_estimate_flow_bidir.  state_*, stats* may be NULL.
 */
int of_estimate_flow_scaled(of_ctx *ctx, of_params *params, const float *im1, const float *im2, int H, int W, int C,
                            const of_upsample_opts *opts, float *out_uv, of_stats *stats);
int of_estimate_flow_bidir_scaled(of_ctx *ctx, of_params *params, const float *im1, const float *im2, int H, int W,
                                  int C, const of_upsample_opts *opts, double alpha1, double alpha2, float *out_fw,
                                  float *out_bw, uint8_t *state_fw, uint8_t *state_bw, of_stats *stats_fw,
                                  of_stats *stats_bw);
/*
 * of_session_set_flow_scale: the open sessions named by `kinds` (one or more
 * of OF_SESSION_*) estimate their pairs as of_estimate_flow_bidir_scaled with
 * `opts` from now on; scale 1 (range is then not read) returns them to
 * of_estimate_flow_bidir.  Allowed between a session's open and its second
 * push, that is before its first pair; later, or with a named kind not open,
 * or kinds naming none: OF_EINVAL, and no session is changed.  What follows
 * the estimate in a push (advance, fuse, compose, noise, fit, warp) sees
 * full-resolution flows and states and is unchanged.  The reduced frames and
 * low flows are arena memory of the push: a session's own allocations, and so
 * OF_OPT_DEVICE_BYTES of an open session, do not change.
 */
#define OF_SESSION_TRACKS 1
#define OF_SESSION_DENOISE 2
#define OF_SESSION_STAB 4
int of_session_set_flow_scale(of_ctx *ctx, int kinds, const of_upsample_opts *opts);

/*
 * Multi-frame super-resolution along the flow.  The temporal denoiser puts
 * every warped neighbour back on the frame's own pixel grid; here the frame
 * and its neighbours are resampled onto a grid s times finer, every
 * neighbour's pixels placed where its flow says they belong, so the sub-pixel
 * phases the flows carry add detail instead of being averaged away.  It is the
 * inverse of the camera model of_reduce_frame states (box integration by an
 * integer factor).  Everything in double from the fp32 inputs, no fma
 * contraction, no transcendental, in exactly the order written (a numpy
 * float64 restatement gives the same bits); bil, inside and near as defined
 * above ("Using a flow on an image"); images H x W x C interleaved, flows
 * planar 2 x H x W in low-resolution pixels running centre -> neighbour k,
 * states as for of_fuse_frames.  C is 1..4, n is 0..8 (with n = 0 neigh, flows
 * and states may be NULL).  s = factor; the output is sH x sW x C.
 * s*s*H*W >= 2^31: OF_ENOTSUP.
 *
 * Weights:  Wk = of_fuse_weights(center, neigh, flows, states; sigma,
 * strength, patch), n x H x W fp32 planes.
 *
 * Resampling:  rho2 = reach*reach.  For output pixel (Y, X):
 *   r = (Y - 0.5*(s-1))/s;  q = (X - 0.5*(s-1))/s          (of_flow_upsample's mapping)
 *   ic = Y / s; jc = X / s                                  (integer division)
 *   acc_c = 0 for every c;  S = 0
 *   frames k = 0 (the centre: zr = r, zq = q, R = 1.0), then k = 1..n ascending:
 *     k >= 1:  R = Wk[k][ic][jc];  R == 0: skip the frame
 *              u = bil(F_k.x, r, q); v = bil(F_k.y, r, q);  zr = r + v; zq = q + u
 *              !inside(zr, zq): skip the frame              (a non-finite flow at any tap lands here)
 *     a0 = floor(zr + 0.5); b0 = floor(zq + 0.5)
 *     a = a0-1 .. a0+1, inside that b = b0-1 .. b0+1 (row-major), positions outside the frame skipped:
 *       dy = a - zr; dx = b - zq; x = (dy*dy + dx*dx)/rho2;  !(x < 1): skip the tap
 *       K = (1 - x)*(1 - x);  w = K*R
 *       acc_c = acc_c + w*N_k,c[a][b] for every c (ascending);  S = S + w
 *   out_c = (float)(acc_c/S);  out_support = (float)S
 * S > 0 always: the centre's nearest tap is closer than 0.5 per axis, so
 * x < 0.5/0.5625 there.  The 3 x 3 window is complete because reach <= 1.5.
 * The skips are part of the definition: a zero term must not touch the sign of
 * a zero sum.  out_support is the weight the output pixel rests on; above the
 * value of the n = 0 result it counts what the neighbours added.
 *
 * Back-projection, one step when back > 0:
 *   L = of_reduce_frame(out, s)                             (H x W x C again)
 *   e_c(i,j) = I_c(i,j) - L_c(i,j)
 *   out_c(Y,X) = (float)(out_c(Y,X) + back*e_c(Y/s, X/s))
 * With back = 1 the result reduces back to the centre frame, up to rounding;
 * the centre's noise comes back with it, so the default is 0.
 *
 * Two limits.  sigma must cover the aliasing between the frames as well as the
 * noise: on a strongly aliased scene of the numpy prototype sigma = 5 left a
 * mean neighbour weight of 0.005, and the output was the single-frame result.
 * reach = 0.75 is the best of {0.6, 0.75, 1.0, 1.5} in that prototype on one
 * texture; it is not a measured optimum.
 *   neigh       : n x H x W x C
 *   flows       : n x 2 x H x W
 *   states      : n x H x W bytes, or NULL
 *   out         : sH x sW x C
 *   out_support : sH x sW, or NULL
 * Options: any value out of range or not finite: OF_EINVAL, checked on the
 * host before any launch (every entry checks the whole struct).
 */
typedef struct of_sr_opts {
  int32_t factor;   /* s, 2..4 */
  int32_t radius;   /* session only: neighbours on each side, 1..2 */
  int32_t patch;    /* as of_fuse_opts, 0..3 */
  int32_t pad_;
  double sigma, strength;   /* as of_fuse_opts: the neighbour weight */
  double reach;     /* kernel radius in low-resolution pixels, 0.75..1.5 */
  double back;      /* back-projection step, 0..1 */
  double alpha1, alpha2;    /* session only: forward-backward test, as of_fb_consistency; >= 0 */
} of_sr_opts;
int of_super_resolve(of_ctx *ctx, const float *center, int H, int W, int C, int n, const float *neigh,
                     const float *flows, const uint8_t *states, const of_sr_opts *opts, float *out,
                     float *out_support);
/*
 * The super-resolver session: one per context, beside the other kinds; it
 * keeps what the denoiser session keeps (the last 2R+1 frames, the last 2R
 * adjacent pairs' flows and states) and of_sr_open / _push / _flush / _close
 * behave as of_denoise_open / _push / _flush / _close do, with the same
 * neighbours in the same order (-1, +1, -2, +2; two frames apart through
 * of_flow_compose).  Frame t is emitted as of_super_resolve of that frame with
 * those neighbours: out is sH x sW x C, out_support sH x sW or NULL; a clip of
 * one frame gives the n = 0 result.  The session's buffers count in
 * OF_OPT_DEVICE_BYTES from open to close.  It is not a kind
 * of_session_set_flow_scale takes: its pairs are estimated at full resolution.
 */
int of_sr_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_sr_opts *opts);
int of_sr_push(of_ctx *ctx, const float *frame, float *out, float *out_support, int32_t *out_index);
int of_sr_flush(of_ctx *ctx, float *out, float *out_support, int32_t *out_index);
int of_sr_close(of_ctx *ctx);

/*
 * Flow-guided video inpainting.  A region is marked in every frame of a clip
 * (an object to remove; of_masks_* below carries one drawn mask through the
 * clip); the region is filled with what the other frames
 * show there, carried along the motion (Huang et al. 2016; Xu et al. 2019,
 * without their networks).  Under the marks the flows are completed from their
 * surroundings by the solver itself (a data weight of 0, "Per-pixel data-term
 * weights" above); a marked pixel then walks through the completed flows of
 * the adjacent pairs until it lands on a pixel that some frame really saw.
 * Everything in double from the fp32 or byte inputs, no fma contraction, in
 * exactly the order written (a numpy float64 restatement gives the same bits);
 * bil and inside as defined above ("Using a flow on an image"); frames
 * H x W x C interleaved, flows planar 2 x H x W, masks H x W bytes, a nonzero
 * byte marking a pixel to be replaced.  H * W >= 2^31: OF_ENOTSUP.  Any option
 * out of range or not finite: OF_EINVAL, checked on the host before any launch
 * (every entry checks the whole struct).
 *
 * Grown mask:  D = grow(M, g):  D(i,j) = 1 where any M(i+a, j+b) != 0 with
 * |a|, |b| <= g inside the frame, else 0; g = 0 gives M != 0.
 *
 * Pair weight of frames j and j+1 with grown masks D_j, D_j+1:
 *   w(i,j) = 0.0f where grow(D_j | D_j+1, margin) is set, else 1.0f
 * so the data term of both flows of the pair is off under the holes of either
 * frame, margin pixels around them, and where the other frame's hole may land.
 * The frames themselves go into the estimate unchanged: the object's own
 * pixels are plausible content for the smoothness term to start from.
 *
 * Fill of frame t from the frames I_s, the grown masks D_s and the flows fw_s
 * (s -> s+1) and bw_s (s+1 -> s) of the adjacent pairs within `radius` of t.
 * A pixel (i, j) with D_t(i,j) == 0: out = the frame's own value, status
 * OF_INPAINT_KEPT, both hop counts 0.  A pixel with D_t(i,j) != 0 walks
 * forward (flows fw_t, fw_t+1, ..., targets t+1, t+2, ...) and backward (flows
 * bw_t-1, bw_t-2, ..., targets t-1, t-2, ...).  Each walk starts from r = i,
 * q = j without a hit; for hop d = 1 .. radius, while the target frame exists:
 *   u = bil(F.x, r, q); v = bil(F.y, r, q)        (F: the flow of this hop)
 *   u or v not finite                        -> the walk ends without a hit
 *   r = r + v; q = q + u
 *   !inside(r, q)                            -> the walk ends without a hit
 *   i0 = floor(r); j0 = floor(q); i1 = min(i0+1, H-1); j1 = min(j0+1, W-1)
 *   any of D_target at (i0,j0) (i0,j1) (i1,j0) (i1,j1) nonzero -> next hop
 *   otherwise: colour_c = bil(I_target_c, r, q); hops = d; hit; the walk ends
 * With a forward hit at df (colour cf) and a backward hit at db (colour cb):
 *   out_c = (float)(((double)db*cf_c + (double)df*cb_c) / (double)(df + db))
 * (the nearer frame counts more); with one hit (float) of its colour; with
 * none the frame's own value.  Status OF_INPAINT_FILLED or OF_INPAINT_UNFILLED;
 * out_hops holds df, then db (0 = no hit).  Flows of +-1e30 are finite: their
 * walk ends at !inside.  The walk consults no forward-backward state: until it
 * hits it moves only through grown holes, where that test says nothing, and the
 * hit itself uses no flow.
 *
 * Known limits: this fill has no spatial fallback (a pixel that no frame
 * within `radius` reveals comes back OF_INPAINT_UNFILLED) and no seam or
 * exposure blending: both are "Gradient-domain blending" below
 * (of_inpaint_blend, of_inpaint_set_blend).  A hole bordered by two motions
 * gets the smoothness term's blend of them; the marks must cover shadows and
 * reflections themselves, `grow` only pads them.
 */
#define OF_INPAINT_KEPT 0
#define OF_INPAINT_FILLED 1
#define OF_INPAINT_UNFILLED 2
#define OF_INPAINT_MAX_RADIUS 16
#define OF_INPAINT_MAX_GROW 8
#define OF_INPAINT_MAX_MARGIN 16
#define OF_MASK_GROW_MAX 24
typedef struct of_inpaint_opts {
  int32_t radius;   /* frames on each side a walk may reach, 1..16 (8) */
  int32_t grow;     /* g of the grown masks, 0..8 (2) */
  int32_t margin;   /* session only: the pair weight's margin, 0..16 (4) */
  int32_t pad_;
} of_inpaint_opts;
/* grow(a | b, g), b may be NULL, g 0..24: out_mask H x W bytes (0 / 1) and / or
 * out_weight H x W fp32 (0.0f where the grown mask is set, else 1.0f, the pair
 * weight when a and b are two frames' grown masks); either may be NULL, not
 * both */
int of_mask_grow(of_ctx *ctx, const uint8_t *a, const uint8_t *b, int H, int W, int g, uint8_t *out_mask,
                 float *out_weight);
/*
 *   frames     : T x H x W x C, C 1..4
 *   masks      : T x H x W bytes as the caller drew them; grown by opts->grow inside
 *   fw, bw     : (T-1) x 2 x H x W, pair s = frames (s, s+1); NULL allowed when T == 1
 *   t          : the frame to fill, 0 .. T-1
 *   out        : H x W x C
 *   out_status : H x W bytes, or NULL
 *   out_hops   : 2 x H x W bytes (df, db), or NULL
 */
int of_inpaint_fill(of_ctx *ctx, const float *frames, const uint8_t *masks, const float *fw, const float *bw, int T,
                    int H, int W, int C, int t, const of_inpaint_opts *opts, float *out, uint8_t *out_status,
                    uint8_t *out_hops);
/*
 * The inpainter session: one per context, beside the other kinds; a delayed
 * emitter of radius opts->radius like the denoiser.  It keeps the last
 * 2 radius + 1 frames and grown masks and both flows of the last 2 radius
 * adjacent pairs on the device; its buffers count in OF_OPT_DEVICE_BYTES from
 * open to close.  C is 1 or 3.  A push stores the frame and grow(mask, grow)
 * and, from the second frame on, estimates the pair (previous, this): the pair
 * weight w is built on the device and both directions are estimated from zero
 * flows with a fresh copy of the open's params, bitwise
 * of_estimate_flow_weighted(previous, this, w) and
 * of_estimate_flow_weighted(this, previous, w).  Open therefore refuses what
 * that entry refuses (a general spatial_filters list, AltBA: OF_ENOTSUP).
 * Frame t is emitted, once frame t + radius is in or at the flush, as
 * of_inpaint_fill of that frame with the frames and pairs within radius that
 * exist; a clip of one frame comes back as it is, its marked pixels
 * OF_INPAINT_UNFILLED.  out: H x W x C; out_status: H x W bytes or NULL;
 * *out_index: the emitted frame or -1.  A push after a flush and a second open
 * are refused (OF_EINVAL).  It is not a kind of_session_set_flow_scale takes.
 */
int of_inpaint_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_inpaint_opts *opts);
int of_inpaint_push(of_ctx *ctx, const float *frame, const uint8_t *mask, float *out, uint8_t *out_status,
                    int32_t *out_index);
int of_inpaint_flush(of_ctx *ctx, float *out, uint8_t *out_status, int32_t *out_index);
int of_inpaint_close(of_ctx *ctx);

/*
 * Gradient-domain blending and the spatial fallback of the inpainter: a
 * Poisson solve over the hole (Perez et al. 2003, as in Huang et al. 2016 and
 * Xu et al. 2019).  The propagated colours supply the gradients and the
 * frame's own pixels around the hole the boundary values, so an exposure
 * offset of a source frame is spread through the hole instead of sitting at
 * its rim; where no colour was propagated the gradients are zero and the same
 * solve gives a smooth membrane.  Everything in double from the fp32 or byte
 * inputs, no fma contraction, in exactly the order written (a numpy float64
 * restatement gives the same bits).  H * W >= 2^31: OF_ENOTSUP.  Any option out
 * of range: OF_EINVAL, checked on the host before any launch.
 *
 * The linear problem, per channel on an H x W frame: a label plane (OF_PSN_FIXED,
 * OF_PSN_UNKNOWN, OF_PSN_EXCLUDED), a value plane v (the Dirichlet data where
 * fixed, the start value where unknown), a source plane s and a byte plane h
 * ("has a source"; both may be NULL: no guidance).  For an unknown p, N(p) is
 * its 4-neighbours inside the frame that are not excluded, in the order up,
 * down, left, right, and deg = |N(p)|:
 *   deg x_p - sum_{n in N(p), unknown} x_n = g_p + f_p
 *   g = 0.0; for n in N(p) with h_p and h_n:  g = g + (s_p - s_n)
 *   f = 0.0; for n in N(p), fixed:            f = f + v_n
 *   b_p = g + f
 * deg = 0: x_p = v_p; fixed and excluded pixels come back as v.
 *
 * The solver is a fixed multigrid schedule of elementwise steps: no reduction,
 * no stopping test, so it depends on (H, W, options) alone and its result is
 * a function of the inputs to the bit.  A component of unknowns without a
 * fixed neighbour is singular and gets no special case: what the schedule
 * makes of the start values is the result.
 *   Levels.  Level l has ceil(H / 2^l) x ceil(W / 2^l) cells, cell (I, J) of
 *   level l+1 covering cells 2I, 2I+1 x 2J, 2J+1 of level l (anchored at the
 *   frame's origin, cells outside the frame excluded); L is the first level
 *   with (rows + 2) * (columns + 2) <= 1024.  A cell has an integer diagonal d
 *   (0: not solved for) and integer weights w towards up, down, left, right.
 *   Level 0: d = deg on the unknown pixels, w = 1 towards an unknown
 *   neighbour.  Level l+1, the Galerkin operator of piecewise-constant
 *   transfer, from the children c00 c01 / c10 c11:
 *     up = up(c00) + up(c01); down = down(c10) + down(c11)
 *     left = left(c00) + left(c10); right = right(c01) + right(c11)
 *     d = d(c00) + d(c01) + d(c10) + d(c11)
 *         - 2 (right(c00) + right(c10) + down(c00) + down(c01))
 *   Sweep (red-black Gauss-Seidel).  For colour k = 0, then 1, every cell with
 *   d > 0 and (row + column) & 1 == k at once:
 *     t = b; for n = up, down, left, right with w_n != 0: t = t + (double)w_n * x_n
 *     x = t / (double)d
 *   Residual of a cell with d > 0 (0.0 elsewhere):
 *     r = b - (double)d * x; for n as above: r = r + (double)w_n * x_n
 *   cycle(l), l < L: `sweeps` sweeps; the next level's b = ((r(c00) + r(c01)) +
 *   r(c10)) + r(c11) where its d > 0, else 0.0, and its x = 0.0; cycle(l+1),
 *   and once more when l + 1 < L (a W-cycle); x = x + 1.5 * x_parent on the
 *   cells with d > 0 (1.5: the Galerkin correction of piecewise-constant
 *   transfer undershoots smooth errors by about half; measured in
 *   DESIGN.md); `sweeps` sweeps.  cycle(L): `coarse_sweeps` sweeps.
 *   The solve: x = v, then `cycles` times cycle(0).
 * The library works on a window around the unknowns only; cells without an
 * unknown change nothing, so the window is invisible in the result.
 *
 * Blended fill of frame t (of_inpaint_blend; inputs as of_inpaint_fill).  (s, st)
 * = of_inpaint_fill of frame t with grow + 1 (a propagated colour on the
 * one-pixel ring around the hole as well: the boundary gradients), h = (st ==
 * OF_INPAINT_FILLED), Om = grow(M_t, grow), I the frame.
 *   Stage 1: unknown = Om & h, excluded = Om & !h, fixed elsewhere with value
 *            I; start s; guidance (s, h).
 *   Stage 2: unknown = Om & !h, everything else fixed at stage 1's result (in
 *            double); start I; no guidance.  Skipped when Om is empty; where
 *            Om & !h is empty it changes nothing.
 *   out = (float) of the result on Om, I elsewhere; status OF_INPAINT_KEPT
 *   outside Om, OF_INPAINT_FILLED on Om & h, OF_INPAINT_SPATIAL on Om & !h;
 *   OF_INPAINT_UNFILLED never appears.
 *
 * Known limits: the membrane is smooth, no texture is synthesised; a gain
 * change scales the copied gradients and is only partly corrected (on the
 * tests' scene with 3 % per frame, a mean squared error of 120 becomes 24);
 * colours from different source frames meet inside the hole with their
 * gradient seams left as they are; a region that touches a single fixed pixel
 * converges slowly (the coarsest level is relaxed, not solved).
 */
#define OF_INPAINT_SPATIAL 3
#define OF_PSN_FIXED 0
#define OF_PSN_UNKNOWN 1
#define OF_PSN_EXCLUDED 2
#define OF_BLEND_MAX_CYCLES 64
#define OF_BLEND_MAX_SWEEPS 2
#define OF_BLEND_MAX_COARSE_SWEEPS 64
typedef struct of_blend_opts {
  int32_t cycles;         /* W-cycles of a solve, 1..64 (8) */
  int32_t sweeps;         /* red-black sweeps before and after the coarse correction, 1..2 (2) */
  int32_t coarse_sweeps;  /* sweeps of the coarsest level per visit, 1..64 (32) */
  int32_t pad_;
} of_blend_opts;
/*
 *   label      : H x W bytes, OF_PSN_* (anything else: OF_EINVAL)
 *   values     : H x W x C interleaved, C 1..4
 *   source     : H x W x C, or NULL
 *   has_source : H x W bytes (nonzero = has a source), NULL exactly when source is
 *   out        : H x W x C doubles
 */
int of_poisson_solve(of_ctx *ctx, const uint8_t *label, const float *values, const float *source,
                     const uint8_t *has_source, int H, int W, int C, const of_blend_opts *opts, double *out);
/* arguments as of_inpaint_fill, without the hop counts */
int of_inpaint_blend(of_ctx *ctx, const float *frames, const uint8_t *masks, const float *fw, const float *bw, int T,
                     int H, int W, int C, int t, const of_inpaint_opts *opts, const of_blend_opts *blend, float *out,
                     uint8_t *out_status);
/*
 * Blending in the inpainter session: valid after of_inpaint_open and before
 * the first push, otherwise OF_EINVAL; NULL turns it off again.  With it set
 * every emitted frame is of_inpaint_blend of that frame instead of
 * of_inpaint_fill; the masks grown by one more are kept beside the ring's and
 * count in OF_OPT_DEVICE_BYTES from this call to the close, the solver's
 * buffers come from the context's grow-only arena.  Without it the pushes are
 * bitwise what they are without this call.
 */
int of_inpaint_set_blend(of_ctx *ctx, const of_blend_opts *blend);

/*
 * Mask propagation: a marked object followed through a clip.  The binary mask
 * of the previous frame is carried to the current one along the backward flow
 * (current -> previous); a pixel whose flow cannot be trusted is decided by a
 * colour-guided vote of its decided neighbours; a pixel with no decided
 * neighbour stays unmarked and is reported as such; a small mode filter cleans
 * the result.  of_masks_* followed by of_inpaint_* removes an object from one
 * drawn mask.  Everything in double from the fp32 or byte inputs, no fma
 * contraction, in exactly the order written (a numpy float64 restatement gives
 * the same bits); bil and inside as defined above ("Using a flow on an image").
 *   M : the previous mask, H x W bytes, nonzero = marked
 *   G : the current frame, H x W x C interleaved fp32, C 1..4, the guide
 *   B : the flow current -> previous, planar 2 x H x W
 *   S : the forward-backward state of B, H x W bytes in of_fb_consistency's
 *       encoding, or NULL (all 0)
 * H * W >= 2^31: OF_ENOTSUP.  Any option out of range or not finite: OF_EINVAL,
 * checked on the host before any launch (every entry checks the whole struct).
 *
 * Carry.  m = (M != 0) as 0.0 / 1.0; (u, v) = B(i,j).  Pixel (i, j) is decided
 * when u and v are finite, inside(i + v, j + u) holds and S(i,j) == 0:
 *   A(i,j) = (float)bil(m, i + v, j + u); label = A >= 0.5f; status OF_MASK_CARRIED
 * Otherwise it is undecided and A(i,j) = -1.0f.
 *
 * Vote.  For each undecided pixel p = (i, j), with R = vote_radius: di = -R..R
 * in the outer loop, dj = -R..R in the inner one, starting from num = den = 0.0
 * and cnt = ones = 0; for every n = (i + di, j + dj) inside the frame that is
 * decided:
 *   D = 0.0; D = D + (G_c(p) - G_c(n))*(G_c(p) - G_c(n)) for c ascending; D = D / C
 *   z = D / (range*range)
 *   w = z < 1 ? (1 - z)*(1 - z) : 0                  (a non-finite G: z < 1 is false)
 *   num = num + w*(double)A(n); den = den + w; cnt += 1; ones += A(n) >= 0.5f
 * Then
 *   den > 0         : label = num >= 0.5*den,  status OF_MASK_VOTED
 *   else cnt > 0    : label = 2*ones >= cnt,   status OF_MASK_VOTED
 *   else            : label = 0,               status OF_MASK_UNKNOWN
 *
 * Smooth.  One pass with radius s = smooth over the labels (s = 0: none): over
 * the (2s+1)^2 window clipped to the frame, k = the labels equal to 1 and n =
 * the window's pixels, all integer:
 *   2k > n: 1;  2k < n: 0;  otherwise the pixel's own label
 * The status plane is not touched.
 *
 * Known limits.  The vote needs colour contrast between object and
 * surroundings: on the synthetic scene of the tests the mean IoU over 8 frames
 * is 0.84 without and 0.98 with it (tests/test_mask_cpu.py); and it can only
 * spread labels that some decided pixel carries, so an object whose whole area
 * is undecided in one pair is lost from then on.  The labels are
 * thresholded at every step, so the outline drifts over long clips: re-anchor
 * with a keyframe.  smooth = 1 rounds corners (a 14 x 18 rectangle loses its 4
 * corner pixels).  One object per call.  No scale, batch or stream variant.
 */
#define OF_MASK_CARRIED 0
#define OF_MASK_VOTED 1
#define OF_MASK_UNKNOWN 2
#define OF_MASK_GIVEN 3
#define OF_MASK_MAX_VOTE_RADIUS 12
#define OF_MASK_MAX_SMOOTH 2
typedef struct of_mask_opts {
  int32_t vote_radius;   /* R of the vote's window, 1..12 (8) */
  int32_t smooth;        /* s of the mode filter, 0..2 (1) */
  double range;          /* the vote's colour range on the frames' value scale, like of_upsample_opts; finite, > 0 (20) */
  double alpha1, alpha2; /* session only: forward-backward test, as of_fb_consistency; >= 0 */
} of_mask_opts;
/*
 *   prev_mask  : H x W bytes
 *   guide      : H x W x C, C 1..4
 *   flow       : 2 x H x W, current -> previous
 *   state      : H x W bytes, or NULL
 *   out_mask   : H x W bytes, 0 / 1
 *   out_status : H x W bytes, or NULL
 */
int of_mask_advance(of_ctx *ctx, const uint8_t *prev_mask, const float *guide, int H, int W, int C, const float *flow,
                    const uint8_t *state, const of_mask_opts *opts, uint8_t *out_mask, uint8_t *out_status);
/*
 * The mask propagator session: one per context, beside the other kinds.  It
 * keeps the previous frame and the current mask on the device; its buffers
 * count in OF_OPT_DEVICE_BYTES from open to close, and of_ctx_destroy closes
 * it.  C is 1 or 3.  A push with a mask (the first frame, or a re-anchor
 * later) stores mask != 0, returns it with status OF_MASK_GIVEN everywhere and
 * estimates nothing; the first push without a mask is OF_EINVAL.  A push
 * without a mask estimates the pair (previous, this) in both directions at full
 * resolution from zero flows with a fresh copy of the open's params and
 * advances the stored mask along the backward flow with its state: bitwise
 *   fw, bw, state_fw, state_bw = of_estimate_flow_bidir(previous, this; alpha1, alpha2)
 *   out_mask, out_status = of_mask_advance(mask, this, bw, state_bw)
 * out_mask: H x W bytes; out_status: H x W bytes or NULL.  A second open is
 * refused (OF_EINVAL).  It is not a kind of_session_set_flow_scale takes: its
 * pairs are estimated at full resolution.
 */
int of_masks_open(of_ctx *ctx, const of_params *params, int H, int W, int C, const of_mask_opts *opts);
int of_masks_push(of_ctx *ctx, const float *frame, const uint8_t *mask, uint8_t *out_mask, uint8_t *out_status);
int of_masks_close(of_ctx *ctx);

/*
 * Blind temporal consistency: the flicker of a per-frame operator removed
 * (Bonneel et al. 2015; Lai et al. 2018 without the network).  Beside the clip
 * V there is a second clip P, the same frames after an operator that knows
 * nothing about time (tone mapping, grading, dehazing, colourisation, ...):
 * every frame of P looks right, the clip flickers.  Output frame t keeps the
 * gradients of P_t and leans, where the original frames say the surface is
 * the same, on the previous output warped along the backward flow: a screened
 * Poisson problem per frame.  Everything in double from the fp32 or byte
 * inputs, no fma contraction, in exactly the order written (a numpy float64
 * restatement gives the same bits); bil and inside as defined above ("Using a
 * flow on an image").  H * W >= 2^31: OF_ENOTSUP.  Any option out of range or
 * not finite: OF_EINVAL, checked on the host before any launch (every entry
 * checks the whole struct).
 *
 * The screened problem, per channel on an H x W frame: a target plane P (fp32,
 * whose gradients are wanted), an anchor plane A (fp64) and a screening plane
 * q >= 0 (fp64).  For pixel p, N(p) is its 4-neighbours inside the frame in
 * the order up, down, left, right, and deg = |N(p)|:
 *   (deg + q_p) x_p - sum_{n in N(p)} x_n = b_p
 *   g = 0.0; for n in N(p):  g = g + (P_p - P_n)
 *   b_p = g + q_p * A_p
 * The start value is x = P.  With q == 0 everywhere the start's residual is
 * exactly 0 (the differences and sums of fp32 values of one scale are exact in
 * double) and the result is P to the bit; that singular case gets no special
 * handling.  A 1 x 1 frame has deg = 0: x = (q * A) / q if q > 0, else P.
 *
 * The solver is the fixed W-cycle schedule of "Gradient-domain blending" above,
 * with no reduction and no stopping test: a function of (H, W, options) alone.
 *   Levels and L as there.  Every level's window is its whole grid plus an
 *   apron of one cell of level L on every side, anchored at the frame's origin.
 *   d and w are those of the all-unknown problem (level 0: d = deg, w = 1
 *   towards a neighbour inside the frame; 0 outside the frame), their Galerkin
 *   coarsening the one stated there.  A double plane q per level is new: level
 *   0 as given (0.0 outside the frame), level l+1 the Galerkin term of
 *   piecewise-constant transfer,
 *     q = ((q(c00) + q(c01)) + q(c10)) + q(c11)
 *   A cell is solved for where (double)d + q > 0.
 *   Sweep (red-black, colour k = 0, then 1, as there):
 *     t = b; for n = up, down, left, right with w_n != 0: t = t + (double)w_n * x_n
 *     x = t / ((double)d + q)
 *   Residual of a solved cell (0.0 elsewhere):
 *     r = b - ((double)d + q) * x; for n as above: r = r + (double)w_n * x_n
 *   Restriction, the correction x = x + 1.5 * x_parent (on the cells with
 *   d > 0; 1.5 was measured again for this operator against 1.0 and 1.25,
 *   DESIGN.md) and the cycle as there.  The solve: x = P, then `cycles` times
 *   cycle(0).
 * The options are an of_blend_opts with its ranges; OF_CONSIST_CYCLES (5) is
 * the cycle count at which every convergence case of the tests (q in patches
 * of 0, 1e-3, 1 and 1e3) and the tests' scene are within half an 8-bit level
 * of the exact solution.
 *
 * The consistency step of frame t: the frame V_t and its predecessor V_{t-1}
 * (H x W x C, C 1..4), the processed frame P_t (H x W x Cp, Cp 1..4,
 * independent of C: a grey clip can be colourised), the previous output
 * O_{t-1} (H x W x Cp fp32, as emitted), the flow f from t to t-1 and its
 * forward-backward state s (NULL: all 0).  With (u, v) = f(i, j):
 *   w   = of_fuse_weights(center V_t, one neighbour V_{t-1}, flow f, state s;
 *         sigma, strength, patch), a float plane
 *   vis = u, v finite && inside(i + v, j + u) && s(i,j) == 0       (w's own rule)
 *   q   = lambda * (double)w where vis, else 0.0
 *   A_c = bil(O_{t-1,c}, i + v, j + u) where vis, else 0.0
 *   O_t = (float) of the screened solve of (P_t, A, q), per channel
 *   out_weight = w       (where the output leans on the past)
 * lambda is finite and >= 0 (1).  At 0 the step returns P_t to the bit; a
 * large lambda returns the warped previous output where it is visible.  sigma
 * is what the original frames may differ by where they show the same surface.
 *
 * Known limits.  The first frame's look is the anchor and errors accumulate
 * along a long clip: lambda trades flicker against drift, and there is no
 * long-term keyframe.  Where the forward-backward state or the weight rejects
 * the past the pixel follows the processed frame alone, so newly revealed
 * regions can still flicker.  Causal: no look-ahead.  No scale, batch or
 * stream variant.
 */
#define OF_CONSIST_CYCLES 5
#define OF_CONSIST_MAX_CHANNELS 4
typedef struct of_consist_opts {
  of_fuse_opts fuse;    /* sigma, strength, patch of the weight; alpha1, alpha2 session only; radius is not read */
  of_blend_opts solve;  /* the solver's cycles (5), sweeps (2), coarse_sweeps (32) */
  double lambda;        /* the weight of the past, finite, >= 0 (1) */
} of_consist_opts;
/*
 * of_screened_solve: the solver on its own.
 *   target : H x W x C interleaved fp32, C 1..4
 *   anchor : H x W x C doubles
 *   weight : H x W doubles, the plane q; a negative or non-finite value: OF_EINVAL
 *   out    : H x W x C doubles
 */
int of_screened_solve(of_ctx *ctx, const float *target, const double *anchor, const double *weight, int H, int W,
                      int C, const of_blend_opts *opts, double *out);
/*
 *   frame, prev_frame : H x W x C
 *   processed         : H x W x Cp
 *   prev_out          : H x W x Cp
 *   flow              : 2 x H x W, frame -> prev_frame
 *   state             : H x W bytes, or NULL
 *   out               : H x W x Cp
 *   out_weight        : H x W, or NULL
 */
int of_consist_step(of_ctx *ctx, const float *frame, const float *prev_frame, int H, int W, int C,
                    const float *processed, const float *prev_out, int Cp, const float *flow, const uint8_t *state,
                    const of_consist_opts *opts, float *out, float *out_weight);
/*
 * The temporal consistency session: one per context, beside the other kinds.
 * It keeps the previous frame V_{k-1} and the previous output O_{k-1} on the
 * device; their bytes count in OF_OPT_DEVICE_BYTES from open to close, and
 * of_ctx_destroy closes it.  C is 1 or 3, Cp 1..4.  It is not a delayed
 * emitter: push k returns output k.  Push 0 returns `processed` to the bit
 * (out_weight 0 everywhere).  Push k > 0 estimates the pair (k-1, k) in both
 * directions at full resolution from zero flows with a fresh copy of the
 * open's params and runs the step along the backward flow with its state:
 * bitwise
 *   fw, bw, state_fw, state_bw = of_estimate_flow_bidir(V_{k-1}, V_k; alpha1, alpha2)
 *   out, out_weight = of_consist_step(V_k, V_{k-1}, processed, O_{k-1}, bw, state_bw)
 * out: H x W x Cp; out_weight: H x W or NULL.  A second open is refused
 * (OF_EINVAL), as are push and close without an open session.  It is not a
 * kind of_session_set_flow_scale takes (there is no OF_SESSION_* bit for it):
 * its pairs are estimated at full resolution.
 */
int of_consist_open(of_ctx *ctx, const of_params *params, int H, int W, int C, int Cp, const of_consist_opts *opts);
int of_consist_push(of_ctx *ctx, const float *frame, const float *processed, float *out, float *out_weight);
int of_consist_close(of_ctx *ctx);

/*
 * Layered motion segmentation.  of_fit_motion finds one motion, the dominant
 * one; of_segment_motion splits a flow into up to K parametric motions of one
 * model, a label per pixel and a class for what no motion explains
 * (OF_LAYER_NONE): hypotheses from a grid of cells, consensus extraction of one
 * layer after the other, joint assign-and-refit rounds, a mode filter on the
 * labels.  No session.  Everything in double from the fp32 inputs, no fma
 * contraction, in exactly the order written; coordinates, models, w0, the 13
 * sums with their order, the solve with its rank-loss fallback and the matrix
 * are those of "Global motion estimation" above.  H * W >= 2^31: OF_ENOTSUP.
 *
 * Per pixel: s, cx, cy, x, y and w0 as in the fit.  r2(th, p) is the fit's r2
 * of pixel p against th, (th0 + th1*x) + th2*y and so on, with the pixel's own
 * (u, v).  A pixel is usable when w0 > 0; total = the number of usable pixels.
 * c2 = cutoff*cutoff.  "count reaches the support" is
 * !((double)count < min_support*(double)total).  Counts are integers.
 * A pass "on a set M" is a pass k >= 1 of the fit with the cutoff c2 (never
 * updated) in which every pixel outside M counts as masked by `state`:
 * w = w0*[p in M]*((1 - t)*(1 - t)), t = min(r2/c2, 1.0).
 *
 * 1. Hypotheses.  Pass 0 of the fit (th = 0, w = w0) gives the 13 values of
 *    every 8 x 64 tile; nty, ntx are the tile counts, g = grid,
 *    ch = ceil(nty/g), cw = ceil(ntx/g).  Cell (a, b), 0 <= a, b < g, owns tile
 *    rows [a*ch, min((a+1)*ch, nty)) and tile columns [b*cw, min((b+1)*cw, ntx));
 *    an empty cell does not exist.  Each of a cell's 13 sums is its tiles'
 *    values, in row-major order inside the cell, reduced by the group tree
 *    (zero-padded to a multiple of 64, each group of 64 through the halving
 *    tree, until one value is left).  Sw > 0: hypothesis a*g + b is the solve
 *    of the model on those sums (a rank loss solves the translation);
 *    otherwise the cell has no hypothesis.
 * 2. Extraction, for l = 0 .. K-1, rem = the usable pixels not yet removed.
 *    count_h = #{p in rem : r2(th_h, p) < c2} for every hypothesis h; h* has
 *    the largest count, the lowest index on a tie.  No hypothesis, or count_h*
 *    does not reach the support: stop.  th = th_h*; `passes` passes on rem,
 *    each solved as in the fit; !(Sw > 0) ends the passes and keeps th.
 *    inl = {p in rem : r2(th, p) < c2}.  #inl does not reach the support: the
 *    layer is discarded and the extraction stops.  Otherwise th is layer l and
 *    rem -= inl.  n = the layers extracted; they keep this order.
 * 3. Joint rounds, `rounds` times: assign, then for every layer l one pass on
 *    {usable p : label(p) = l}, solved when Sw > 0 (else th_l is kept).
 *    Assign: a pixel whose u and v are finite, whatever its weight or state,
 *    gets the layer with the smallest r2(th_l, p), the lowest l on a tie, if
 *    that r2 < c2, and OF_LAYER_NONE otherwise; a pixel whose flow is not
 *    finite gets OF_LAYER_NONE.  After the rounds the closing assignment
 *    (labels_raw) and per layer one pass on its set that does not solve:
 *    support = Sw, rms = sqrt(Sr/Sw) (NaN without support).  n = 0 is a valid
 *    result: every label is OF_LAYER_NONE.
 * 4. Mode filter, r = smooth > 0: the label of (i, j) becomes the value among
 *    0 .. n-1, 255 that occurs most often in the in-frame part of the
 *    (2r+1) x (2r+1) window of labels_raw around it, the smallest value on a
 *    tie (so OF_LAYER_NONE loses ties).  One pass.  r = 0: labels = labels_raw.
 *    pixels counts the returned plane.
 * degenerate of a layer: 1 when the solve of its hypothesis or of one of its
 * passes lost rank.
 *
 * Known limits.  A hypothesis cell is never finer than one 8 x 64 tile, so a
 * layer without a nearly pure cell is found late or not at all: a 40 x 70
 * frame split at 0.55 W lost the translation case, 67 x 131 and larger held at
 * grid 8.  The smeared band along a motion boundary of an estimated flow
 * comes out OF_LAYER_NONE, and on small frames as a thin extra layer once it
 * exceeds min_support.
 */
#define OF_LAYER_NONE 255
/* Any value out of range or not finite: OF_EINVAL, checked on the host before
 * any launch. */
typedef struct of_layers_opts {
  int32_t model;        /* OF_MOTION_*, 0..2 */
  int32_t max_layers;   /* K, 1..8 (4) */
  int32_t grid;         /* g, hypothesis cells per axis, 1..16 (8) */
  int32_t passes;       /* Tukey refits of an extracted layer, 0..16 (4) */
  int32_t rounds;       /* joint assign-and-refit rounds, 0..16 (3) */
  int32_t smooth;       /* radius of the label mode filter, 0..3 (2) */
  double cutoff;        /* c, pixels, finite, > 0 (1.0) */
  double min_support;   /* fraction of the usable pixels a layer must explain, (0, 1] (0.03) */
} of_layers_opts;
typedef struct of_motion_layer {
  double theta[6];
  double matrix[6];
  double support;       /* Sw of the closing pass */
  double rms;           /* sqrt(Sr/Sw) of the closing pass */
  int64_t pixels;       /* pixels that carry this label in the returned plane */
  int32_t degenerate;   /* 1: a solve of this layer lost rank */
  int32_t pad_;
} of_motion_layer;
/*
 *   uv, weight, state : as of_fit_motion
 *   layers            : max_layers entries; the first *n_layers are written
 *   labels            : H x W bytes, 0 .. n-1 or OF_LAYER_NONE
 *   labels_raw        : H x W bytes, the labels before the mode filter, or NULL
 */
int of_segment_motion(of_ctx *ctx, const float *uv, int H, int W, const float *weight, const uint8_t *state,
                      const of_layers_opts *opts, of_motion_layer *layers, int32_t *n_layers, uint8_t *labels,
                      uint8_t *labels_raw);

/* compute_flow_base() for one pyramid level with the given alpha (one call =
 * all warping iterations of the level; hs.py:109-142, ba.py:143-206,
 * classic_nl.py:200-277).  uv_in / out_uv planar 2 x H x W. */
int of_compute_flow_base(of_ctx *ctx, of_params *params, const float *images, int H, int W, int nc,
                         const float *guide, int gc, double alpha, const float *uv_in, float *out_uv);
/* AltBAOpticalFlow.compute_flow_base(uv, uvhat) (alt_ba.py:189-274): one
 * level of the coupled IRLS (lambda2 annealed 1e-4 -> lambda2 over max_iters
 * warps, coupling weights rho_couple'(uv - uvhat)/x, Li-Osher median update
 * of uvhat, uv <- uvhat when `replacement`); uv, uvhat in and out are planar
 * 2 x H x W */
int of_alt_ba_flow_base(of_ctx *ctx, of_params *params, const float *images, int H, int W, int nc, double alpha,
                        int replacement, const float *uv, const float *uvhat, float *out_uv, float *out_uvhat);

/* ---- device-resident batch path (benchmark / multi-GPU sharding) ---- */
/* upload one RGB/gray pair into slot `slot` of the ctx (H2D, untimed) */
int of_pair_upload(of_ctx *ctx, int slot, const float *im1, const float *im2, int H, int W, int C);
/* run estimate_flow on device-resident slot; result stays on device */
int of_pair_run(of_ctx *ctx, int slot, of_params *params, of_stats *stats);
/* run estimate_flow on slots 0..nslots-1 with `lanes` concurrent pipelines
 * (1..16; each its own HIP stream, device arena and solver state, driven by
 * its own host thread; slot s runs on lane s % lanes).  params is copied per
 * slot and not written back; stats (may be NULL) receives slot 0's.  Returns
 * when every slot is done.  Results: lanes == 1 is bitwise estimate_flow;
 * lanes >= 2 are bitwise equal to each other, and equal to estimate_flow for
 * pairs below 2^20 px; at >= 2^20 px their fine CG solves run two pairs side
 * by side in a different block geometry, so they differ from estimate_flow
 * by CG rounding only (both meet the 1e-6 true residual). */
int of_pairs_run(of_ctx *ctx, int nslots, const of_params *params, int lanes, of_stats *stats);
/* host-to-host batch (the SURVEY.md §8d headline; replaces a Python loop of
 * estimate_flow(im1[k], im2[k], method) calls, interface.py:11-71): reads
 * npairs caller-owned (H, W, C) uint8 frame pairs (C = 1 or 3), writes each
 * pair's flow as planar 2 x H x W fp32 into out_uv[k].  `lanes` pairs in
 * flight as in of_pairs_run; per lane the H2D of pair j+1's bytes and the
 * D2H of pair j-1's flow overlap pair j's kernels (pinned double buffers, one
 * copy stream shared by the lanes).  The flows also stay on the device in
 * slots 0..npairs-1 (of_pair_download, of_rccl_gather_flows); frames an
 * earlier of_pair_upload left in those slots are released (re-upload before
 * of_pair_run / of_pairs_run).  Results equal of_pairs_run on the same frames
 * with the same `lanes` (bitwise; see of_pairs_run for the lanes contract). */
int of_pairs_run_host(of_ctx *ctx, int npairs, const uint8_t *const *im1, const uint8_t *const *im2, int H, int W,
                      int C, const of_params *params, int lanes, float *const *out_uv, of_stats *stats);
/*
 * Streaming host-to-host batch (the reference's per-pair loop over files,
 * flo_io.py:46-113 / metrics.py:5-53, with host I/O overlapped): a pool of
 * `lanes` pipelines (child contexts, one host thread each; lanes >= 2 share
 * the fine-solve token as of_pairs_run) takes (H, W, C) uint8 pairs from a
 * queue, so the lanes never drain between the caller's submissions.
 *   of_pairs_open   start the pool for one frame shape and parameter set
 *   of_pairs_submit queue n pairs; returns at once; the caller keeps im1[k],
 *                   im2[k] and out_uv[k] (planar 2 x H x W fp32) alive until
 *                   the pair is waited for; *first_ticket (may be NULL)
 *                   receives the first pair's ticket, the others follow
 *   of_pairs_wait   block until that pair's flow is in its out_uv
 *   of_pairs_close  finish the queued pairs, stop and free the pool
 * Flows equal of_pairs_run_host's with the same `lanes` bitwise.  While a
 * stream is open the context's compute entries (of_pairs_run,
 * of_pairs_run_host, the stage entries ...) and its settings and profiling
 * calls (of_set_option, of_set_profiling, of_set_solve_log, of_kernel_times,
 * of_kernel_timeline) return OF_EINVAL: lane 0 of the pool is the context.
 */
int of_pairs_open(of_ctx *ctx, int H, int W, int C, const of_params *params, int lanes);
int of_pairs_submit(of_ctx *ctx, int n, const uint8_t *const *im1, const uint8_t *const *im2, float *const *out_uv,
                    int64_t *first_ticket);
int of_pairs_wait(of_ctx *ctx, int64_t ticket);
int of_pairs_close(of_ctx *ctx);
/* the same pool over device-resident pairs: queue the pairs of n slots of
 * this context (of_pair_upload; frame size = the stream's); each flow stays
 * in its slot (of_pair_download, of_rccl_gather_slots).  A slot queued and
 * not yet finished is refused by of_pairs_submit_slots, of_pair_upload and
 * of_pair_download (OF_EINVAL) until its ticket is done.  Tickets
 * share the host submissions' sequence; flows equal of_pairs_run's with the
 * same `lanes` bitwise (the bench's HBM-resident rate: consecutive batches
 * queued back to back, so the lanes never drain between them). */
int of_pairs_submit_slots(of_ctx *ctx, int n, const int *slots, int64_t *first_ticket);
/* D2H of a slot's flow (planar 2 x H x W) */
int of_pair_download(of_ctx *ctx, int slot, float *out_uv);

/* ---- RCCL gather of device-resident results (one process per GPU) ---- */
int of_rccl_unique_id(char *out128);
int of_rccl_init(of_ctx *ctx, const char *id128, int nranks, int rank);
/* gather `nslots` flows (slots 0..nslots-1 of every rank) to rank 0; rank 0's
 * out_uv receives nranks*nslots planar flows (may be NULL on other ranks) */
int of_rccl_gather_flows(of_ctx *ctx, int nslots, float *out_uv_rank0);
/* the same for slots first..first+nslots-1 (rank r's slot first+s lands at
 * flow r*nslots + s) */
int of_rccl_gather_slots(of_ctx *ctx, int first, int nslots, float *out_uv_rank0);
int of_rccl_finalize(of_ctx *ctx);

/* ---- solver diagnostics ---- */
/* Launch geometry of the iterative solver kernels for an H x W level (no
 * device needed): CG ('backslash' k_cgs, 'pcg' k_cg) strips x bands, or the
 * SOR kernel's 64-row strips (grid_x = 2 * strips).  OF_ENOTSUP when the
 * level is too large for the kernel (too wide for the partial-sum slots /
 * too tall for the SOR hand-off words). */
typedef struct of_cg_geometry {
  int32_t grid_x, grid_y;  /* launch grid (blocks) */
  int32_t rows;            /* rows per band */
  int32_t bands;
  int32_t blocks;          /* grid_x * grid_y */
  int32_t strip_cols;      /* output columns of the widest strip (k_cgs: an
                            * edge strip, 120; 128 when one strip covers
                            * the level; interior strips 112) */
} of_cg_geometry;
int of_solver_geometry(int H, int W, int solver, of_cg_geometry *out);

/* Solve log: with it on, every linear solve (_solve_linear_system,
 * base.py:87-172) is followed by an fp64 evaluation of its TRUE relative
 * residual ||b - A x|| / ||b|| from the fp32 operator; records keep the
 * solver's own estimate beside it (CG: the recurrence residual; SOR: the
 * last sweep's ||dx|| / ||x||).  true_rel is the residual of the solver's
 * iterate ('backslash': x_hi + x_lo summed in fp64 after its residual
 * replacement, the quantity its stopping test approximates), true_rel_out
 * that of the fp32 x it returns (the same for 'pcg' and 'sor'; for
 * 'backslash' it includes the rounding of the solution to fp32, whose
 * residual alone is ~2e-6 on Classic+NL robust stages, tools/fp32_floor.py).
 * Enabling clears the log; at most 4096 records per context.  Diagnostic
 * only: adds small launches per solve. */
typedef struct of_solve_record {
  int32_t h, w;
  int32_t solver;   /* enum of_solver */
  int32_t iters;    /* CG iterations / SOR sweeps */
  int32_t done;     /* 1 converged, 2 iteration limit, 3 zero rhs */
  int32_t pad_;
  double true_rel;      /* ||b - A x|| / ||b||, fp64, of the solver's iterate */
  double est_rel;
  double true_rel_out;  /* ... of the returned fp32 x */
} of_solve_record;
int of_set_solve_log(of_ctx *ctx, int enable);
int of_solve_log(of_ctx *ctx, int max, of_solve_record *out, int *n);

/* ---- stage entries (one per hot-path row of SURVEY.md §8a; parity tests) ---- */
/* _rgb2gray + _rgb2lab + per-channel scale_image (interface.py:49-64,74-141) */
int of_preprocess(of_ctx *ctx, const float *rgb1, const float *rgb2, int H, int W,
                  float *gray_pair /*2xHxW*/, float *lab /*3xHxW*/);
/* structure_texture_decomposition_rof (utils/image_processing.py:52-136) */
int of_rof_texture(of_ctx *ctx, const float *im, int H, int W, int C, double theta, int iters,
                   double alp, float *out);
/* compute_image_pyramid level l+1 from level l (utils/pyramid.py:44-73) */
int of_pyramid_level(of_ctx *ctx, const float *im, int H, int W, int C, const double *kern, int ksize,
                     double ratio, float *out, int *outH, int *outW);
/* resample_flow (utils/warping.py:6-45) */
int of_resample_flow(of_ctx *ctx, const float *uv, int H, int W, int nH, int nW, float *out);
/* partial_deriv (utils/derivatives.py:148-296): images planar 2*nc */
int of_partial_deriv(of_ctx *ctx, const float *images, int H, int W, int nc, const float *uv,
                     int interp, const double *deriv_filter, double blend,
                     float *It, float *Ix, float *Iy);
/* flow_operator, matrix-free (classic_nl.py:279-378, ba.py:208-302, hs.py:144-203):
 * coef = 7 planes {wx_u, wy_u, wx_v, wy_v, a_uu, a_uv, a_vv}, rhs = planes {b_u, b_v}.
 * wx_* / wy_* are the (lambda-scaled) weights of the edge to the right / below. */
int of_flow_operator(of_ctx *ctx, const of_params *params, double alpha, const float *uv,
                     const float *duv, const float *It, const float *Ix, const float *Iy,
                     int H, int W, int nc, float *coef, float *rhs);
/* _solve_linear_system (base.py:87-172) on the matrix-free operator */
int of_solve(of_ctx *ctx, const of_params *params, const float *coef, const float *rhs, int H, int W,
             float *x, int *iters, double *rel_residual);
/* General spatial_filters (params->filters.general): the operator in
 * diagonal (DIA) form on the dense offset grid of radius D = max filter
 * dimension - 1, G = (2D + 1)^2 offsets (di, dj) in row-major order
 * (di = -D..D outer): planes = G planes of the u-u block, G of the v-v
 * block, then the u-v coupling (offset 0); (A x)_u(i, j) = sum_o
 * c_u,o(i, j) x_u(i + di, j + dj) + c_uv(i, j) x_v(i, j).  *D_out receives D
 * (the caller sizes planes as (2 G + 1) H W floats, G from its own filters). */
int of_flow_operator_dia(of_ctx *ctx, const of_params *params, double alpha, const float *uv,
                         const float *duv, const float *It, const float *Ix, const float *Iy,
                         int H, int W, int nc, int *D_out, float *planes, float *rhs);
/* _solve_linear_system (base.py:87-172) on a DIA operator of radius D (any
 * sparse A whose u-u / v-v blocks are 2-D stencils and whose u-v block is
 * diagonal; the Python mirror converts scipy matrices) */
int of_solve_dia(of_ctx *ctx, const of_params *params, int D, const float *planes, const float *rhs,
                 int H, int W, float *x, int *iters, double *rel_residual);
/* detect_occlusion (utils/occlusion.py:6-56) */
int of_detect_occlusion(of_ctx *ctx, const float *uv, const float *images, int H, int W, int nc,
                        float *occ);
/* denoise_color_weighted_medfilt2 (utils/weighted_median.py:24-112) */
int of_weighted_median(of_ctx *ctx, const float *uv, const float *guide, int gc, const float *occ,
                       int H, int W, int area_hsz, double sigma_i, float *out);
/* of_weighted_median with the warping loop's fused duv bookkeeping
 * (classic_nl.py:271-275): base == NULL is of_weighted_median; otherwise
 * out = base + (median - base) in float32, computed in the filter's own store
 * with the result written over the base's buffer, as a Classic+NL warp does. */
int of_weighted_median_base(of_ctx *ctx, const float *uv, const float *guide, int gc, const float *occ,
                            int H, int W, int area_hsz, double sigma_i, const float *base, float *out);
/* ---- stage entries of one level's warping loop (parity tests) ----
 * Each runs exactly the host function of_compute_flow_base runs.
 *
 * of_warp_operator: the fused warp + assembly, the default linearisation of
 * every method but AltBA: the level's derivative planes of `images` (planar
 * 2*nc, interpolation and derivative filter of `params`, `blend` as
 * of_partial_deriv) and then coef / rhs of of_flow_operator_weighted at `uv`
 * with no duv, bitwise what of_partial_deriv + of_flow_operator_weighted
 * give.  weight: H x W or NULL.  OF_ENOTSUP where the level would not fuse:
 * nc not 1 or 3, AltBA, or OF_OPT_FUSED_WARP off. */
int of_warp_operator(of_ctx *ctx, const of_params *params, double alpha, const float *images, int H, int W,
                     int nc, const float *uv, const float *weight, double blend, float *coef, float *rhs);
/* The IRLS update (classic_nl.py:250-262): out_uv1 = uv + clip(x), clip to
 * [-1, 1] when `clip` is non-zero, one float32 rounding; with out_occ also
 * detect_occlusion(out_uv1, images) (utils/occlusion.py:6-56) from the same
 * launch.  images (planar 2*nc) may be NULL when out_occ is. */
int of_flow_update(of_ctx *ctx, const float *uv, const float *x, int clip, const float *images, int H, int W,
                   int nc, float *out_uv1, float *out_occ);
/* scipy.ndimage.median_filter(size, mode='reflect') of both components of a
 * flow field at once (hs.py:137-140, ba.py:197-199); size 3, 5 or 7 */
int of_median_filter_flow(of_ctx *ctx, const float *uv, int H, int W, int size, float *out);
/* flow_to_color (viz/flow_color.py:77-107): Middlebury colour coding of an
 * interleaved (H, W, 2) flow of dtype 0 = float32 or 1 = float64 into an
 * (H, W, 3) uint8 image; |u| or |v| > 1e9 is unknown (black).  has_max = 0
 * normalises by the largest known radius, else by max(max_flow, 1e-8).  The
 * arithmetic keeps numpy's dtype rules (the flow's dtype up to the wheel
 * position, float64 for the colour blend) */
int of_flow_to_color(of_ctx *ctx, const void *flow, int dtype, int H, int W, int has_max, double max_flow,
                     uint8_t *out_rgb);
/* scipy.ndimage.median_filter(size, mode='reflect') on each of `planes` planes */
int of_median_filter(of_ctx *ctx, const float *in, int H, int W, int planes, int size, float *out);

#ifdef __cplusplus
}
#endif
#endif /* OPTFLOW_H */
