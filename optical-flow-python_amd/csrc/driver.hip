// driver.hip — liboptflow.so: C ABI (include/optflow.h) + the on-device
// coarse-to-fine GNC x IRLS schedule.  Unity build: the kernel files and the
// host parts are included here so every kernel and its host launch live in
// one TU (one hipcc line, one gfx950 code object).
//
// The host never touches image data between kernels: one of_estimate_flow()
// call uploads a pair, runs preprocessing, pyramids, every warping
// iteration (warp, assembly, solve, update, occlusion, weighted median) on
// one HIP stream, and downloads the flow.  The only host<->device syncs
// inside a pair are the iterative solvers' convergence checks (one pinned
// 80-byte read per chunk of iterations, double-buffered so the GPU always
// has the next chunk queued) and Horn-Schunck's ||x|| < 1e-3 early exit.
//
// Kernel files, one family each, in dependency order like the host parts:
//   kernels_img.hip    colour, filters, resampling, pyramids, ROF
//   kernels_sample.hip the fp64 clamped bilinear sample of frames and flows that the files from kernels_interp.hip on share
//   kernels_warp.hip   warp of frame 2 and the data term's derivatives
//   kernels_assemble.hip system assembly, from derivative planes or fused with the warp; the fp64 assembly
//   kernels_flow.hip   flow update and occlusion, duv bookkeeping, forward-backward check, medians
//   kernels_interp.hip image warp, frame interpolation: splat, resolve, fill, render
//   kernels_wmf.hip    the weighted median
//   kernels_track.hip  point tracker: advance and seed steps
//   kernels_fuse.hip   temporal denoising: flow composition, frame fusion, the fusion's weights
//   kernels_noise.hip  noise-level estimation: the two estimators' keys, the exact radix selection of their median
//   kernels_upsample.hip reduced-resolution flow: the box reduction of a frame, the edge-aware upsampling of a flow
//   kernels_sr.hip     multi-frame super-resolution: the resampling along the flows, the back-projection step
//   kernels_inpaint.hip flow-guided video inpainting: mask growing and the pair weight, the fill along the flows
//   kernels_poisson.hip gradient-domain blending: the multilevel Poisson solver's steps, the blended fill's label planes and result
//   kernels_screen.hip blind temporal consistency: the screened multilevel solver's steps, its setup along the flow and result
//   kernels_mask.hip   mask propagation: the carry along the backward flow, the colour-guided vote, the mode filter
//   kernels_motion.hip global motion: the passes of the robust parametric fit, the affine warp
//   kernels_layers.hip layered motion segmentation (uses the fit's passes)
//   kernels_solve.hip  what the solvers share (partials, fixed-order sums, residual), norm and residual diagnostics
//   kernels_cg.hip     the fed CG: prologue, Jacobi iteration k_cg, check, residual replacement, finalize
//   kernels_cgs.hip    the 'backslash' surrogate iteration k_cgs
//   kernels_cg_wg.hip  a whole CG solve in one workgroup: k_cg_small, k_cg_reg
//   kernels_sor.hip    lexicographic SOR: per-sweep, pipelined and one-workgroup forms
//   kernels_gen.hip    CG on a general filter-bank operator (gen_*)
//
// Host parts, one concern each, in dependency order (a part uses only the
// parts above it, so none needs a forward declaration of a later one):
//   host_core.h     errors, arena, context, session base, profiling, launch(), shared checks, API_* macros
//   host_image.hip  image / flow-field helpers, taps, pyramids, ROF, derivatives, medians
//   host_solve.hip  CG and SOR dispatch, solve log, deferred statistics, gen_* solvers
//   host_flow.hip   assembly dispatch, token, per-level IRLS loops, schedule, estimate_*
//   host_upsample.hip reduced-resolution flow: reduction, upsampling, the scaled estimates, stage and one-call entries
//   host_session.hip what the frame-sequence sessions share: lookup and free, open and push prologues, delayed emission, the flow-scale switch
//   host_track.hip  point tracker: advance and seed steps, stage entries, the session
//   host_noise.hip  noise-level estimation: the pair and single-frame estimators, their stage entries
//   host_fuse.hip   temporal denoising: flow composition, frame fusion, stage entries, the rings of frames and pairs, the session and its automatic sigma
//   host_sr.hip     multi-frame super-resolution: the resampling and back-projection, the stage entry, the session
//   host_poisson.hip the multilevel Poisson solver: levels and windows, setup, the W-cycle schedule, the stage entry
//   host_inpaint.hip flow-guided video inpainting: mask growing, the fill, the blended fill, the stage entries, the session with its weighted pairs
//   host_screen.hip blind temporal consistency: the screened solve's levels and schedule, the step, the stage entries, the session
//   host_mask.hip   mask propagation: one step, the stage entry, the session
//   host_motion.hip global motion: the robust parametric fit, the affine warp, path smoothing, the stabiliser session
//   host_layers.hip layered motion segmentation: hypotheses, extraction, joint rounds, the stage entry
//   batch.hip       lanes, of_pairs_run[_host], pair pool, slot copies, RCCL gather
//   api.hip         context, options, profiling, single-pair and stage entries
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <immintrin.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kernels_img.hip"
#include "kernels_sample.hip"
#include "kernels_warp.hip"
#include "kernels_assemble.hip"
#include "kernels_flow.hip"
#include "kernels_interp.hip"
#include "kernels_wmf.hip"
#include "kernels_track.hip"
#include "kernels_fuse.hip"
#include "kernels_noise.hip"
#include "kernels_upsample.hip"
#include "kernels_sr.hip"
#include "kernels_inpaint.hip"
#include "kernels_poisson.hip"
#include "kernels_screen.hip"
#include "kernels_mask.hip"
#include "kernels_motion.hip"
#include "kernels_layers.hip"
#include "kernels_solve.hip"
#include "kernels_cg.hip"
#include "kernels_cgs.hip"
#include "kernels_cg_wg.hip"
#include "kernels_sor.hip"
#include "kernels_gen.hip"

#include "host_core.h"
#include "host_image.hip"
#include "host_solve.hip"
#include "host_flow.hip"
#include "host_upsample.hip"
#include "host_session.hip"
#include "host_track.hip"
#include "host_noise.hip"
#include "host_fuse.hip"
#include "host_sr.hip"
#include "host_poisson.hip"
#include "host_inpaint.hip"
#include "host_screen.hip"
#include "host_mask.hip"
#include "host_motion.hip"
#include "host_layers.hip"
#include "batch.hip"
#include "api.hip"
