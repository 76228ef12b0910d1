"""MI355X-native variational optical flow.

Drop-in for jordanshivers/optical-flow-python: same estimate_flow() /
compute_flow() API and method registry; the coarse-to-fine IRLS hot path runs
as hand-written HIP kernels for gfx950 in liboptflow.so (include/optflow.h).
"""
from optical_flow.interface import (estimate_flow, estimate_flow_batch, PairStream, estimate_flow_bidirectional,
                                    BidirectionalFlow, interpolate_frames, INTERP_BLEND, INTERP_FRAME1_ONLY,
                                    INTERP_FRAME2_ONLY, INTERP_NEITHER, INTERP_FILLED)
from optical_flow.tracking import (advance_points, seed_points, PointTracker, track_points, Trajectories,
                                   TRACK_ALIVE, TRACK_OCCLUDED, TRACK_LEFT_FRAME, TRACK_MOTION_BOUNDARY)
from optical_flow.temporal import compose_flows, fuse_frames, fuse_weights, TemporalDenoiser, denoise_frames
from optical_flow.superres import super_resolve, SuperResolver, super_resolve_frames
from optical_flow.inpaint import (grow_mask, pair_weight, propagate_fill, VideoInpainter, inpaint_frames,
                                  INPAINT_KEPT, INPAINT_FILLED, INPAINT_UNFILLED, poisson_fill, blend_fill,
                                  INPAINT_SPATIAL)
from optical_flow.masks import (advance_mask, MaskPropagator, propagate_masks, MASK_CARRIED, MASK_VOTED, MASK_UNKNOWN,
                                MASK_GIVEN)
from optical_flow.consistency import screened_poisson, consistency_step, TemporalConsistency, consistent_frames
from optical_flow.noise import estimate_noise, NoiseEstimate
from optical_flow.motion import (fit_motion, warp_affine, Stabilizer, stabilize_frames, MotionFit, segment_motion,
                                 MotionLayers, MotionLayer, LAYER_NONE)
from optical_flow.upsample import reduce_frame, upsample_flow
from optical_flow.utils.warping import warp_image
from optical_flow.utils.occlusion import forward_backward_check, FB_CONSISTENT, FB_OCCLUDED, FB_OUT_OF_FRAME
from optical_flow.io.flo_io import read_flo, write_flo
from optical_flow.viz.flow_color import flow_to_color
from optical_flow.viz.plot_flow import plot_flow
from optical_flow.evaluation.metrics import flow_angular_error
from optical_flow.methods.config import load_of_method

__all__ = ['estimate_flow', 'estimate_flow_batch', 'PairStream', 'read_flo', 'write_flo', 'flow_to_color', 'plot_flow', 'flow_angular_error',
           'load_of_method', 'estimate_flow_bidirectional', 'BidirectionalFlow', 'forward_backward_check',
           'FB_CONSISTENT', 'FB_OCCLUDED', 'FB_OUT_OF_FRAME', 'interpolate_frames', 'warp_image', 'INTERP_BLEND',
           'INTERP_FRAME1_ONLY', 'INTERP_FRAME2_ONLY', 'INTERP_NEITHER', 'INTERP_FILLED', 'advance_points',
           'seed_points', 'PointTracker', 'track_points', 'Trajectories', 'TRACK_ALIVE', 'TRACK_OCCLUDED',
           'TRACK_LEFT_FRAME', 'TRACK_MOTION_BOUNDARY', 'compose_flows', 'fuse_frames', 'TemporalDenoiser',
           'denoise_frames', 'fit_motion', 'warp_affine', 'Stabilizer', 'stabilize_frames', 'MotionFit',
           'segment_motion', 'MotionLayers', 'MotionLayer', 'LAYER_NONE', 'estimate_noise', 'NoiseEstimate',
           'reduce_frame', 'upsample_flow', 'fuse_weights', 'super_resolve', 'SuperResolver', 'super_resolve_frames',
           'grow_mask', 'pair_weight', 'propagate_fill', 'VideoInpainter', 'inpaint_frames', 'INPAINT_KEPT',
           'INPAINT_FILLED', 'INPAINT_UNFILLED', 'advance_mask', 'MaskPropagator', 'propagate_masks', 'MASK_CARRIED',
           'MASK_VOTED', 'MASK_UNKNOWN', 'MASK_GIVEN', 'poisson_fill', 'blend_fill', 'INPAINT_SPATIAL', 'screened_poisson',
           'consistency_step', 'TemporalConsistency', 'consistent_frames']
