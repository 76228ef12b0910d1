"""ctypes mirror of include/optflow.h (POD structs and enums only).

Kept free of any library loading so that both the product binding
(optical_flow._native) and the test oracle wrapper (oracle/oracle.py) can
share the exact struct layout.
"""
import ctypes as C

OF_ABI_VERSION = 3

OF_OK, OF_EINVAL, OF_EHIP, OF_ENOMEM, OF_ENOTSUP, OF_ERCCL = 0, -1, -2, -3, -4, -5

METHOD = {"hs": 0, "ba": 1, "classic_nl": 2, "alt_ba": 3}
INTERP = {"cubic": 0, "bi-cubic": 1, "bi-linear": 2}
SOLVER = {"backslash": 0, "pcg": 1, "sor": 2}
PENALTY = {
    "quadratic": 0, "lorentzian": 1, "charbonnier": 2, "generalized_charbonnier": 3,
    "geman_mcclure": 4, "huber": 5, "tukey": 6, "gaussian": 7, "tdist": 8, "tdist_unnorm": 9,
    "const": 100,
}
MAX_LEVELS = 32
OF_OPT_SOR_PIPELINE = 1  # of_set_option
OF_OPT_SOR_FALLBACKS = 2  # of_get_option (read-only counter)
OF_OPT_FUSED_WARP = 3  # of_set_option: warp + assembly in one kernel (default 1)
OF_OPT_DEVICE_BYTES = 4  # of_get_option (read-only): grow-only device bytes of the context and its lanes
OF_OPT_RCCL_NRANKS = 5  # of_get_option (read-only): ranks of the RCCL communicator (ncclCommCount; 0 = none)


class OfPenalty(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad_", C.c_int32), ("p0", C.c_double), ("p1", C.c_double)]


_INT_FIELDS = [
    "method", "solver", "interp", "texture", "fc", "auto_level", "pyramid_levels", "gnc_iters",
    "gnc_pyramid_levels", "max_iters", "max_warping_iters", "max_linear", "pcg_maxiter",
    "sor_max_iters", "limit_update", "median_filter_size", "mf_iter", "use_wmf", "area_hsz",
    "itersLO", "exact_maxiter", "display", "guide_mode", "pad_",
]
_DBL_FIELDS = [
    "lambda_", "lambda_q", "alpha", "pyramid_spacing", "gnc_pyramid_spacing", "pcg_rtol",
    "exact_rtol", "sor_omega", "sor_tol", "blend", "alp", "sigma_i", "sigmaD2", "sigmaS2",
    "lambda2", "lambda3",
]


MAX_FILTERS = 8
MAX_FDIM = 5


class OfFilterSet(C.Structure):
    """of_filter_set: a general spatial_filters list (general = 0: the
    default [[1, -1]], [[1], [-1]] pair)"""
    _fields_ = [("general", C.c_int32), ("n", C.c_int32),
                ("fh", C.c_int32 * MAX_FILTERS), ("fw", C.c_int32 * MAX_FILTERS),
                ("taps", (C.c_double * (MAX_FDIM * MAX_FDIM)) * MAX_FILTERS),
                ("rho_u", OfPenalty * MAX_FILTERS), ("rho_v", OfPenalty * MAX_FILTERS),
                ("qua_u", OfPenalty * MAX_FILTERS), ("qua_v", OfPenalty * MAX_FILTERS)]


class OfParams(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in _INT_FIELDS]
                + [(n, C.c_double) for n in _DBL_FIELDS]
                + [("deriv_filter", C.c_double * 5),
                   ("rho_data", OfPenalty), ("rho_spatial_u", OfPenalty * 2), ("rho_spatial_v", OfPenalty * 2),
                   ("qua_data", OfPenalty), ("qua_spatial_u", OfPenalty * 2), ("qua_spatial_v", OfPenalty * 2),
                   ("rho_couple", OfPenalty), ("filters", OfFilterSet)])


class OfStats(C.Structure):
    _fields_ = [
        ("n_levels", C.c_int32),
        ("level_h", C.c_int32 * MAX_LEVELS),
        ("level_w", C.c_int32 * MAX_LEVELS),
        ("level_stage", C.c_int32 * MAX_LEVELS),
        ("level_ms", C.c_double * MAX_LEVELS),
        ("solves", C.c_int32),
        ("solver_iters_total", C.c_int32),
        ("solver_iters_max", C.c_int32),
        ("solves_not_converged", C.c_int32),
        ("total_ms", C.c_double),
        ("preprocess_ms", C.c_double),
    ]

    def as_dict(self):
        n = self.n_levels
        return {
            "levels": [{"h": self.level_h[i], "w": self.level_w[i], "stage": self.level_stage[i],
                        "ms": self.level_ms[i]} for i in range(n)],
            "solves": self.solves, "solver_iters_total": self.solver_iters_total,
            "solver_iters_max": self.solver_iters_max,
            "solves_not_converged": self.solves_not_converged,
            "total_ms": self.total_ms, "preprocess_ms": self.preprocess_ms,
        }


# of_set_progress (include/optflow.h): events and flags
OF_EV_STAGE, OF_EV_LEVEL, OF_EV_ITER, OF_EV_STAGE_END = 0, 1, 2, 3
OF_PROGRESS_ITER, OF_PROGRESS_FLOW = 1, 2


class OfProgress(C.Structure):
    _fields_ = [("event", C.c_int32), ("stage", C.c_int32), ("level", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("iter", C.c_int32), ("lin", C.c_int32), ("pad_", C.c_int32),
                ("norm", C.c_double), ("elapsed_s", C.c_double), ("uv", C.POINTER(C.c_float))]


OfProgressFn = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(OfProgress))


class OfCgGeometry(C.Structure):
    _fields_ = [("grid_x", C.c_int32), ("grid_y", C.c_int32), ("rows", C.c_int32), ("bands", C.c_int32),
                ("blocks", C.c_int32), ("strip_cols", C.c_int32)]


class OfSolveRecord(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("solver", C.c_int32), ("iters", C.c_int32),
                ("done", C.c_int32), ("pad_", C.c_int32), ("true_rel", C.c_double), ("est_rel", C.c_double),
                ("true_rel_out", C.c_double)]

    def as_dict(self):
        return {"h": self.h, "w": self.w, "solver": self.solver, "iters": self.iters, "done": self.done,
                "true_rel": self.true_rel, "est_rel": self.est_rel, "true_rel_out": self.true_rel_out}


# point tracker (include/optflow.h, "Dense point trajectories"): track status bytes
OF_TRACK_ALIVE, OF_TRACK_OCCLUDED, OF_TRACK_LEFT_FRAME, OF_TRACK_MOTION_BOUNDARY = 0, 1, 2, 3
TRACK_MAX_STEP = 64
TRACK_MAX_TRACKS = 1 << 24


class OfTrackOpts(C.Structure):
    _fields_ = [("step", C.c_int32), ("max_tracks", C.c_int32), ("alpha1", C.c_double), ("alpha2", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("min_eig", C.c_double)]


# temporal denoising (include/optflow.h, "Motion-compensated temporal denoising")
FUSE_MAX_NEIGHBOURS = 8
FUSE_MAX_CHANNELS = 4
FUSE_MAX_PATCH = 3
FUSE_MAX_RADIUS = 2


class OfFuseOpts(C.Structure):
    _fields_ = [("radius", C.c_int32), ("patch", C.c_int32), ("sigma", C.c_double), ("strength", C.c_double),
                ("alpha1", C.c_double), ("alpha2", C.c_double)]


# noise-level estimation (include/optflow.h, "Noise-level estimation")
NOISE_MAX_CHANNELS = 4


class OfNoiseEstimate(C.Structure):
    _fields_ = [("sigma", C.c_double), ("sigma_c", C.c_double * 4), ("n", C.c_int64)]


# global motion and stabilisation (include/optflow.h, "Global motion estimation")
MOTION_MODEL = {"translation": 0, "similarity": 1, "affine": 2}
MOTION_MAX_ITERS = 64
STAB_MAX_RADIUS = 30


class OfMotionOpts(C.Structure):
    _fields_ = [("model", C.c_int32), ("iters", C.c_int32), ("kappa", C.c_double), ("decay", C.c_double),
                ("c_min", C.c_double)]


class OfMotionFit(C.Structure):
    _fields_ = [("theta", C.c_double * 6), ("matrix", C.c_double * 6), ("cutoff", C.c_double),
                ("support", C.c_double), ("rms", C.c_double), ("passes", C.c_int32), ("degenerate", C.c_int32)]


class OfStabOpts(C.Structure):
    _fields_ = [("fit", OfMotionOpts), ("radius", C.c_int32), ("pad_", C.c_int32), ("sigma_t", C.c_double),
                ("alpha1", C.c_double), ("alpha2", C.c_double)]


# layered motion segmentation (include/optflow.h, "Layered motion segmentation")
OF_LAYER_NONE = 255
LAYERS_MAX, LAYERS_MAX_GRID, LAYERS_MAX_PASSES, LAYERS_MAX_ROUNDS, LAYERS_MAX_SMOOTH = 8, 16, 16, 16, 3


class OfLayersOpts(C.Structure):
    _fields_ = [("model", C.c_int32), ("max_layers", C.c_int32), ("grid", C.c_int32), ("passes", C.c_int32),
                ("rounds", C.c_int32), ("smooth", C.c_int32), ("cutoff", C.c_double), ("min_support", C.c_double)]


class OfMotionLayer(C.Structure):
    _fields_ = [("theta", C.c_double * 6), ("matrix", C.c_double * 6), ("support", C.c_double), ("rms", C.c_double),
                ("pixels", C.c_int64), ("degenerate", C.c_int32), ("pad_", C.c_int32)]


# reduced-resolution flow (include/optflow.h, "Reduced-resolution flow with edge-aware upsampling")
UPSAMPLE_MIN_SCALE, UPSAMPLE_MAX_SCALE = 2, 4
UPSAMPLE_MAX_CHANNELS = 4
OF_SESSION_TRACKS, OF_SESSION_DENOISE, OF_SESSION_STAB = 1, 2, 4  # of_session_set_flow_scale


class OfUpsampleOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("pad_", C.c_int32), ("range", C.c_double)]


# multi-frame super-resolution (include/optflow.h, "Multi-frame super-resolution along the flow")
SR_MIN_FACTOR, SR_MAX_FACTOR = 2, 4
SR_MAX_NEIGHBOURS = 8
SR_MIN_REACH, SR_MAX_REACH = 0.75, 1.5


class OfSrOpts(C.Structure):
    _fields_ = [("factor", C.c_int32), ("radius", C.c_int32), ("patch", C.c_int32), ("pad_", C.c_int32),
                ("sigma", C.c_double), ("strength", C.c_double), ("reach", C.c_double), ("back", C.c_double),
                ("alpha1", C.c_double), ("alpha2", C.c_double)]


# flow-guided video inpainting (include/optflow.h, "Flow-guided video inpainting"): status bytes and ranges
OF_INPAINT_KEPT, OF_INPAINT_FILLED, OF_INPAINT_UNFILLED = 0, 1, 2
INPAINT_MAX_RADIUS, INPAINT_MAX_GROW, INPAINT_MAX_MARGIN = 16, 8, 16
INPAINT_MAX_CHANNELS = 4
MASK_GROW_MAX = 24


class OfInpaintOpts(C.Structure):
    _fields_ = [("radius", C.c_int32), ("grow", C.c_int32), ("margin", C.c_int32), ("pad_", C.c_int32)]


# gradient-domain blending (include/optflow.h, "Gradient-domain blending"): the status byte, labels and ranges
OF_INPAINT_SPATIAL = 3
OF_PSN_FIXED, OF_PSN_UNKNOWN, OF_PSN_EXCLUDED = 0, 1, 2
BLEND_MAX_CYCLES, BLEND_MAX_SWEEPS, BLEND_MAX_COARSE_SWEEPS = 64, 2, 64
BLEND_MAX_CHANNELS = 4


class OfBlendOpts(C.Structure):
    _fields_ = [("cycles", C.c_int32), ("sweeps", C.c_int32), ("coarse_sweeps", C.c_int32), ("pad_", C.c_int32)]


# mask propagation (include/optflow.h, "Mask propagation"): status bytes and ranges
OF_MASK_CARRIED, OF_MASK_VOTED, OF_MASK_UNKNOWN, OF_MASK_GIVEN = 0, 1, 2, 3
MASK_MAX_VOTE_RADIUS, MASK_MAX_SMOOTH = 12, 2
MASK_MAX_CHANNELS = 4


class OfMaskOpts(C.Structure):
    _fields_ = [("vote_radius", C.c_int32), ("smooth", C.c_int32), ("range", C.c_double), ("alpha1", C.c_double),
                ("alpha2", C.c_double)]


# blind temporal consistency (include/optflow.h, "Blind temporal consistency")
CONSIST_CYCLES = 5
CONSIST_MAX_CHANNELS = 4


class OfConsistOpts(C.Structure):
    _fields_ = [("fuse", OfFuseOpts), ("solve", OfBlendOpts), ("lambda_", C.c_double)]


def penalty(kind, p0=1.0, p1=0.0):
    return OfPenalty(PENALTY[kind], 0, float(p0), float(p1))


def penalty_from_robust(rf):
    """OfPenalty from an optical_flow.robust.RobustFunction (robust_function.py:47-83)."""
    p = list(rf.param) + [0.0]
    return OfPenalty(PENALTY[rf.method], 0, float(p[0]), float(p[1]))
