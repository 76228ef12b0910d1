"""What the package's modules share around the C ABI: the argument validators
(ValueError before the library or a context is touched), the method ->
of_params step, and the base classes of the frame-sequence sessions
(PointTracker, TemporalDenoiser, Stabilizer, SuperResolver, VideoInpainter)."""
import ctypes as C

import numpy as np

from optical_flow import _abi
from optical_flow import _native as nat
from optical_flow.methods.config import load_of_method


def method_params(method, params):
    """The configured method object of `method` with the `params` overrides,
    and its of_params."""
    ope = load_of_method(method)
    if params is not None:
        ope.parse_input_parameter(params)
    return ope, ope.to_params()


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def _number(name, v, positive):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
            or (v <= 0 if positive else v < 0):
        raise ValueError(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
    return float(v)


def _flow_scale(scale, upsample_range, range_name="upsample_range"):
    """The `scale` / `upsample_range` keywords as an of_upsample_opts, or None
    for scale 1 (the full-resolution estimate, today's C calls)."""
    scale = _int_in("scale", scale, 1, _abi.UPSAMPLE_MAX_SCALE)
    rng = _number(range_name, upsample_range, True)
    return None if scale == 1 else _abi.OfUpsampleOpts(scale, 0, rng)


def _frame_size(H, W):
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise ValueError(f"frames must be non-empty and below 2^31 pixels, got {H} x {W}")


def _frame_shape(shape):
    """A session's frame shape as (shape, H, W, channels): (H, W) or (H, W, 3)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise ValueError(f"shape must be (H, W) or (H, W, 3), got {shape}")
    H, W = shape[:2]
    _frame_size(H, W)
    return shape, H, W, 3 if len(shape) == 3 else 1


def _clip(frames):
    """A clip as a list of arrays: at least one frame, all of one shape."""
    frames = [np.asarray(f) for f in frames]
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("frames must be a non-empty sequence of frames of one shape")
    return frames


def _flow(name, f, shape=None):
    f = np.asarray(f)
    if f.ndim != 3 or f.shape[2] != 2 or f.dtype.kind not in "fiu" or (shape is not None and f.shape[:2] != shape):
        want = "(H, W, 2)" if shape is None else f"{shape + (2,)}"
        raise ValueError(f"{name} must be a {want} array of numbers, got {f.dtype} {f.shape}")
    return f


def _state(name, s, H, W):
    """A forward-backward mask as contiguous (H, W) uint8, or None."""
    if s is None:
        return None
    s = np.asarray(s)
    if s.shape != (H, W) or s.dtype.kind not in "iub" or (s.size and (s.min() < 0 or s.max() > 255)):
        raise ValueError(f"{name} must be ({H}, {W}) integers in 0..255, got {s.dtype} {s.shape}")
    return np.ascontiguousarray(s, dtype=np.uint8)


def _planar32(f):
    with np.errstate(over='ignore'):
        return nat.planar(f)


class Closing:
    """close() on leaving a `with` block and, quietly, at garbage collection."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Session(Closing):
    """A frame-sequence session of a context: of_<kind>_open at construction,
    of_<kind>_close in close().  Subclasses name the C entries' prefix
    (_PREFIX), their OF_SESSION_* bit (_KIND) and themselves in the "is closed"
    error (_NAME)."""
    _PREFIX = _NAME = _KIND = None

    def __init__(self, shape, method, params, make_opts, context, scale=1, upsample_range=20.0):
        """`make_opts(H, W)` validates the session's own arguments into its
        options struct; everything is validated before the library or a
        context is touched.  `scale` > 1 estimates every pair at reduced
        resolution (of_session_set_flow_scale right after the open); 1 makes
        no such call."""
        self._ctx = None
        self.shape, self.H, self.W, self.channels = _frame_shape(shape)
        self._opts = make_opts(self.H, self.W)
        up = _flow_scale(scale, upsample_range)
        P = method_params(method, params)[1]
        self.frames = 0
        ctx = nat.context() if context is None else context
        ctx.check(self._open(ctx, P))
        self._ctx = ctx
        if up is not None:
            try:
                ctx.check(ctx.lib.of_session_set_flow_scale(ctx.handle, self._KIND, C.byref(up)))
            except Exception:
                self.close()
                raise

    def _open(self, ctx, P):
        """The return code of the session's open entry on `ctx`."""
        return getattr(ctx.lib, self._PREFIX + "open")(ctx.handle, C.byref(P), self.H, self.W, self.channels,
                                                       C.byref(self._opts))

    def _live(self):
        if self._ctx is None:
            raise ValueError(f"the {self._NAME} is closed")
        return self._ctx

    def _call(self, entry, *args):
        """of_<kind>_<entry>(handle, *args) on the session's context, checked."""
        ctx = self._live()
        ctx.check(getattr(ctx.lib, self._PREFIX + entry)(ctx.handle, *args))

    def _push(self, frame, *args):
        """of_<kind>_push of `frame`, checked against the session's shape, as
        contiguous float32."""
        self._live()
        f = np.asarray(frame)
        if f.shape != self.shape or f.dtype.kind not in "fiu":
            raise ValueError(f"frames must be {self.shape} arrays of numbers, got {f.dtype} {f.shape}")
        self._call("push", nat.ptr(nat.f32(np.asarray(f, dtype=float))), *args)
        self.frames += 1

    def close(self):
        if self._ctx is not None:
            ctx, self._ctx = self._ctx, None
            if ctx.handle:  # a destroyed context has closed its sessions
                ctx.check(getattr(ctx.lib, self._PREFIX + "close")(ctx.handle))


class DelayedSession(Session):
    """A session whose push returns frame t once frame t + radius is in: None,
    or (index, frame).  Subclasses give _flush_step(), one of_<kind>_flush
    call's result in the same form."""

    def flush(self):
        """Yields (index, frame) for the frames still pending at the end of
        the clip, each processed with the neighbours that exist.  No push
        after it."""
        while True:
            r = self._flush_step()
            if r is None:
                return
            yield r

    @classmethod
    def run_clip(cls, frames, last, *args):
        """`frames` through a session cls(shape, *args): the frames it returns,
        (T,) + their shape, float64, and the session's attribute `last` after each,
        stacked, both by frame index; for a tuple of attribute names, a tuple
        of such stacks."""
        frames = _clip(frames)
        out = None  # (T,) + the shape of the frames the session returns, which need not be the input's
        names = (last,) if isinstance(last, str) else tuple(last)
        extra = [[None] * len(frames) for _ in names]
        with cls(frames[0].shape, *args) as s:
            def take(r):
                nonlocal out
                if r is not None:
                    if out is None:
                        out = np.empty((len(frames),) + r[1].shape, dtype=np.float64)
                    out[r[0]] = r[1]
                    for e, name in zip(extra, names):
                        e[r[0]] = getattr(s, name)
            for f in frames:
                take(s.push(f))
            for r in s.flush():
                take(r)
        stacks = tuple(np.stack(e) for e in extra)
        return out, (stacks[0] if isinstance(last, str) else stacks)
