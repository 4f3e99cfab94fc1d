"""ctypes view of include/vslam_hip.h.

`CApi(path, prefix)` binds one shared library that exports the C ABI with the given symbol
prefix.  The product binds `libvslam_hip.so` with prefix ``vslam_`` (see ``hip.py``); the test
suite binds the CPU oracle with prefix ``orc_`` through ``tests/_oracle.py``.  Nothing in this
package loads the oracle.
"""
import ctypes as C
import numpy as np

from . import color as _color

MAX_REGIONS = 16

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_STATE = 0, -1, -2, -3, -4, -5
LOCALIZING, TRACKING = 0, 1
MOTION_CONSTANT_VELOCITY, MOTION_NONE, MOTION_CAMERA_ODOMETRY = 0, 1, 2      # enum vslam_motion_model


class Config(C.Structure):
    """struct vslam_config (include/vslam_hip.h)."""
    _fields_ = [
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("K", C.c_double * 9), ("baseline_h", C.c_double * 3),
        ("det_rows", C.c_int32), ("det_cols", C.c_int32),
        ("detector_threshold_minimum", C.c_int32), ("detector_threshold_maximum", C.c_int32),
        ("detector_threshold_maximum_change", C.c_double),
        ("target_number_of_keypoints_tolerance", C.c_double),
        ("bin_size_pixels", C.c_int32), ("enable_keypoint_binning", C.c_int32),
        ("minimum_projection_tracking_distance_pixels", C.c_int32),
        ("maximum_projection_tracking_distance_pixels", C.c_int32),
        ("minimum_descriptor_distance_tracking", C.c_double),
        ("maximum_descriptor_distance_tracking", C.c_double),
        ("maximum_reliable_depth_meters", C.c_double),
        ("maximum_depth_meters", C.c_double),
        ("minimum_depth_meters", C.c_double),
        ("maximum_matching_distance_triangulation", C.c_double),
        ("minimum_disparity_pixels", C.c_double),
        ("maximum_epipolar_search_offset_pixels", C.c_int32),
        ("minimum_track_length_for_landmark_creation", C.c_int32),
        ("minimum_number_of_landmarks_to_track", C.c_int32),
        ("tunnel_vision_ratio", C.c_double), ("good_tracking_ratio", C.c_double),
        ("enable_landmark_recovery", C.c_int32),
        ("minimum_delta_angular_for_movement", C.c_double),
        ("minimum_delta_translational_for_movement", C.c_double),
        ("aligner_error_delta_for_convergence", C.c_double),
        ("aligner_maximum_error_kernel", C.c_double),
        ("aligner_damping", C.c_double),
        ("aligner_maximum_number_of_iterations", C.c_int32),
        ("aligner_minimum_number_of_inliers", C.c_int32),
        ("landmark_maximum_error_squared_meters", C.c_double),
        ("landmark_maximum_number_of_iterations", C.c_int32),
        ("max_keypoints", C.c_int32), ("max_points", C.c_int32), ("max_history_frames", C.c_int32),
        ("descriptor_type", C.c_int32),
    ]

    def copy(self):
        c = Config()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(Config))
        return c


class FrameInfo(C.Structure):
    """struct vslam_frame_info (include/vslam_hip.h)."""
    _fields_ = [
        ("frame_index", C.c_int32), ("status", C.c_int32), ("status_at_start", C.c_int32),
        ("n_keypoints_left", C.c_int32), ("n_keypoints_right", C.c_int32),
        ("n_detected_left", C.c_int32), ("n_detected_right", C.c_int32),
        ("thresholds", C.c_int32 * MAX_REGIONS),
        ("track_attempts", C.c_int32), ("n_tracked", C.c_int32), ("n_lost", C.c_int32),
        ("n_tracked_landmarks", C.c_int32), ("aligner_ran", C.c_int32),
        ("aligner_iterations", C.c_int32), ("aligner_converged", C.c_int32),
        ("n_inliers", C.c_int32), ("n_outliers", C.c_int32), ("total_error", C.c_double),
        ("n_after_prune", C.c_int32), ("n_recovered", C.c_int32),
        ("n_active_landmarks", C.c_int32), ("n_new_stereo", C.c_int32), ("n_points", C.c_int32),
        ("track_broken", C.c_int32), ("fallback", C.c_int32), ("window_pixels", C.c_int32),
        ("error_flags", C.c_int32), ("tau_track", C.c_double), ("tau_triangulation", C.c_double),
        ("camera_left_to_world", C.c_double * 12), ("previous_to_current", C.c_double * 12),
    ]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class KeypointsView(C.Structure):
    """struct vslam_keypoints_view (stage views: pointers into the context's pinned report buffer, valid until the next view call)."""
    _fields_ = [("n", C.c_int32 * 2), ("xy", C.POINTER(C.c_int16) * 2), ("score", C.POINTER(C.c_uint8) * 2), ("desc", C.POINTER(C.c_uint8) * 2)]


class TrackView(C.Structure):
    _fields_ = [("n_tracked", C.c_int32), ("n_lost", C.c_int32), ("n_tracked_landmarks", C.c_int32),
                ("tracked4", C.POINTER(C.c_int32)), ("lost", C.POINTER(C.c_int32))]


class AlignerView(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_inliers", C.c_int32), ("n_outliers", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("total_error", C.c_double), ("chi", C.POINTER(C.c_double)), ("inlier", C.POINTER(C.c_uint8)), ("T", C.c_double * 12), ("H", C.c_double * 36)]


class PointsView(C.Structure):
    _fields_ = [("n", C.c_int32), ("first_full", C.c_int32), ("kp", C.POINTER(C.c_int16)), ("meta", C.POINTER(C.c_int32)), ("cam", C.POINTER(C.c_double)),
                ("desc", C.POINTER(C.c_uint8)), ("info", FrameInfo), ("seconds_tracking", C.c_double), ("seconds_pose_optimization", C.c_double),
                ("seconds_point_recovery", C.c_double), ("seconds_landmark_optimization", C.c_double), ("seconds_point_triangulation", C.c_double)]


class DepthParams(C.Structure):
    """struct vslam_depth_params (include/vslam_hip.h)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("K_left", C.c_double * 9), ("K_left_inverse", C.c_double * 9),
                ("K_right_inverse", C.c_double * 9), ("right_to_left", C.c_double * 12),
                ("depth_scale_factor_intensity_to_meters", C.c_double), ("minimum_depth_meters", C.c_double),
                ("maximum_depth_meters", C.c_double), ("enable_point_triangulation", C.c_int32),
                ("enable_keypoint_binning", C.c_int32), ("bin_size_pixels", C.c_int32), ("descriptor_type", C.c_int32),
                ("detector_type", C.c_int32)]

    @staticmethod
    def make(rows, cols, K_left, K_left_inverse, K_right_inverse, right_to_left, scale=1e-3, min_depth=0.1, max_depth=10.0,
             triangulation=1, binning=1, bin_px=6, descriptor=0, detector=0):
        p = DepthParams()
        p.rows, p.cols = int(rows), int(cols)
        for name, a in (("K_left", K_left), ("K_left_inverse", K_left_inverse), ("K_right_inverse", K_right_inverse), ("right_to_left", right_to_left)):
            flat = np.ascontiguousarray(a, np.float64).ravel()
            getattr(p, name)[:] = list(flat)
        p.depth_scale_factor_intensity_to_meters = scale
        p.minimum_depth_meters, p.maximum_depth_meters = min_depth, max_depth
        p.enable_point_triangulation, p.enable_keypoint_binning, p.bin_size_pixels = int(triangulation), int(binning), int(bin_px)
        p.descriptor_type = int(descriptor)
        p.detector_type = int(detector)      # 0 FAST, 1 ORB (OrbDetector)
        return p


class VslamError(RuntimeError):
    """Raised for a negative vslam_status (the reference throws std::runtime_error)."""

    def __init__(self, code, text):
        super().__init__("vslam status %d: %s" % (code, text))
        self.code = code


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


CLAHE_MAX_TILES = 32        # VSLAM_CLAHE_MAX_TILES


def _clahe_luts(get, tiles, sides):
    """The tables behind a get_clahe_luts entry as uint8 [sides, tilesY, tilesX, 256].  The entry writes as many tables as the switch in
    the LIBRARY holds tiles, so it gets a buffer for the largest grid whatever this object believes the grid to be."""
    buf = np.zeros(sides * CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256, np.uint8)
    get(buf)
    if tiles is None:
        raise ValueError("clahe_luts: the tile grid is unknown, CLAHE was not switched on through this object's set_clahe")
    return buf[:sides * tiles[0] * tiles[1] * 256].reshape(sides, tiles[1], tiles[0], 256).copy()


class CApi(object):
    """One loaded library + one context (n_streams independent sequences)."""

    def __init__(self, lib_path, prefix):
        self.lib = C.CDLL(lib_path)
        self.prefix = prefix
        self.ctx = None

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    # -- lifetime ---------------------------------------------------------------------------
    def default_config(self, which="kitti"):
        cfg = Config()
        self.fn("default_config_" + which)(C.byref(cfg))
        return cfg

    def create(self, cfg, device=0, n_streams=1):
        self.destroy()
        ctx = C.c_void_p()
        f = self.fn("create")
        f.restype = C.c_int
        rc = f(C.byref(cfg), C.c_int(device), C.c_int(n_streams), C.byref(ctx))
        if rc != OK:
            raise VslamError(rc, self.last_error(None))
        self.ctx = ctx
        self.cfg = cfg.copy()
        self.n_streams = n_streams
        self.rect = None
        self._ds_state = None
        self.color = 0
        return self

    def destroy(self):
        if self.ctx is not None:
            self.fn("destroy")(self.ctx)
            self.ctx = None

    def last_error(self, ctx):
        if not self.has("last_error"):
            return ""
        f = self.fn("last_error")
        f.restype = C.c_char_p
        s = f(ctx)
        return s.decode() if s else ""

    def check(self, rc):
        if rc != OK:
            raise VslamError(rc, self.last_error(self.ctx))

    def reset(self):
        self.check(self.fn("reset")(self.ctx))

    def set_stream_active(self, stream, active=True):
        self.check(self.fn("set_stream_active")(self.ctx, C.c_int(stream), C.c_int(1 if active else 0)))

    def reset_stream(self, stream):
        self.check(self.fn("reset_stream")(self.ctx, C.c_int(stream)))

    def reset_streams(self, streams):
        ids = np.ascontiguousarray(streams, np.int32)
        if len(ids):
            self.check(self.fn("reset_streams")(self.ctx, C.c_int32(len(ids)), _p(ids, C.c_int32)))

    # -- whole frame --------------------------------------------------------------------------
    def process_host(self, left, right):
        """left/right: uint8 arrays [n_streams, rows, stride] (C-contiguous); while a colour format is set (set_color_input):
        [n_streams, rows, cols, channels]."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        ch = _color.channels(getattr(self, "color", 0))
        if ch > 1:
            if left.ndim == 3:
                left, right = left[None], right[None]
            assert left.ndim == 4 and left.shape[3] == ch, (left.shape, ch)
            n, rows, cols = left.shape[:3]
            want = self._incoming_size()
            assert left.shape == right.shape and n == self.n_streams and (rows, cols) == want, (left.shape, right.shape, want)
            self.check(self.fn("process_host")(self.ctx, _p(left, C.c_uint8), _p(right, C.c_uint8), C.c_int32(cols * ch), C.c_size_t(rows * cols * ch)))
            return
        if left.ndim == 2:
            left, right = left[None], right[None]
        assert left.shape == right.shape and left.shape[0] == self.n_streams
        want = self._incoming_size()                      # downscaling context: full images; rectifying context: raw images
        assert left.shape[1] == want[0] and left.shape[2] >= want[1], (left.shape, want)
        stride = left.shape[2]
        self.check(self.fn("process_host")(self.ctx, _p(left, C.c_uint8), _p(right, C.c_uint8),
                                           C.c_int32(stride), C.c_size_t(left.shape[1] * stride)))

    def process_device(self, left_ptr, right_ptr, row_stride, image_stride):
        self.check(self.fn("process_device")(self.ctx, C.c_void_p(left_ptr), C.c_void_p(right_ptr),
                                             C.c_int32(row_stride), C.c_size_t(image_stride)))

    def synchronize(self):
        self.check(self.fn("synchronize")(self.ctx))

    def _incoming_size(self):
        """(rows, cols) of the frames the frame entries take: the full size while downscaling, else the raw size of a rectifying context,
        else the context's own."""
        ds = getattr(self, "_ds_state", None)
        if ds is not None:
            return ds[1], ds[2]
        rect = getattr(self, "rect", None)
        return (int(rect.raw_rows), int(rect.raw_cols)) if rect is not None else (int(self.cfg.rows), int(self.cfg.cols))

    # -- integer-factor reduction of the incoming frames (vslam_set_downscale; definition: downscale.py) -----------------------
    def set_downscale(self, factor, full_rows=0, full_cols=0):
        """factor 2 .. 4: the frame entries take images of full_rows x full_cols (colour images too) and reduce them on the device ahead
        of rectification; full // factor must be the raw size of a rectifying context, else the context's own.  factor 1: off."""
        self.check(self.fn("set_downscale")(self.ctx, C.c_int32(int(factor)), C.c_int32(int(full_rows)), C.c_int32(int(full_cols))))
        self._ds_state = None if int(factor) == 1 else (int(factor), int(full_rows), int(full_cols))

    def downscale(self):
        """(factor, full_rows, full_cols) in force; (1, 0, 0) while off."""
        f, r, c_ = C.c_int32(), C.c_int32(), C.c_int32()
        self.check(self.fn("get_downscale")(self.ctx, C.byref(f), C.byref(r), C.byref(c_)))
        return f.value, r.value, c_.value

    def downscaled_images(self, stream=0):
        """The reduced pair the last submitted frame of `stream` was downscaled to (full // factor)."""
        f, r, c_ = self.downscale()
        rows, cols = (r // f, c_ // f) if f > 1 else (int(self.cfg.rows), int(self.cfg.cols))
        L = np.zeros((rows, cols), np.uint8)
        R = np.zeros((rows, cols), np.uint8)
        self.check(self.fn("get_downscaled_images")(self.ctx, C.c_int(stream), _p(L, C.c_uint8), _p(R, C.c_uint8)))
        return L, R

    # -- smoothing of the grey pair ahead of the equalisation slot (vslam_set_smoothing; definition: smooth.py) ------------------
    def set_smoothing(self, mode, ksize=0):
        """mode smooth.GAUSSIAN (ksize 3 / 5 / 7) or smooth.MEDIAN (3 / 5); smooth.OFF frees the stage's buffers."""
        self.check(self.fn("set_smoothing")(self.ctx, C.c_int(int(mode)), C.c_int32(int(ksize))))

    def smoothing(self):
        """(mode, ksize) in force; (0, 0) while off."""
        m, k = C.c_int(), C.c_int32()
        self.check(self.fn("get_smoothing")(self.ctx, C.byref(m), C.byref(k)))
        return m.value, k.value

    def smoothed_images(self, stream=0):
        """The smoothed pair of the last submitted frame of `stream`, ahead of the equalisation."""
        L = np.zeros((int(self.cfg.rows), int(self.cfg.cols)), np.uint8)
        R = np.zeros_like(L)
        self.check(self.fn("get_smoothed_images")(self.ctx, C.c_int(stream), _p(L, C.c_uint8), _p(R, C.c_uint8)))
        return L, R

    # -- rectification of raw pairs (vslam_set_rectification) ---------------------------------------------------------
    def set_rectification(self, rect):
        """rect: rectify.Rectification (its maps at the context's rows x cols), or None to switch rectification off."""
        if rect is None:
            self.check(self.fn("set_rectification")(self.ctx, C.c_int32(0), C.c_int32(0), None, None, None, None))
            self.rect = None
            return
        if (rect.rows, rect.cols) != (self.cfg.rows, self.cfg.cols):
            raise ValueError("set_rectification: maps are %dx%d, the context is %dx%d" % (rect.rows, rect.cols, self.cfg.rows, self.cfg.cols))
        xl, al = np.ascontiguousarray(rect.map_xy_left, np.int16), np.ascontiguousarray(rect.map_a_left, np.uint16)
        xr, ar = np.ascontiguousarray(rect.map_xy_right, np.int16), np.ascontiguousarray(rect.map_a_right, np.uint16)
        self.check(self.fn("set_rectification")(self.ctx, C.c_int32(rect.raw_rows), C.c_int32(rect.raw_cols), _p(xl, C.c_int16), _p(al, C.c_uint16),
                                                _p(xr, C.c_int16), _p(ar, C.c_uint16)))
        self.rect = rect

    def set_rectification_mask(self, on=True, margin=0):
        """The rectification maps' validity (rectify.validity, eroded by margin) as part of the context-wide keep-mask of both sides."""
        self.check(self.fn("set_rectification_mask")(self.ctx, C.c_int(1 if on else 0), C.c_int32(int(margin))))

    def rectification_mask(self):
        """(on, margin) in force."""
        on, m = C.c_int(), C.c_int32()
        self.check(self.fn("get_rectification_mask")(self.ctx, C.byref(on), C.byref(m)))
        return bool(on.value), m.value

    def map_validity_mask(self, map_xy, map_a, raw_rows, raw_cols, margin=0):
        """vslam_map_validity_mask: the eroded packed validity words of one remap map -> uint64 [rows, (cols + 63) // 64]."""
        mxy = np.ascontiguousarray(map_xy, np.int16)
        ma = np.ascontiguousarray(map_a, np.uint16)
        assert mxy.shape[:2] == ma.shape and mxy.shape[2] == 2
        rows, cols = ma.shape
        w = np.zeros((rows, (cols + 63) // 64), np.uint64)
        self.check(self.fn("map_validity_mask")(*self._ctx_args(), _p(mxy, C.c_int16), _p(ma, C.c_uint16), C.c_int32(rows), C.c_int32(cols),
                                                C.c_int32(int(raw_rows)), C.c_int32(int(raw_cols)), C.c_int32(int(margin)), _p(w, C.c_uint64)))
        return w

    def rectified_images(self, stream=0):
        """The rectified pair the last submitted frame of `stream` was processed on."""
        rows, cols = int(self.cfg.rows), int(self.cfg.cols)
        L = np.zeros((rows, cols), np.uint8)
        R = np.zeros((rows, cols), np.uint8)
        self.check(self.fn("get_rectified_images")(self.ctx, C.c_int(stream), _p(L, C.c_uint8), _p(R, C.c_uint8)))
        return L, R

    # -- histogram equalisation of the input pair (vslam_set_equalization) ------------------------------------------------
    def set_equalization(self, on=True):
        self.check(self.fn("set_equalization")(self.ctx, C.c_int(1 if on else 0)))

    def equalized_images(self, stream=0):
        """The equalised pair the last submitted frame of `stream` was processed on."""
        rows, cols = int(self.cfg.rows), int(self.cfg.cols)
        L = np.zeros((rows, cols), np.uint8)
        R = np.zeros((rows, cols), np.uint8)
        self.check(self.fn("get_equalized_images")(self.ctx, C.c_int(stream), _p(L, C.c_uint8), _p(R, C.c_uint8)))
        return L, R

    def equalization_histograms(self, stream=0):
        """uint32 [2, 256]: the counts of the left and right image of the last submitted frame of `stream`."""
        h = np.zeros((2, 256), np.uint32)
        self.check(self.fn("get_equalization_histograms")(self.ctx, C.c_int(stream), _p(h, C.c_uint32)))
        return h

    # -- CLAHE of the input pair, the second mode of the equalisation slot (vslam_set_clahe) ------------------------------
    def set_clahe(self, on=True, clip_limit=40.0, tiles=(8, 8)):
        """tiles = (tilesX, tilesY).  equalized_images() returns the CLAHE pair while this is on."""
        self.check(self.fn("set_clahe")(self.ctx, C.c_int(1 if on else 0), C.c_double(clip_limit), C.c_int(int(tiles[0])), C.c_int(int(tiles[1]))))
        self.clahe_tiles = (int(tiles[0]), int(tiles[1])) if on else None

    def clahe_luts(self, stream=0):
        """uint8 [2, tilesY, tilesX, 256]: the tables of the left and right image of the last submitted frame of `stream`."""
        return _clahe_luts(lambda buf: self.check(self.fn("get_clahe_luts")(self.ctx, C.c_int(stream), _p(buf, C.c_uint8))), getattr(self, "clahe_tiles", None), 2)

    # -- colour input (vslam_set_color_input) ---------------------------------------------------------------------------
    def set_color_input(self, fmt):
        """fmt: color.BGR8 / RGB8 / BGRA8 / RGBA8, or color.GRAY8 to switch it off.  While set, the frame entries take interleaved colour
        images (process_host: [n_streams, rows, cols, channels]; device entries: strides in bytes)."""
        self.check(self.fn("set_color_input")(self.ctx, C.c_int(int(fmt))))
        self.color = int(fmt)

    def gray_images(self, stream=0):
        """The grey pair the last submitted frame of `stream` was converted to, at the input size (the raw size of a rectifying context)."""
        rows, cols = self._incoming_size()
        L = np.zeros((rows, cols), np.uint8)
        R = np.zeros((rows, cols), np.uint8)
        self.check(self.fn("get_gray_images")(self.ctx, C.c_int(stream), _p(L, C.c_uint8), _p(R, C.c_uint8)))
        return L, R

    # -- detection masks (vslam_set_detection_mask, vslam_set_frame_masks; semantics: mask.py) ------------------------------
    def _mask_side(self, m, lead):
        """One side's masks as (address, row stride, image stride, keep-alive): a uint8 numpy array or a torch tensor, [rows, stride] or
        with `lead` a leading stream axis, unit column stride.  None stays None."""
        if m is None:
            return None
        if hasattr(m, "data_ptr"):            # a torch tensor: read in place
            if str(m.dtype) != "torch.uint8" or m.stride(-1) != 1:
                raise ValueError("mask: a uint8 tensor with unit column stride is required")
            shape, strides, addr, keep = tuple(m.shape), tuple(m.stride()), m.data_ptr(), m
        else:
            a = np.asarray(m)
            if a.dtype != np.uint8 or a.ndim < 2 or (a.shape[-1] > 1 and a.strides[-1] != 1) or a.strides[-2] < a.shape[-1]:
                a = np.ascontiguousarray(m, np.uint8)
            shape, strides, addr, keep = a.shape, a.strides, a.ctypes.data, a
        if lead and len(shape) == 2:
            shape, strides = (1,) + tuple(shape), (0,) + tuple(strides)
        if len(shape) != (3 if lead else 2) or shape[-2] != self.cfg.rows or shape[-1] < self.cfg.cols:
            raise ValueError("mask: expected %s%d x >= %d, got %s" % ("n_streams x " if lead else "", self.cfg.rows, self.cfg.cols, tuple(shape)))
        if lead and shape[0] != self.n_streams:
            raise ValueError("mask: %d masks for %d streams" % (shape[0], self.n_streams))
        return addr, int(strides[-2]), int(strides[0]) if lead else 0, keep

    def set_detection_mask(self, left=None, right=None, margin=0):
        """The static masks of the two sides (2-D uint8, non-zero = keep; None: that side unmasked; both None: off)."""
        L, R = self._mask_side(left, False), self._mask_side(right, False)
        if L is not None and R is not None and L[1] != R[1]:
            R = self._mask_side(np.ascontiguousarray(right), False)
            L = self._mask_side(np.ascontiguousarray(left), False)
        stride = (L or R or (0, int(self.cfg.cols)))[1]
        self.check(self.fn("set_detection_mask")(self.ctx, C.c_void_p(L[0] if L else None), C.c_void_p(R[0] if R else None), C.c_int32(stride),
                                                 C.c_int32(int(margin))))

    def set_frame_masks(self, left=None, right=None, margin=0):
        """The next frame's masks: uint8 [n_streams, rows, stride] (or [rows, stride] on one stream) per side, numpy arrays (host) or torch
        device tensors (read in place; the caller keeps them alive until that frame has finished).  None: that side has none; both None
        cancels a pending set."""
        dev = [hasattr(m, "data_ptr") and m.is_cuda for m in (left, right) if m is not None]
        if dev and any(dev) != all(dev):
            raise ValueError("set_frame_masks: both sides on the host or both on the device")
        L, R = self._mask_side(left, True), self._mask_side(right, True)
        if L is not None and R is not None and L[1:3] != R[1:3]:
            raise ValueError("set_frame_masks: the two sides differ in their strides")
        _, stride, istride, _ = L or R or (0, int(self.cfg.cols), 0, None)
        self.check(self.fn("set_frame_masks")(self.ctx, C.c_void_p(L[0] if L else None), C.c_void_p(R[0] if R else None), C.c_int32(stride),
                                              C.c_size_t(istride), C.c_int32(int(margin)), C.c_int(1 if dev and dev[0] else 0)))
        # the masks stay valid until their frame has been synchronised: the sets of the frames that may still be queued are kept alive
        self._frame_masks_alive = (getattr(self, "_frame_masks_alive", ()) + ((L, R),))[-3:]

    def detection_mask(self, stream=0, side=0):
        """The effective packed keep-mask the last frame of `stream` used: uint64 [rows, (cols + 63) // 64] (mask.unpack)."""
        rows, tx = int(self.cfg.rows), (int(self.cfg.cols) + 63) // 64
        w = np.zeros((rows, tx), np.uint64)
        self.check(self.fn("get_detection_mask")(self.ctx, C.c_int(stream), C.c_int(side), _p(w, C.c_uint64)))
        return w

    def mask_pack_u8(self, image, margin=0):
        """vslam_mask_pack_u8: image is a 2-D uint8 array or view with unit column stride (its row stride and alignment are passed on as
        they are) -> uint64 [rows, (cols + 63) // 64]."""
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2 or (img.shape[1] > 1 and img.strides[1] != 1) or (img.shape[0] > 1 and img.strides[0] < img.shape[1]):
            img = np.ascontiguousarray(image, np.uint8)
        rows, cols = img.shape
        stride = img.strides[0] if rows > 1 else max(cols, 1)
        w = np.zeros((rows, (cols + 63) // 64), np.uint64)
        self.check(self.fn("mask_pack_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols), C.c_int32(stride),
                                           C.c_int32(int(margin)), _p(w, C.c_uint64)))
        return w

    # -- motion models and pose guesses (vslam_set_motion_model, vslam_set_pose_guess*) -----------------------------------
    def set_motion_model(self, model, dead_reckoning_limit=0):
        """model: MOTION_CONSTANT_VELOCITY (default) / MOTION_NONE / MOTION_CAMERA_ODOMETRY; dead_reckoning_limit N > 0 (odometry only): a
        Tracking stream localizes again after N consecutive frames without an accepted aligner result."""
        self.check(self.fn("set_motion_model")(self.ctx, C.c_int(int(model)), C.c_int32(int(dead_reckoning_limit))))

    def motion_model(self):
        m, n = C.c_int(), C.c_int32()
        self.check(self.fn("get_motion_model")(self.ctx, C.byref(m), C.byref(n)))
        return m.value, n.value

    def set_pose_guess(self, T, stream=0):
        """The external camera_left_to_world (3 x 4, or 12 values row-major) of the stream's next frame."""
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        assert t.size == 12, t.shape
        self.check(self.fn("set_pose_guess")(self.ctx, C.c_int(stream), _p(t, C.c_double)))

    def set_pose_guesses(self, T):
        """Those of all streams: float64 [n_streams, 12] (or [n_streams, 3, 4])."""
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        assert t.size == 12 * self.n_streams, (t.shape, self.n_streams)
        self.check(self.fn("set_pose_guesses")(self.ctx, _p(t, C.c_double), C.c_int(0)))

    def set_pose_guesses_device(self, ptr):
        """ptr: device memory, float64 [n_streams][12], read at the head of the next frame; the caller keeps it alive until that frame is
        finished."""
        self.check(self.fn("set_pose_guesses")(self.ctx, C.c_void_p(ptr), C.c_int(1)))

    def pose_guess(self, stream=0):
        """(guess, guess_previous) of the stream as its last frame left them, float64 [12] each."""
        g, p = np.zeros(12, np.float64), np.zeros(12, np.float64)
        self.check(self.fn("get_pose_guess")(self.ctx, C.c_int(stream), _p(g, C.c_double), _p(p, C.c_double)))
        return g, p

    def motion_prior(self, guess, guess_previous):
        """vslam_motion_prior: inverse(guess[i]) * guess_previous[i], float64 [n, 12] -> [n, 12]."""
        g = np.ascontiguousarray(guess, np.float64).reshape(-1, 12)
        p = np.ascontiguousarray(guess_previous, np.float64).reshape(-1, 12)
        assert g.shape == p.shape, (g.shape, p.shape)
        out = np.zeros_like(g)
        self.check(self.fn("motion_prior")(self.ctx, C.c_int32(len(g)), _p(g, C.c_double), _p(p, C.c_double), _p(out, C.c_double)))
        return out

    # -- readback -----------------------------------------------------------------------------
    def frame_info(self, stream=0):
        fi = FrameInfo()
        self.check(self.fn("get_frame_info")(self.ctx, C.c_int(stream), C.byref(fi)))
        return fi

    def keypoints(self, stream=0, side=0):
        cap = int(self.cfg.max_keypoints)
        n = C.c_int32()
        xy = np.zeros((cap, 2), np.int16)
        score = np.zeros(cap, np.int32)
        desc = np.zeros((cap, 32), np.uint8)
        self.check(self.fn("get_keypoints")(self.ctx, C.c_int(stream), C.c_int(side), C.c_int32(cap), C.byref(n),
                                            _p(xy, C.c_int16), _p(score, C.c_int32), _p(desc, C.c_uint8)))
        k = n.value
        return xy[:k].copy(), score[:k].copy(), desc[:k].copy()

    def points(self, stream=0):
        cap = int(self.cfg.max_points)
        n = C.c_int32()
        kp = np.zeros((cap, 4), np.int16)
        meta = np.zeros((cap, 6), np.int32)
        cam = np.zeros((cap, 3), np.float64)
        lm = np.zeros((cap, 3), np.float64)
        self.check(self.fn("get_points")(self.ctx, C.c_int(stream), C.c_int32(cap), C.byref(n), _p(kp, C.c_int16),
                                         _p(meta, C.c_int32), _p(cam, C.c_double), _p(lm, C.c_double)))
        k = n.value
        return dict(kp=kp[:k].copy(), meta=meta[:k].copy(), cam=cam[:k].copy(), lm=lm[:k].copy())

    # -- landmark map (vslam_enable_map) ------------------------------------------------------------------------------
    def enable_map(self, capacity_per_stream):
        """Keep every landmark of every stream on the device (capacity_per_stream entries each); 0 turns the map off."""
        self.check(self.fn("enable_map")(self.ctx, C.c_int32(int(capacity_per_stream))))

    def map_size(self, stream=0):
        n = C.c_int32()
        self.check(self.fn("get_map_size")(self.ctx, C.c_int(stream), C.byref(n)))
        return n.value

    def map(self, stream=0, first=0):
        """Landmarks first .. of `stream`: dict of numpy arrays id, xyz [n, 3] (world), first_frame, last_frame, updates, desc [n, 32]."""
        cap = max(self.map_size(stream) - int(first), 0)
        n = C.c_int32()
        xyz = np.zeros((max(cap, 1), 3), np.float64)
        info = np.zeros((max(cap, 1), 3), np.int32)
        desc = np.zeros((max(cap, 1), 32), np.uint8)
        self.check(self.fn("get_map")(self.ctx, C.c_int(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n), _p(xyz, C.c_double),
                                      _p(info, C.c_int32), _p(desc, C.c_uint8)))
        k = n.value
        return dict(id=np.arange(int(first), int(first) + k, dtype=np.int32), xyz=xyz[:k].copy(), first_frame=info[:k, 0].copy(),
                    last_frame=info[:k, 1].copy(), updates=info[:k, 2].copy(), desc=desc[:k].copy())

    # -- the map's colours (vslam_enable_map_colors; needs the map and colour input) ------------------------------------
    def enable_map_colors(self, on=True):
        """Keep the colour of every map entry (its left keypoint's pixel in the frame's left colour image at the last update)."""
        self.check(self.fn("enable_map_colors")(self.ctx, C.c_int(1 if on else 0)))

    def map_colors(self, stream=0, first=0):
        """uint8 [n, 3] (r, g, b) of landmarks first .. of `stream`, in map() order."""
        cap = max(self.map_size(stream) - int(first), 0)
        n = C.c_int32()
        rgb = np.zeros((max(cap, 1), 3), np.uint8)
        self.check(self.fn("get_map_colors")(self.ctx, C.c_int(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n), _p(rgb, C.c_uint8)))
        return rgb[:n.value].copy()

    # -- landmark observations (vslam_enable_observations; needs the map) ----------------------------------------------
    def enable_observations(self, capacity_per_stream):
        """Log (landmark id, frame, keypoints) of every point that carries a map id, capacity_per_stream entries per stream; 0 turns it off."""
        self.check(self.fn("enable_observations")(self.ctx, C.c_int32(int(capacity_per_stream))))

    def observation_count(self, stream=0):
        n = C.c_int32()
        self.check(self.fn("get_observation_count")(self.ctx, C.c_int(stream), C.byref(n)))
        return n.value

    def observations(self, stream=0, first=0):
        """Log entries first .. of `stream`: dict of numpy arrays id, frame (0-based per stream), kp [n, 4] (xL, yL, xR, yR)."""
        cap = max(self.observation_count(stream) - int(first), 0)
        n = C.c_int32()
        idf = np.zeros((max(cap, 1), 2), np.int32)
        kp = np.zeros((max(cap, 1), 4), np.int16)
        self.check(self.fn("get_observations")(self.ctx, C.c_int(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n), _p(idf, C.c_int32),
                                               _p(kp, C.c_int16)))
        k = n.value
        return dict(id=idf[:k, 0].copy(), frame=idf[:k, 1].copy(), kp=kp[:k].copy())

    def point_ids(self, stream=0):
        """Map id (or -1) of every point of the finished frame, in points() order; needs the map only."""
        cap = int(self.cfg.max_points)
        n = C.c_int32()
        ids = np.zeros(max(cap, 1), np.int32)
        self.check(self.fn("get_point_ids")(self.ctx, C.c_int(stream), C.c_int32(cap), C.byref(n), _p(ids, C.c_int32)))
        return ids[:n.value].copy()

    def aligner_result(self, stream=0):
        cap = int(self.cfg.max_points)
        n = C.c_int32()
        chi = np.zeros(cap, np.float64)
        inl = np.zeros(cap, np.uint8)
        T = np.zeros(12, np.float64)
        H = np.zeros(36, np.float64)
        self.check(self.fn("get_aligner_result")(self.ctx, C.c_int(stream), C.c_int32(cap), C.byref(n),
                                                 _p(chi, C.c_double), _p(inl, C.c_uint8), _p(T, C.c_double),
                                                 _p(H, C.c_double)))
        k = n.value
        return dict(chi=chi[:k].copy(), inlier=inl[:k].copy(), T=T.reshape(3, 4), H=H.reshape(6, 6))

    def aligner_weights_of(self, stream=0):
        """StereoUVAligner::_weights_translation as the stream's last initialize() left it."""
        cap = int(self.cfg.max_points)
        n = C.c_int32()
        w = np.zeros(cap, np.float64)
        self.check(self.fn("get_aligner_weights")(self.ctx, C.c_int(stream), C.c_int32(cap), C.byref(n), _p(w, C.c_double)))
        return w[:n.value].copy()

    def aligner_weights(self, cfg, sizes, inverse_depth, depth):
        """Weights after each of a sequence of StereoUVAligner::initialize calls on one aligner (known-answer tests)."""
        n = np.ascontiguousarray(sizes, np.int32); inv = np.ascontiguousarray(inverse_depth, np.int32)
        d = np.ascontiguousarray(depth, np.float64)
        out = np.zeros(max(int(n.sum()), 1), np.float64)
        first = (self.ctx,) if self.prefix == "vslam_" else (C.byref(cfg),)
        self.check(self.fn("aligner_weights")(*first, C.c_int32(n.shape[0]), _p(n, C.c_int32), _p(inv, C.c_int32), _p(d, C.c_double),
                                              _p(out, C.c_double)))
        return out[:int(n.sum())]

    def poses(self, stream, first, count):
        out = np.zeros((count, 12), np.float64)
        self.check(self.fn("get_poses")(self.ctx, C.c_int(stream), C.c_int32(first), C.c_int32(count),
                                        _p(out, C.c_double)))
        return out.reshape(count, 3, 4)

    # -- stage views (copies of what the pointers show, taken at once: the buffer is reused by the next view call) --------------
    def view_keypoints(self, stream=0):
        v = KeypointsView()
        self.check(self.fn("view_keypoints")(self.ctx, C.c_int(stream), C.byref(v)))
        out = []
        for d in (0, 1):
            n = v.n[d]
            out.append((np.ctypeslib.as_array(v.xy[d], (max(n, 1), 2))[:n].copy(), np.ctypeslib.as_array(v.score[d], (max(n, 1),))[:n].copy(),
                        np.ctypeslib.as_array(v.desc[d], (max(n, 1), 32))[:n].copy()))
        return out

    def view_keypoints_xy(self, stream=0):
        """Coordinates and scores as soon as the detector has written them (descriptors: view_keypoints afterwards)."""
        v = KeypointsView()
        self.check(self.fn("view_keypoints_xy")(self.ctx, C.c_int(stream), C.byref(v)))
        out = []
        for d in (0, 1):
            n = v.n[d]
            out.append((np.ctypeslib.as_array(v.xy[d], (max(n, 1), 2))[:n].copy(), np.ctypeslib.as_array(v.score[d], (max(n, 1),))[:n].copy(), bool(v.desc[d])))
        return out

    def view_track(self, stream=0):
        v = TrackView()
        self.check(self.fn("view_track")(self.ctx, C.c_int(stream), C.byref(v)))
        return dict(n_tracked_landmarks=v.n_tracked_landmarks, tracked4=np.ctypeslib.as_array(v.tracked4, (max(v.n_tracked, 1), 4))[:v.n_tracked].copy(),
                    lost=np.ctypeslib.as_array(v.lost, (max(v.n_lost, 1),))[:v.n_lost].copy())

    def view_aligner(self, stream=0):
        v = AlignerView()
        self.check(self.fn("view_aligner")(self.ctx, C.c_int(stream), C.byref(v)))
        return dict(n_inliers=v.n_inliers, n_outliers=v.n_outliers, iterations=v.iterations, converged=v.converged, total_error=v.total_error,
                    chi=np.ctypeslib.as_array(v.chi, (max(v.n, 1),))[:v.n].copy(), inlier=np.ctypeslib.as_array(v.inlier, (max(v.n, 1),))[:v.n].copy(),
                    T=np.array(v.T).reshape(3, 4), H=np.array(v.H).reshape(6, 6))

    def view_points(self, stream=0, in_progress=False):
        v = PointsView()
        self.check(self.fn("view_points")(self.ctx, C.c_int(stream), C.c_int(1 if in_progress else 0), C.byref(v)))
        n, f = v.n, v.first_full
        out = dict(n=n, first_full=f, kp=np.ctypeslib.as_array(v.kp, (max(n, 1), 4))[:n].copy(), meta=np.ctypeslib.as_array(v.meta, (max(n, 1), 6))[:n].copy(),
                   cam=np.ctypeslib.as_array(v.cam, (max(n, 1), 3))[:n].copy(), info=FrameInfo.from_buffer_copy(bytes(v.info)),
                   seconds=[v.seconds_tracking, v.seconds_pose_optimization, v.seconds_point_recovery, v.seconds_landmark_optimization, v.seconds_point_triangulation])
        out["desc"] = np.ctypeslib.as_array(v.desc, (max(n, 1), 64))[:n].copy() if in_progress else None
        return out

    # -- stand-alone stages ---------------------------------------------------------------------
    def fast_detect(self, image, roi, threshold, cap=65536):
        image = np.ascontiguousarray(image, np.uint8)
        rows, stride = image.shape
        x, y, w, h = roi
        n = C.c_int32()
        xy = np.zeros((cap, 2), np.int16)
        score = np.zeros(cap, np.int32)
        self.check(self.fn("fast_detect")(self.ctx, _p(image, C.c_uint8), C.c_int32(rows), C.c_int32(stride),
                                          C.c_int32(stride), C.c_int32(x), C.c_int32(y), C.c_int32(w), C.c_int32(h),
                                          C.c_int32(threshold), C.c_int32(cap), C.byref(n), _p(xy, C.c_int16),
                                          _p(score, C.c_int32)))
        return xy[:n.value].copy(), score[:n.value].copy()

    def brief_describe(self, image, xy):
        image = np.ascontiguousarray(image, np.uint8)
        xy = np.ascontiguousarray(xy, np.int16)
        rows, stride = image.shape
        n = xy.shape[0]
        keep = np.zeros(n, np.uint8)
        desc = np.zeros((n, 32), np.uint8)
        self.check(self.fn("brief_describe")(self.ctx, _p(image, C.c_uint8), C.c_int32(rows), C.c_int32(stride),
                                             C.c_int32(stride), C.c_int32(n), _p(xy, C.c_int16), _p(keep, C.c_uint8),
                                             _p(desc, C.c_uint8)))
        return keep, desc

    # -- descriptor test pairs (run-time data, one table per device) --------------------------------
    def get_pattern(self, which, device=0):
        """which: "brief" ({y1, x1, y2, x2}) or "orb" ({x1, y1, x2, y2}); returns int8 [256, 4]."""
        out = np.zeros((256, 4), np.int8)
        rc = getattr(self.lib, self.prefix + "get_%s_pattern" % which)(C.c_int(device), _p(out, C.c_int8))
        if rc != 0:
            raise VslamError(rc, "get_%s_pattern" % which)
        return out

    def set_pattern(self, which, pairs, device=0):
        pairs = np.ascontiguousarray(pairs, np.int8).reshape(256, 4)
        rc = getattr(self.lib, self.prefix + "set_%s_pattern" % which)(C.c_int(device), _p(pairs, C.c_int8))
        if rc != 0:
            raise VslamError(rc, "set_%s_pattern: table rejected" % which)

    def knn2(self, query, train, norm=0):
        query = np.ascontiguousarray(query, np.uint8)
        train = np.ascontiguousarray(train, np.uint8)
        nq, nt = query.shape[0], train.shape[0]
        idx = np.zeros((nq, 2), np.int32)
        dist = np.zeros((nq, 2), np.float32)
        self.check(self.fn("knn2")(self.ctx, C.c_int(norm), C.c_int32(nq), _p(query, C.c_uint8), C.c_int32(nt),
                                   _p(train, C.c_uint8), _p(idx, C.c_int32), _p(dist, C.c_float)))
        return idx, dist

    def align_points(self, moving, fixed, omega, weight, T_init):
        moving = np.ascontiguousarray(moving, np.float64)
        fixed = np.ascontiguousarray(fixed, np.float64)
        omega = np.ascontiguousarray(omega, np.float64)
        weight = np.ascontiguousarray(weight, np.float64)
        T_init = np.ascontiguousarray(T_init, np.float64).reshape(12)
        n = moving.shape[0]
        T = np.zeros(12, np.float64)
        chi = np.zeros(n, np.float64)
        inl = np.zeros(n, np.uint8)
        ninl, its = C.c_int32(), C.c_int32()
        err = C.c_double()
        H = np.zeros(36, np.float64)
        self.check(self.fn("align_points")(self.ctx, C.c_int32(n), _p(moving, C.c_double), _p(fixed, C.c_double),
                                           _p(omega, C.c_double), _p(weight, C.c_double), _p(T_init, C.c_double),
                                           _p(T, C.c_double), _p(chi, C.c_double), _p(inl, C.c_uint8), C.byref(ninl),
                                           C.byref(err), C.byref(its), _p(H, C.c_double)))
        return dict(T=T.reshape(3, 4), chi=chi, inlier=inl, n_inliers=ninl.value, total_error=err.value,
                    iterations=its.value, H=H.reshape(6, 6))


    def align_points_uvd(self, moving, fixed_uvd, omega_uv, omega_depth, weight, T_init):
        moving = np.ascontiguousarray(moving, np.float64)
        fixed = np.ascontiguousarray(fixed_uvd, np.float64)
        ouv = np.ascontiguousarray(omega_uv, np.float64)
        od = np.ascontiguousarray(omega_depth, np.float64)
        weight = np.ascontiguousarray(weight, np.float64)
        T_init = np.ascontiguousarray(T_init, np.float64).reshape(12)
        n = moving.shape[0]
        T = np.zeros(12, np.float64)
        chi = np.zeros(n, np.float64)
        inl = np.zeros(n, np.uint8)
        ninl, its = C.c_int32(), C.c_int32()
        err = C.c_double()
        H = np.zeros(36, np.float64)
        self.check(self.fn("align_points_uvd")(self.ctx, C.c_int32(n), _p(moving, C.c_double), _p(fixed, C.c_double),
                                               _p(ouv, C.c_double), _p(od, C.c_double), _p(weight, C.c_double),
                                               _p(T_init, C.c_double), _p(T, C.c_double), _p(chi, C.c_double),
                                               _p(inl, C.c_uint8), C.byref(ninl), C.byref(err), C.byref(its),
                                               _p(H, C.c_double)))
        return dict(T=T.reshape(3, 4), chi=chi, inlier=inl, n_inliers=ninl.value, total_error=err.value,
                    iterations=its.value, H=H.reshape(6, 6))

    def track_match(self, T, d, tau_track, tau_tri, by_appearance, cam, prev_desc_left, prev_desc_right, epi,
                    rc_left, desc_left, rc_right, desc_right):
        """StereoFramePointGenerator::track on caller-provided data (known-answer tests): returns (tracked [n][4], lost)."""
        T = np.ascontiguousarray(T, np.float64).reshape(12)
        cam = np.ascontiguousarray(cam, np.float64)
        pdl = np.ascontiguousarray(prev_desc_left, np.uint8); pdr = np.ascontiguousarray(prev_desc_right, np.uint8)
        epi = np.ascontiguousarray(epi, np.int32)
        rcl = np.ascontiguousarray(rc_left, np.int32); dl = np.ascontiguousarray(desc_left, np.uint8)
        rcr = np.ascontiguousarray(rc_right, np.int32); dr = np.ascontiguousarray(desc_right, np.uint8)
        n = cam.shape[0]
        out = np.zeros((max(n, 1), 4), np.int32)
        lost = np.zeros(max(n, 1), np.int32)
        nt, nl = C.c_int32(), C.c_int32()
        self.check(self.fn("track_match")(self.ctx, _p(T, C.c_double), C.c_int32(int(d)), C.c_double(float(tau_track)),
                                          C.c_double(float(tau_tri)), C.c_int32(int(by_appearance)), C.c_int32(n),
                                          _p(cam, C.c_double), _p(pdl, C.c_uint8), _p(pdr, C.c_uint8), _p(epi, C.c_int32),
                                          C.c_int32(rcl.shape[0]), _p(rcl, C.c_int32), _p(dl, C.c_uint8),
                                          C.c_int32(rcr.shape[0]), _p(rcr, C.c_int32), _p(dr, C.c_uint8),
                                          C.byref(nt), _p(out, C.c_int32), C.byref(nl), _p(lost, C.c_int32)))
        return out[:nt.value].copy(), lost[:nl.value].copy()


    def stereo_match(self, tau_tri, rc_left, desc_left, rc_right, desc_right, cap=8192):
        """StereoFramePointGenerator::compute on caller-provided features: (left, right, distance, offset) rows."""
        rcl = np.ascontiguousarray(rc_left, np.int32); dl = np.ascontiguousarray(desc_left, np.uint8)
        rcr = np.ascontiguousarray(rc_right, np.int32); dr = np.ascontiguousarray(desc_right, np.uint8)
        out = np.zeros((cap, 4), np.int32)
        n = C.c_int32()
        self.check(self.fn("stereo_match")(self.ctx, C.c_double(float(tau_tri)), C.c_int32(rcl.shape[0]), _p(rcl, C.c_int32),
                                           _p(dl, C.c_uint8), C.c_int32(rcr.shape[0]), _p(rcr, C.c_int32), _p(dr, C.c_uint8),
                                           C.c_int32(cap), C.byref(n), _p(out, C.c_int32)))
        return out[:n.value].copy()

    def stereo_recover(self, image_left, image_right, w2c, has_landmark, landmark_world, prev_desc_left, prev_desc_right, tau_track, tau_tri,
                       row_stride=None):
        """StereoFramePointGenerator::recoverPoints on caller-provided lost points (known-answer tests): dict of
        index / xy4 / dist / desc / xyz rows of the recovered points in lost-list order.  row_stride: the images are [rows, row_stride]
        arrays (padded rows); default: their own width."""
        L = np.ascontiguousarray(image_left, np.uint8); R = np.ascontiguousarray(image_right, np.uint8)
        stride = L.shape[1] if row_stride is None else int(row_stride)
        if L.shape[1] != stride or R.shape != L.shape:
            raise ValueError("stereo_recover: images must be two [rows, row_stride] arrays")
        w = np.ascontiguousarray(w2c, np.float64).reshape(12)
        hl = np.ascontiguousarray(has_landmark, np.uint8); lm = np.ascontiguousarray(landmark_world, np.float64)
        pdl = np.ascontiguousarray(prev_desc_left, np.uint8); pdr = np.ascontiguousarray(prev_desc_right, np.uint8)
        n = hl.shape[0]
        idx = np.zeros(max(n, 1), np.int32); xy4 = np.zeros((max(n, 1), 4), np.int32); dist = np.zeros(max(n, 1), np.int32)
        desc = np.zeros((max(n, 1), 64), np.uint8); xyz = np.zeros((max(n, 1), 3), np.float64)
        k = C.c_int32()
        head = (self.ctx,) if self.prefix == "vslam_" else (C.byref(self.cfg),)
        self.check(self.fn("stereo_recover")(*head, _p(L, C.c_uint8), _p(R, C.c_uint8), C.c_int32(stride), _p(w, C.c_double), C.c_int32(n),
                                             _p(hl, C.c_uint8), _p(lm, C.c_double), _p(pdl, C.c_uint8), _p(pdr, C.c_uint8),
                                             C.c_double(float(tau_track)), C.c_double(float(tau_tri)), C.byref(k), _p(idx, C.c_int32),
                                             _p(xy4, C.c_int32), _p(dist, C.c_int32), _p(desc, C.c_uint8), _p(xyz, C.c_double)))
        k = k.value
        return dict(index=idx[:k].copy(), xy4=xy4[:k].copy(), dist=dist[:k].copy(), desc=desc[:k].copy(), xyz=xyz[:k].copy())

    # -- RGB-D components.  The oracle's entry points (prefix orc_) take no context. --------------------------------
    def _ctx_args(self):
        return (self.ctx,) if self.prefix == "vslam_" else ()

    def depth_space_map(self, params, depth):
        depth = np.ascontiguousarray(depth, np.uint16)
        rows, cols = depth.shape
        space = np.zeros((rows, cols, 3), np.float32)
        rmap = np.zeros((rows, cols), np.int16); cmap = np.zeros((rows, cols), np.int16)
        self.check(self.fn("depth_space_map")(*self._ctx_args(), C.byref(params), _p(depth, C.c_uint16), C.c_int32(cols),
                                              _p(space, C.c_float), _p(rmap, C.c_int16), _p(cmap, C.c_int16)))
        return space, rmap, cmap

    def depth_compute(self, params, space, rc_features, rc_tracked, cap=8192):
        """space: host map or None (HIP only: the map the last depth_space_map call left on the device)."""
        rcf = np.ascontiguousarray(rc_features, np.int32).reshape(-1, 2)
        rct = np.ascontiguousarray(rc_tracked, np.int32).reshape(-1, 2)
        sp = None if space is None else np.ascontiguousarray(space, np.float32)
        nf, xyz = np.zeros(cap, np.int32), np.zeros((cap, 3), np.float64)
        tf_, txyz = np.zeros(cap, np.int32), np.zeros((cap, 3), np.float64)
        nn, nt = C.c_int32(), C.c_int32()
        self.check(self.fn("depth_compute")(*self._ctx_args(), C.byref(params), None if sp is None else _p(sp, C.c_float),
                                            C.c_int32(rcf.shape[0]), _p(rcf, C.c_int32), C.c_int32(rct.shape[0]),
                                            _p(rct, C.c_int32), C.c_int32(cap), C.byref(nn), _p(nf, C.c_int32),
                                            _p(xyz, C.c_double), C.byref(nt), _p(tf_, C.c_int32), _p(txyz, C.c_double)))
        return nf[:nn.value].copy(), xyz[:nn.value].copy(), tf_[:nt.value].copy(), txyz[:nt.value].copy()

    def depth_track(self, params, space, T, d, tau, by_appearance, cam, prev_desc, prev_flags, rc_left, desc_left):
        """DepthFramePointGenerator::track on caller-provided data: (tracked [n][2], xyz [n][3], temporary [m][2], lost, landmarks)."""
        T = np.ascontiguousarray(T, np.float64).reshape(12)
        cam = np.ascontiguousarray(cam, np.float64).reshape(-1, 3)
        pd = np.ascontiguousarray(prev_desc, np.uint8); pf = np.ascontiguousarray(prev_flags, np.uint8)
        rc = np.ascontiguousarray(rc_left, np.int32).reshape(-1, 2); dl = np.ascontiguousarray(desc_left, np.uint8)
        sp = None if space is None else np.ascontiguousarray(space, np.float32)
        nP = cam.shape[0]
        out2, xyz = np.zeros((max(nP, 1), 2), np.int32), np.zeros((max(nP, 1), 3), np.float64)
        tmp2, lost = np.zeros((max(nP, 1), 2), np.int32), np.zeros(max(nP, 1), np.int32)
        nt, ntmp, nl, nlm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.check(self.fn("depth_track")(*self._ctx_args(), C.byref(params), None if sp is None else _p(sp, C.c_float), _p(T, C.c_double),
                                          C.c_int32(int(d)), C.c_double(float(tau)), C.c_int32(int(by_appearance)), C.c_int32(nP),
                                          _p(cam, C.c_double), _p(pd, C.c_uint8), _p(pf, C.c_uint8), C.c_int32(rc.shape[0]),
                                          _p(rc, C.c_int32), _p(dl, C.c_uint8), C.byref(nt), _p(out2, C.c_int32), _p(xyz, C.c_double),
                                          C.byref(ntmp), _p(tmp2, C.c_int32), C.byref(nl), _p(lost, C.c_int32), C.byref(nlm)))
        return out2[:nt.value].copy(), xyz[:nt.value].copy(), tmp2[:ntmp.value].copy(), lost[:nl.value].copy(), nlm.value

    def depth_recover(self, params, space, image_left, world_to_camera_left, has_landmark, landmark_world, prev_desc, keypoint_size, tau,
                      row_stride=None):
        """DepthFramePointGenerator::recoverPoints on caller-provided data: (lost-list index, keypoint xy, descriptor, xyz).
        row_stride: the image is a [rows, row_stride] array (padded rows); default: its own width."""
        img = np.ascontiguousarray(image_left, np.uint8)
        stride = img.shape[1] if row_stride is None else int(row_stride)
        if img.shape[1] != stride:
            raise ValueError("depth_recover: the image must be a [rows, row_stride] array")
        w2c = np.ascontiguousarray(world_to_camera_left, np.float64).reshape(12)
        hl = np.ascontiguousarray(has_landmark, np.uint8); lm = np.ascontiguousarray(landmark_world, np.float64).reshape(-1, 3)
        pd = np.ascontiguousarray(prev_desc, np.uint8)
        sp = None if space is None else np.ascontiguousarray(space, np.float32)
        n = lm.shape[0]
        idx, xy = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2), np.float32)
        desc, xyz = np.zeros((max(n, 1), 32), np.uint8), np.zeros((max(n, 1), 3), np.float64)
        nr = C.c_int32()
        self.check(self.fn("depth_recover")(*self._ctx_args(), C.byref(params), None if sp is None else _p(sp, C.c_float), _p(img, C.c_uint8),
                                            C.c_int32(stride), _p(w2c, C.c_double), C.c_int32(n), _p(hl, C.c_uint8), _p(lm, C.c_double),
                                            _p(pd, C.c_uint8), C.c_float(float(keypoint_size)), C.c_double(float(tau)), C.byref(nr),
                                            _p(idx, C.c_int32), _p(xy, C.c_float), _p(desc, C.c_uint8), _p(xyz, C.c_double)))
        k = nr.value
        return idx[:k].copy(), xy[:k].copy(), desc[:k].copy(), xyz[:k].copy()

    def landmark_update(self, cfg, offsets, frame_of, world_to_camera, camera_to_world, cam, world, updates):
        """Landmark::update for a batch of landmarks (last measurement of each list = the new observation)."""
        off = np.ascontiguousarray(offsets, np.int32); fo = np.ascontiguousarray(frame_of, np.int32)
        w2c = np.ascontiguousarray(world_to_camera, np.float64).reshape(-1, 12); c2w = np.ascontiguousarray(camera_to_world, np.float64).reshape(-1, 12)
        cm = np.ascontiguousarray(cam, np.float64).reshape(-1, 3)
        w = np.array(world, np.float64).reshape(-1, 3).copy(); u = np.array(updates, np.int32).copy()
        first = (self.ctx,) if self.prefix == "vslam_" else (C.byref(cfg),)
        self.check(self.fn("landmark_update")(*first, C.c_int32(w.shape[0]), _p(off, C.c_int32), _p(fo, C.c_int32), C.c_int32(w2c.shape[0]),
                                              _p(w2c, C.c_double), _p(c2w, C.c_double), _p(cm, C.c_double), _p(w, C.c_double), _p(u, C.c_int32)))
        return w, u

    # -- OrbDetector components -------------------------------------------------------------------------------------
    def resize_linear_u8(self, image, dst_rows, dst_cols):
        img = np.ascontiguousarray(image, np.uint8)
        dst = np.zeros((int(dst_rows), int(dst_cols)), np.uint8)
        self.check(self.fn("resize_linear_u8")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                               C.c_int32(img.shape[1]), _p(dst, C.c_uint8), C.c_int32(dst.shape[0]), C.c_int32(dst.shape[1])))
        return dst

    def equalize_hist_u8(self, image):
        """vslam_equalize_hist_u8: image is a 2-D uint8 array or view with unit column stride (its row stride and alignment are passed
        on as they are) -> (dst, hist256)."""
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2 or (img.shape[1] > 1 and img.strides[1] != 1) or (img.shape[0] > 1 and img.strides[0] < img.shape[1]):
            img = np.ascontiguousarray(image, np.uint8)
        rows, cols = img.shape
        stride = img.strides[0] if rows > 1 else max(cols, 1)
        dst = np.zeros((rows, cols), np.uint8)
        hist = np.zeros(256, np.uint32)
        self.check(self.fn("equalize_hist_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols), C.c_int32(stride),
                                               _p(dst, C.c_uint8), _p(hist, C.c_uint32)))
        return dst, hist

    def clahe_u8(self, image, clip_limit=40.0, tiles=(8, 8), out=None):
        """vslam_clahe_u8: image (and out, when given) is a 2-D uint8 array or view with unit column stride; row strides and alignments
        are passed on as they are.  out=None: a dense result; out is image: in place.  -> (dst, luts [tilesY, tilesX, 256])."""
        img = np.asarray(image)
        dst = np.zeros(img.shape, np.uint8) if out is None else out
        for a in (img, dst):
            if a.dtype != np.uint8 or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 1) or (a.shape[0] > 1 and a.strides[0] < a.shape[1]):
                raise ValueError("clahe_u8: 2-D uint8 arrays with unit column stride are required")
        if dst.shape != img.shape:
            raise ValueError("clahe_u8: out has another shape")
        rows, cols = img.shape
        tx, ty = int(tiles[0]), int(tiles[1])
        luts = np.zeros((max(ty, 0), max(tx, 0), 256), np.uint8)
        stride = lambda a: a.strides[0] if rows > 1 else max(cols, 1)
        self.check(self.fn("clahe_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols), C.c_int32(stride(img)),
                                       C.c_double(clip_limit), C.c_int32(tx), C.c_int32(ty), C.c_void_p(dst.ctypes.data), C.c_int32(stride(dst)),
                                       _p(luts, C.c_uint8)))
        return dst, luts

    def bilateral_depth_u16(self, depth, depth_scale, sigma_color=2.0, sigma_space=2.0, out=None, row_stride=None):
        """vslam_bilateral_depth_u16: depth (and out, when given) is a 2-D uint16 array or view with unit column stride; row strides and
        alignments are passed on as they are.  out=None: a dense result; out is depth: in place.  row_stride (elements) overrides the
        source's own, for the refusal tests.  -> (dst, lut float32 [4098])."""
        img = np.asarray(depth)
        dst = np.zeros(img.shape, np.uint16) if out is None else out
        for a in (img, dst):
            if a.dtype != np.uint16 or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 2) or (a.shape[0] > 1 and (a.strides[0] < 2 * a.shape[1] or a.strides[0] % 2)):
                raise ValueError("bilateral_depth_u16: 2-D uint16 arrays with unit column stride are required")
        if dst.shape != img.shape:
            raise ValueError("bilateral_depth_u16: out has another shape")
        rows, cols = img.shape
        lut = np.zeros(4098, np.float32)
        stride = lambda a: a.strides[0] // 2 if rows > 1 else max(cols, 1)
        self.check(self.fn("bilateral_depth_u16")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols),
                                                  C.c_int32(stride(img) if row_stride is None else int(row_stride)), C.c_double(depth_scale),
                                                  C.c_double(sigma_color), C.c_double(sigma_space), C.c_void_p(dst.ctypes.data),
                                                  C.c_int32(stride(dst)), _p(lut, C.c_float)))
        return dst, lut

    def gray_u8(self, image, fmt, cols=None):
        """vslam_gray_u8: image is a uint8 array [rows, cols, channels], or a 2-D array or view [rows, >= channels * cols bytes] with unit
        column stride whose row stride and alignment are passed on as they are (cols is then required) -> grey [rows, cols]."""
        img = np.asarray(image)
        if img.ndim == 3:
            img = np.ascontiguousarray(img, np.uint8)
            cols = img.shape[1]
            img = img.reshape(img.shape[0], -1)
        elif img.dtype != np.uint8 or img.ndim != 2 or (img.shape[1] > 1 and img.strides[1] != 1) or (img.shape[0] > 1 and img.strides[0] < img.shape[1]):
            img = np.ascontiguousarray(image, np.uint8)
        if img.ndim != 2 or cols is None:
            raise ValueError("gray_u8: a [rows, cols, channels] array, or a [rows, bytes] array together with cols")
        rows = img.shape[0]
        stride = img.strides[0] if rows > 1 else max(img.shape[1], 1)
        dst = np.zeros((max(rows, 0), max(int(cols), 0)), np.uint8)
        self.check(self.fn("gray_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(int(cols)), C.c_int32(stride), C.c_int(int(fmt)),
                                      _p(dst, C.c_uint8)))
        return dst

    def _downscale(self, name, dtype, image, factor, out, row_stride, dst_row_stride):
        size = np.dtype(dtype).itemsize
        img = np.asarray(image)

        def plain(a):
            return a.dtype == dtype and a.ndim == 2 and (a.shape[1] <= 1 or a.strides[1] == size) and \
                (a.shape[0] <= 1 or (a.strides[0] >= size * a.shape[1] and a.strides[0] % size == 0))
        if not plain(img):
            raise ValueError("%s: a 2-D %s array with unit column stride is required" % (name, np.dtype(dtype).name))
        rows, cols = img.shape
        f = int(factor)
        orows, ocols = (rows // f, cols // f) if f > 0 else (0, 0)
        dst = np.zeros((orows, ocols), dtype) if out is None else out
        if not plain(dst) or dst.shape != (orows, ocols):
            raise ValueError("%s: out is not a 2-D %s array of %d x %d with unit column stride" % (name, np.dtype(dtype).name, orows, ocols))
        stride = lambda a: a.strides[0] // size if a.shape[0] > 1 else max(a.shape[1], 1)
        self.check(self.fn(name)(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols),
                                 C.c_int32(stride(img) if row_stride is None else int(row_stride)), C.c_int32(f), C.c_void_p(dst.ctypes.data),
                                 C.c_int32(stride(dst) if dst_row_stride is None else int(dst_row_stride))))
        return dst

    def downscale_u8(self, image, factor, out=None, row_stride=None, dst_row_stride=None):
        """vslam_downscale_u8: image (and out, when given) is a 2-D uint8 array or view with unit column stride; row strides and alignments
        are passed on as they are.  out=None: a dense result.  row_stride / dst_row_stride (bytes) override the arrays' own, for the
        refusal tests.  -> uint8 [rows // factor, cols // factor]."""
        return self._downscale("downscale_u8", np.uint8, image, factor, out, row_stride, dst_row_stride)

    def downscale_depth_u16(self, depth, factor, out=None, row_stride=None, dst_row_stride=None):
        """vslam_downscale_depth_u16: as downscale_u8 on 2-D uint16 arrays or views; the strides are in elements."""
        return self._downscale("downscale_depth_u16", np.uint16, depth, factor, out, row_stride, dst_row_stride)

    def smooth_u8(self, image, mode, ksize, row_stride=None):
        """vslam_smooth_u8: image is a 2-D uint8 array or view with unit column stride; its row stride and alignment are passed on as
        they are (row_stride, bytes, overrides the array's own, for the refusal tests) -> a dense uint8 [rows, cols]."""
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2 or (img.shape[1] > 1 and img.strides[1] != 1) or (img.shape[0] > 1 and img.strides[0] < img.shape[1]):
            raise ValueError("smooth_u8: a 2-D uint8 array with unit column stride is required")
        rows, cols = img.shape
        stride = img.strides[0] if rows > 1 else max(cols, 1)
        dst = np.zeros((rows, cols), np.uint8)
        self.check(self.fn("smooth_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(cols),
                                        C.c_int32(stride if row_stride is None else int(row_stride)), C.c_int(int(mode)), C.c_int32(int(ksize)),
                                        C.c_void_p(dst.ctypes.data)))
        return dst

    def sample_color_u8(self, image, fmt, xy, maps=None, cols=None):
        """vslam_sample_color_u8: image as in gray_u8 ([rows, cols, channels], or [rows, bytes] with cols, strides and alignment passed on);
        xy int16 [n, 2] (x, y); maps None or (map_xy int16 [R, C, 2], map_a uint16 [R, C]) -> uint8 [n, 3] (r, g, b)."""
        img = np.asarray(image)
        if img.ndim == 3:
            img = np.ascontiguousarray(img, np.uint8)
            cols = img.shape[1]
            img = img.reshape(img.shape[0], -1)
        elif img.dtype != np.uint8 or img.ndim != 2 or (img.shape[1] > 1 and img.strides[1] != 1) or (img.shape[0] > 1 and img.strides[0] < img.shape[1]):
            img = np.ascontiguousarray(image, np.uint8)
        if img.ndim != 2 or cols is None:
            raise ValueError("sample_color_u8: a [rows, cols, channels] array, or a [rows, bytes] array together with cols")
        rows = img.shape[0]
        stride = img.strides[0] if rows > 1 else max(img.shape[1], 1)
        pts = np.ascontiguousarray(xy, np.int16).reshape(-1, 2)
        mxy = ma = None
        mr = mc = 0
        if maps is not None:
            mxy = np.ascontiguousarray(maps[0], np.int16)
            ma = np.ascontiguousarray(maps[1], np.uint16)
            assert mxy.shape[:2] == ma.shape and mxy.shape[2] == 2
            mr, mc = ma.shape
        rgb = np.zeros((max(len(pts), 1), 3), np.uint8)
        self.check(self.fn("sample_color_u8")(*self._ctx_args(), C.c_void_p(img.ctypes.data), C.c_int32(rows), C.c_int32(int(cols)), C.c_int32(stride),
                                              C.c_int(int(fmt)), None if mxy is None else _p(mxy, C.c_int16), None if ma is None else _p(ma, C.c_uint16),
                                              C.c_int32(mr), C.c_int32(mc), _p(pts, C.c_int16), C.c_int32(len(pts)), _p(rgb, C.c_uint8)))
        return rgb[:len(pts)].copy()

    def remap_u8(self, image, map_xy, map_a, cols=None):
        """vslam_remap_u8: image is rows x stride (cols <= stride bytes used), the maps give the output size."""
        img = np.ascontiguousarray(image, np.uint8)
        mxy = np.ascontiguousarray(map_xy, np.int16)
        ma = np.ascontiguousarray(map_a, np.uint16)
        assert mxy.shape[:2] == ma.shape and mxy.shape[2] == 2
        cols = img.shape[1] if cols is None else int(cols)
        dst = np.zeros(ma.shape, np.uint8)
        self.check(self.fn("remap_u8")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(cols), C.c_int32(img.shape[1]),
                                       _p(mxy, C.c_int16), _p(ma, C.c_uint16), C.c_int32(ma.shape[0]), C.c_int32(ma.shape[1]), _p(dst, C.c_uint8)))
        return dst

    def remap_nearest_u16(self, image, map_xy, map_a, cols=None):
        """vslam_remap_nearest_u16: image is rows x stride uint16 (cols <= stride elements used), the maps give the output size."""
        img = np.ascontiguousarray(image, np.uint16)
        mxy = np.ascontiguousarray(map_xy, np.int16)
        ma = np.ascontiguousarray(map_a, np.uint16)
        assert mxy.shape[:2] == ma.shape and mxy.shape[2] == 2
        cols = img.shape[1] if cols is None else int(cols)
        dst = np.zeros(ma.shape, np.uint16)
        self.check(self.fn("remap_nearest_u16")(*self._ctx_args(), _p(img, C.c_uint16), C.c_int32(img.shape[0]), C.c_int32(cols), C.c_int32(img.shape[1]),
                                                _p(mxy, C.c_int16), _p(ma, C.c_uint16), C.c_int32(ma.shape[0]), C.c_int32(ma.shape[1]), _p(dst, C.c_uint16)))
        return dst

    def harris_angle(self, image, xy):
        img = np.ascontiguousarray(image, np.uint8)
        pts = np.ascontiguousarray(xy, np.int16).reshape(-1, 2)
        resp, ang = np.zeros(pts.shape[0], np.float32), np.zeros(pts.shape[0], np.float32)
        self.check(self.fn("harris_angle")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                           C.c_int32(img.shape[1]), C.c_int32(pts.shape[0]), _p(pts, C.c_int16), _p(resp, C.c_float),
                                           _p(ang, C.c_float)))
        return resp, ang

    def orb_detect(self, image, nfeatures=5000, scale_factor=1.2, nlevels=8, edge_threshold=31, patch_size=31, fast_threshold=20, cap=20000,
                   row_stride=None):
        """cv::ORB::detect (HARRIS_SCORE): rows of (x, y, size, angle, response, octave).  row_stride: the image is a [rows, cols] uint8
        view into padded rows (row stride row_stride bytes, unit column stride) and is passed where it lies, as the RGB-D tracker passes
        a detector region; default: a dense copy, its own width."""
        if row_stride is None:
            img = np.ascontiguousarray(image, np.uint8)
            stride = img.shape[1]
        else:
            img, stride = np.asarray(image), int(row_stride)
            if img.dtype != np.uint8 or img.ndim != 2 or stride < img.shape[1] or (img.shape[1] > 1 and img.strides[1] != 1) or \
                    (img.shape[0] > 1 and img.strides[0] != stride):
                raise ValueError("orb_detect: with row_stride the image must be a [rows, cols] uint8 view whose rows lie row_stride bytes apart")
        out = np.zeros((cap, 6), np.float32)
        n = C.c_int32()
        self.check(self.fn("orb_detect")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                         C.c_int32(stride), C.c_int32(int(nfeatures)), C.c_float(float(scale_factor)), C.c_int32(int(nlevels)),
                                         C.c_int32(int(edge_threshold)), C.c_int32(int(patch_size)), C.c_int32(int(fast_threshold)),
                                         C.c_int32(cap), C.byref(n), _p(out, C.c_float)))
        return out[:n.value].copy()

    def gaussian_blur7_u8(self, image):
        img = np.ascontiguousarray(image, np.uint8)
        out = np.zeros_like(img)
        self.check(self.fn("gaussian_blur7_u8")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                                C.c_int32(img.shape[1]), _p(out, C.c_uint8)))
        return out

    def orb_describe(self, image, xy, angle_degrees=-1.0):
        """cv::ORB::create()->compute() at integer keypoints with one angle: (keep, descriptors)."""
        img = np.ascontiguousarray(image, np.uint8)
        pts = np.ascontiguousarray(xy, np.int16).reshape(-1, 2)
        n = pts.shape[0]
        keep = np.zeros(n, np.uint8)
        desc = np.zeros((n, 32), np.uint8)
        self.check(self.fn("orb_describe")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                           C.c_int32(img.shape[1]), C.c_int32(n), _p(pts, C.c_int16), C.c_float(float(angle_degrees)),
                                           _p(keep, C.c_uint8), _p(desc, C.c_uint8)))
        return keep, desc

    def orb_describe_keypoints(self, image, keypoints, scale_factor=1.2):
        """cv::ORB::create()->compute() on keypoints with octave and angle (rows of orb_detect): (keep, descriptors)."""
        img = np.ascontiguousarray(image, np.uint8)
        kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 6)
        n = kp.shape[0]
        keep = np.zeros(max(n, 1), np.uint8)
        desc = np.zeros((max(n, 1), 32), np.uint8)
        self.check(self.fn("orb_describe_keypoints")(*self._ctx_args(), _p(img, C.c_uint8), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]),
                                                     C.c_int32(img.shape[1]), C.c_int32(n), _p(kp, C.c_float), C.c_float(float(scale_factor)),
                                                     _p(keep, C.c_uint8), _p(desc, C.c_uint8)))
        return keep[:n], desc[:n]

    def point_in_camera(self, xy_previous, xy_current, T, K):
        xp = np.ascontiguousarray(xy_previous, np.float32).reshape(-1, 2)
        xc = np.ascontiguousarray(xy_current, np.float32).reshape(-1, 2)
        T = np.ascontiguousarray(T, np.float64).reshape(12); K = np.ascontiguousarray(K, np.float64).reshape(9)
        out = np.zeros((xp.shape[0], 3), np.float64)
        self.check(self.fn("point_in_camera")(*self._ctx_args(), C.c_int32(xp.shape[0]), _p(xp, C.c_float), _p(xc, C.c_float),
                                              _p(T, C.c_double), _p(K, C.c_double), _p(out, C.c_double)))
        return out

def _extra_methods():
    def copy_poses_device(self, first, count, dst_ptr):
        self.check(self.fn("copy_poses_device")(self.ctx, C.c_int32(first), C.c_int32(count), C.c_void_p(dst_ptr)))

    def copy_current_poses_device(self, dst_ptr):
        self.check(self.fn("copy_current_poses_device")(self.ctx, C.c_void_p(dst_ptr)))

    def enable_timers(self, on=True):
        self.check(self.fn("enable_timers")(self.ctx, C.c_int(1 if on else 0)))

    def kernel_times(self):
        ms = (C.c_double * 8)()
        n = (C.c_int32 * 8)()
        self.check(self.fn("get_kernel_times")(self.ctx, ms, n))
        names = ["k_fast_box", "k_emit", "k_brief", "k_track_candidates", "k_frame", "k_recover_brief",
                 "k_update_landmarks", "k_stereo_dist"]
        return {names[i]: (ms[i], n[i]) for i in range(8)}

    def timers(self):
        sec = (C.c_double * 8)()
        self.check(self.fn("get_timers")(self.ctx, sec))
        names = ["keypoint_detection", "descriptor_extraction", "point_triangulation", "tracking", "track_creation",
                 "pose_optimization", "landmark_optimization", "point_recovery"]
        return {names[i]: sec[i] for i in range(8)}

    def set_hip_stream(self, stream_ptr):
        self.check(self.fn("set_hip_stream")(self.ctx, C.c_void_p(stream_ptr)))

    for f in (copy_poses_device, copy_current_poses_device, enable_timers, kernel_times, timers, set_hip_stream):
        setattr(CApi, f.__name__, f)


_extra_methods()


class _RgbdMapApi(object):
    """vslam_rgbd_enable_map / _enable_observations and their getters (the device-resident loop only), shared by RgbdTracker and
    RgbdBatch: the dict keys of CApi.map / CApi.observations, with xy and cam in place of kp."""

    def enable_map(self, capacity_per_stream):
        """Keep every landmark of every sequence on the device (capacity_per_stream entries each); 0 turns map and log off."""
        self._check(self.lib.vslam_rgbd_enable_map(self.h, C.c_int32(int(capacity_per_stream))))

    def map_size(self, stream=0):
        n = C.c_int32()
        self._check(self.lib.vslam_rgbd_get_map_size(self.h, C.c_int32(stream), C.byref(n)))
        return n.value

    def map(self, stream=0, first=0):
        """Landmarks first .. of `stream`: dict of numpy arrays id, xyz [n, 3] (world), first_frame, last_frame, updates, desc [n, 32]."""
        cap = max(self.map_size(stream) - int(first), 0)
        n = C.c_int32()
        xyz = np.zeros((max(cap, 1), 3), np.float64)
        info = np.zeros((max(cap, 1), 3), np.int32)
        desc = np.zeros((max(cap, 1), 32), np.uint8)
        self._check(self.lib.vslam_rgbd_get_map(self.h, C.c_int32(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n), _p(xyz, C.c_double),
                                                _p(info, C.c_int32), _p(desc, C.c_uint8)))
        k = n.value
        return dict(id=np.arange(int(first), int(first) + k, dtype=np.int32), xyz=xyz[:k].copy(), first_frame=info[:k, 0].copy(),
                    last_frame=info[:k, 1].copy(), updates=info[:k, 2].copy(), desc=desc[:k].copy())

    def enable_map_colors(self, on=True):
        """Keep the colour of every map entry (the pixel of its point in the frame's colour image when the entry is written)."""
        self._check(self.lib.vslam_rgbd_enable_map_colors(self.h, C.c_int(1 if on else 0)))

    def map_colors(self, stream=0, first=0):
        """uint8 [n, 3] (r, g, b) of landmarks first .. of `stream`, in map() order."""
        cap = max(self.map_size(stream) - int(first), 0)
        n = C.c_int32()
        rgb = np.zeros((max(cap, 1), 3), np.uint8)
        self._check(self.lib.vslam_rgbd_get_map_colors(self.h, C.c_int32(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n), _p(rgb, C.c_uint8)))
        return rgb[:n.value].copy()

    def enable_observations(self, capacity_per_stream):
        """Log (landmark id, frame, keypoint, camera coordinates) of every point that carries a map id; needs the map; 0 turns it off."""
        self._check(self.lib.vslam_rgbd_enable_observations(self.h, C.c_int32(int(capacity_per_stream))))

    def observation_count(self, stream=0):
        n = C.c_int32()
        self._check(self.lib.vslam_rgbd_get_observation_count(self.h, C.c_int32(stream), C.byref(n)))
        return n.value

    def observations(self, stream=0, first=0):
        """Log entries first .. of `stream`: dict of numpy arrays id, frame (0-based per sequence), xy [n, 2] float32, cam [n, 3] float64."""
        cap = max(self.observation_count(stream) - int(first), 0)
        n = C.c_int32()
        idf = np.zeros((max(cap, 1), 2), np.int32)
        xy = np.zeros((max(cap, 1), 2), np.float32)
        cam = np.zeros((max(cap, 1), 3), np.float64)
        self._check(self.lib.vslam_rgbd_get_observations(self.h, C.c_int32(stream), C.c_int32(int(first)), C.c_int32(cap), C.byref(n),
                                                         _p(idf, C.c_int32), _p(xy, C.c_float), _p(cam, C.c_double)))
        k = n.value
        return dict(id=idf[:k, 0].copy(), frame=idf[:k, 1].copy(), xy=xy[:k].copy(), cam=cam[:k].copy())

    def point_ids(self, stream=0):
        """Map id (or -1) of every point of the finished frame, in points() order; needs the map only."""
        cap = int(self.cfg.max_points) * 4
        n = C.c_int32()
        ids = np.zeros(max(cap, 1), np.int32)
        self._check(self.lib.vslam_rgbd_get_point_ids(self.h, C.c_int32(stream), C.c_int32(cap), C.byref(n), _p(ids, C.c_int32)))
        return ids[:n.value].copy()


class _RgbdUndistortApi(object):
    """vslam_rgbd_set_undistortion / _get_undistorted (the device-resident loop only), shared by RgbdTracker and RgbdBatch."""

    def set_undistortion(self, und):
        """und: rectify.Undistortion (its maps at the tracker's rows x cols), or None to switch it off.  While set, process / submit take
        raw frames of und.raw_rows x und.raw_cols."""
        if und is None:
            self._check(self.lib.vslam_rgbd_set_undistortion(self.h, C.c_int32(0), C.c_int32(0), None, None))
            self._raw_size = None
            return
        if (und.rows, und.cols) != (self.cfg.rows, self.cfg.cols):
            raise ValueError("set_undistortion: maps are %dx%d, the tracker is %dx%d" % (und.rows, und.cols, self.cfg.rows, self.cfg.cols))
        mxy, ma = np.ascontiguousarray(und.map_xy, np.int16), np.ascontiguousarray(und.map_a, np.uint16)
        self._check(self.lib.vslam_rgbd_set_undistortion(self.h, C.c_int32(und.raw_rows), C.c_int32(und.raw_cols), _p(mxy, C.c_int16), _p(ma, C.c_uint16)))
        self._raw_size = (int(und.raw_rows), int(und.raw_cols))

    def undistorted(self, stream=0):
        """(image, depth) the last finished frame of `stream` was processed on."""
        rows, cols = int(self.cfg.rows), int(self.cfg.cols)
        img = np.zeros((rows, cols), np.uint8)
        dep = np.zeros((rows, cols), np.uint16)
        self._check(self.lib.vslam_rgbd_get_undistorted(self.h, C.c_int32(stream), _p(img, C.c_uint8), _p(dep, C.c_uint16)))
        return img, dep


class _RgbdEqualizeApi(object):
    """vslam_rgbd_set_equalization / _get_equalized (the device-resident loop only), shared by RgbdTracker and RgbdBatch."""

    def set_equalization(self, on=True):
        self._check(self.lib.vslam_rgbd_set_equalization(self.h, C.c_int(1 if on else 0)))

    def equalized(self, stream=0):
        """The equalised intensity image the last finished frame of `stream` was processed on."""
        img = np.zeros((int(self.cfg.rows), int(self.cfg.cols)), np.uint8)
        self._check(self.lib.vslam_rgbd_get_equalized(self.h, C.c_int32(stream), _p(img, C.c_uint8)))
        return img

    def set_clahe(self, on=True, clip_limit=40.0, tiles=(8, 8)):
        """vslam_rgbd_set_clahe: the slot's second mode, tiles = (tilesX, tilesY); equalized() returns the processed image while it is on."""
        self._check(self.lib.vslam_rgbd_set_clahe(self.h, C.c_int(1 if on else 0), C.c_double(clip_limit), C.c_int(int(tiles[0])), C.c_int(int(tiles[1]))))
        self._clahe_tiles = (int(tiles[0]), int(tiles[1])) if on else None

    def clahe_luts(self, stream=0):
        """uint8 [tilesY, tilesX, 256]: the tables of the image the last finished frame of `stream` was processed on."""
        return _clahe_luts(lambda buf: self._check(self.lib.vslam_rgbd_get_clahe_luts(self.h, C.c_int32(stream), _p(buf, C.c_uint8))), getattr(self, "_clahe_tiles", None), 1)[0]


class _RgbdBilateralApi(object):
    """vslam_rgbd_set_bilateral / _get_bilateral / _get_filtered_depth (the device-resident loop only), shared by RgbdTracker and RgbdBatch."""

    def set_bilateral(self, on=True, sigma_color=0.0, sigma_space=0.0):
        """The depth image's bilateral filter ahead of the space map; a sigma of 0 selects the reference's 2."""
        self._check(self.lib.vslam_rgbd_set_bilateral(self.h, C.c_int(1 if on else 0), C.c_double(sigma_color), C.c_double(sigma_space)))

    def get_bilateral(self):
        """(on, sigma_color, sigma_space) in force."""
        on, sc, ss = C.c_int(), C.c_double(), C.c_double()
        self._check(self.lib.vslam_rgbd_get_bilateral(self.h, C.byref(on), C.byref(sc), C.byref(ss)))
        return bool(on.value), sc.value, ss.value

    def filtered_depth(self, stream=0):
        """(depth uint16 [rows, cols], lut float32 [4098]) the last finished frame of `stream` was mapped from."""
        dep = np.zeros((int(self.cfg.rows), int(self.cfg.cols)), np.uint16)
        lut = np.zeros(4098, np.float32)
        self._check(self.lib.vslam_rgbd_get_filtered_depth(self.h, C.c_int32(stream), _p(dep, C.c_uint16), _p(lut, C.c_float)))
        return dep, lut


class _RgbdMaskApi(object):
    """vslam_rgbd_set_detection_mask / _get_detection_mask (the device-resident loop only), shared by RgbdTracker and RgbdBatch."""

    def set_detection_mask(self, mask_u8=None, margin=0):
        """The static detection mask of every sequence (2-D uint8 at the processed size, non-zero = keep; semantics: mask.py); None: off."""
        if mask_u8 is None:
            self._check(self.lib.vslam_rgbd_set_detection_mask(self.h, None, C.c_int32(0), C.c_int32(0)))
            return
        m = np.ascontiguousarray(mask_u8, np.uint8)
        if m.shape != (int(self.cfg.rows), int(self.cfg.cols)):
            raise ValueError("set_detection_mask: the mask is %s, the tracker works on %d x %d images" % (m.shape, self.cfg.rows, self.cfg.cols))
        self._check(self.lib.vslam_rgbd_set_detection_mask(self.h, _p(m, C.c_uint8), C.c_int32(m.shape[1]), C.c_int32(int(margin))))

    def detection_mask(self):
        """The context-wide packed keep-mask (static mask AND undistortion validity) the last finished frame used: uint64 [rows,
        (cols + 63) // 64] (mask.unpack)."""
        w = np.zeros((int(self.cfg.rows), (int(self.cfg.cols) + 63) // 64), np.uint64)
        self._check(self.lib.vslam_rgbd_get_detection_mask(self.h, _p(w, C.c_uint64)))
        return w

    def set_undistortion_mask(self, on=True, margin=0):
        """The undistortion maps' validity (rectify.validity, eroded by margin) as part of the context-wide keep-mask."""
        self._check(self.lib.vslam_rgbd_set_undistortion_mask(self.h, C.c_int(1 if on else 0), C.c_int32(int(margin))))

    def undistortion_mask(self):
        """(on, margin) in force."""
        on, m = C.c_int(), C.c_int32()
        self._check(self.lib.vslam_rgbd_get_undistortion_mask(self.h, C.byref(on), C.byref(m)))
        return bool(on.value), m.value

    def set_frame_masks(self, masks=None, margin=0):
        """The next frame's masks, one per sequence: uint8 [n_streams, rows, stride] (or [rows, stride] with one sequence), a numpy array
        (host, copied by the next submit) or a torch device tensor (read in place by that submit's pack launch; the caller keeps it as it
        is until wait() has returned).  None cancels a pending set."""
        n = int(getattr(self, "n", 1))
        if masks is None:
            self._check(self.lib.vslam_rgbd_set_frame_masks(self.h, None, C.c_int32(0), C.c_size_t(0), C.c_int32(0), C.c_int(0)))
            self._frame_masks_alive = None
            return
        if hasattr(masks, "data_ptr"):
            if str(masks.dtype) != "torch.uint8" or masks.stride(-1) != 1:
                raise ValueError("set_frame_masks: a uint8 tensor with unit column stride is required")
            shape, strides, addr, dev = tuple(masks.shape), tuple(masks.stride()), masks.data_ptr(), bool(masks.is_cuda)
        else:
            a = np.asarray(masks)
            if a.dtype != np.uint8 or a.ndim < 2 or (a.shape[-1] > 1 and a.strides[-1] != 1) or a.strides[-2] < a.shape[-1]:
                a = np.ascontiguousarray(masks, np.uint8)
            masks, shape, strides, addr, dev = a, a.shape, a.strides, a.ctypes.data, False
        if len(shape) == 2:
            shape, strides = (1,) + tuple(shape), (0,) + tuple(strides)
        if len(shape) != 3 or shape[0] != n or shape[1] != self.cfg.rows or shape[2] < self.cfg.cols:
            raise ValueError("set_frame_masks: expected %d x %d x >= %d, got %s" % (n, self.cfg.rows, self.cfg.cols, tuple(shape)))
        self._check(self.lib.vslam_rgbd_set_frame_masks(self.h, C.c_void_p(addr), C.c_int32(int(strides[1])), C.c_size_t(int(strides[0])),
                                                        C.c_int32(int(margin)), C.c_int(1 if dev else 0)))
        self._frame_masks_alive = masks

    def set_frame_mask(self, mask, margin=0):
        """set_frame_masks for a tracker of one sequence."""
        self.set_frame_masks(mask, margin)

    def frame_detection_mask(self, stream=0):
        """The effective packed keep-mask (static AND validity AND frame mask) the last finished frame of `stream` used: uint64 [rows,
        (cols + 63) // 64] (mask.unpack)."""
        w = np.zeros((int(self.cfg.rows), (int(self.cfg.cols) + 63) // 64), np.uint64)
        self._check(self.lib.vslam_rgbd_get_frame_detection_mask(self.h, C.c_int32(int(stream)), _p(w, C.c_uint64)))
        return w


class _RgbdColorApi(object):
    """vslam_rgbd_set_color_input / _get_gray (the device-resident loop only), shared by RgbdTracker and RgbdBatch.  While a colour format
    is set, process / submit take the intensity image as [rows, cols, channels] (a batch: [n_streams, rows, cols, channels])."""

    def set_color_input(self, fmt):
        self._check(self.lib.vslam_rgbd_set_color_input(self.h, C.c_int(int(fmt))))

    def gray(self, stream=0):
        """The grey image the last finished frame of `stream` was converted to, at the input size (the raw size while undistorting)."""
        rows, cols = getattr(self, "_full_size", None) or getattr(self, "_raw_size", None) or (int(self.cfg.rows), int(self.cfg.cols))
        img = np.zeros((rows, cols), np.uint8)
        self._check(self.lib.vslam_rgbd_get_gray(self.h, C.c_int32(stream), _p(img, C.c_uint8)))
        return img


class _RgbdDownscaleApi(object):
    """vslam_rgbd_set_downscale / _get_downscale / _get_downscaled (the device-resident loop only), shared by RgbdTracker and RgbdBatch.
    While the factor is not 1, process / submit take image and depth image of full_rows x full_cols."""

    def set_downscale(self, factor, full_rows=0, full_cols=0):
        self._check(self.lib.vslam_rgbd_set_downscale(self.h, C.c_int32(int(factor)), C.c_int32(int(full_rows)), C.c_int32(int(full_cols))))
        self._full_size = None if int(factor) == 1 else (int(full_rows), int(full_cols))

    def downscale(self):
        """(factor, full_rows, full_cols) in force; (1, 0, 0) while off."""
        f, r, c_ = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.vslam_rgbd_get_downscale(self.h, C.byref(f), C.byref(r), C.byref(c_)))
        return f.value, r.value, c_.value

    def downscaled(self, stream=0):
        """(image, depth) the last finished frame of `stream` was downscaled to (full // factor)."""
        f, r, c_ = self.downscale()
        rows, cols = (r // f, c_ // f) if f > 1 else (int(self.cfg.rows), int(self.cfg.cols))
        img = np.zeros((rows, cols), np.uint8)
        dep = np.zeros((rows, cols), np.uint16)
        self._check(self.lib.vslam_rgbd_get_downscaled(self.h, C.c_int32(stream), _p(img, C.c_uint8), _p(dep, C.c_uint16)))
        return img, dep


class _RgbdSmoothApi(object):
    """vslam_rgbd_set_smoothing / _get_smoothing / _get_smoothed (the device-resident loop only), shared by RgbdTracker and RgbdBatch."""

    def set_smoothing(self, mode, ksize=0):
        self._check(self.lib.vslam_rgbd_set_smoothing(self.h, C.c_int(int(mode)), C.c_int32(int(ksize))))

    def smoothing(self):
        """(mode, ksize) in force; (0, 0) while off."""
        m, k = C.c_int(), C.c_int32()
        self._check(self.lib.vslam_rgbd_get_smoothing(self.h, C.byref(m), C.byref(k)))
        return m.value, k.value

    def smoothed(self, stream=0):
        """The smoothed image of the last finished frame of `stream` (equalised in place afterwards while the slot is on)."""
        img = np.zeros((int(self.cfg.rows), int(self.cfg.cols)), np.uint8)
        self._check(self.lib.vslam_rgbd_get_smoothed(self.h, C.c_int32(stream), _p(img, C.c_uint8)))
        return img


class _RgbdMotionApi(object):
    """vslam_rgbd_set_motion_model / _set_pose_guess(es), shared by RgbdTracker and RgbdBatch (both loops)."""

    def set_motion_model(self, model, dead_reckoning_limit=0):
        self._check(self.lib.vslam_rgbd_set_motion_model(self.h, C.c_int(int(model)), C.c_int32(int(dead_reckoning_limit))))

    def motion_model(self):
        m, n = C.c_int(), C.c_int32()
        self._check(self.lib.vslam_rgbd_get_motion_model(self.h, C.byref(m), C.byref(n)))
        return m.value, n.value

    def set_pose_guess(self, T, stream=0):
        """The external camera_left_to_world (12 values row-major) of the sequence's next frame; kept until the next one is set."""
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        assert t.size == 12, t.shape
        self._check(self.lib.vslam_rgbd_set_pose_guess(self.h, C.c_int32(stream), _p(t, C.c_double)))

    def set_pose_guesses(self, T):
        """Those of all sequences, float64 [n_streams, 12]."""
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        assert t.size == 12 * getattr(self, "n", 1), t.shape
        self._check(self.lib.vslam_rgbd_set_pose_guesses(self.h, _p(t, C.c_double), C.c_int(0)))

    def set_pose_guesses_device(self, ptr):
        """ptr: device memory, float64 [n_streams][12], copied on the tracker's queue without a host synchronisation."""
        self._check(self.lib.vslam_rgbd_set_pose_guesses(self.h, C.c_void_p(ptr), C.c_int(1)))


def _row_bytes(left, image_ndim):
    """Row stride in bytes of a C-contiguous image array or batch: its trailing channel axis, when it has one, belongs to the row."""
    return int(left.shape[-1]) if left.ndim == image_ndim else int(left.shape[-2] * left.shape[-1])


class RgbdTracker(_RgbdMapApi, _RgbdUndistortApi, _RgbdEqualizeApi, _RgbdBilateralApi, _RgbdMaskApi, _RgbdColorApi, _RgbdDownscaleApi, _RgbdSmoothApi, _RgbdMotionApi):
    """ctypes view of vslam_rgbd_* (RGB-D mode end to end inside libvslam_hip.so: the device-resident loop, or the host-driven loop over the
    stand-alone entry points when VSLAM_RGBD_HOST=1 is set while the tracker is created)."""

    def __init__(self, api, cfg, params, device=0):
        self.lib = api.lib
        self.cfg = cfg.copy()
        self.lib.vslam_rgbd_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        rc = self.lib.vslam_rgbd_create(C.byref(cfg), C.byref(params), C.c_int(device), C.byref(self.h))
        if rc != OK:
            raise VslamError(rc, self.lib.vslam_rgbd_last_error(None).decode())

    def _check(self, rc):
        if rc != OK:
            raise VslamError(rc, self.lib.vslam_rgbd_last_error(self.h).decode())

    def reset(self):
        self._check(self.lib.vslam_rgbd_reset(self.h))

    def process(self, left, depth, cols=None):
        """left / depth: 2-D arrays; cols: image width when the arrays carry padding columns (row stride = array width)."""
        left = np.ascontiguousarray(left, np.uint8); depth = np.ascontiguousarray(depth, np.uint16)
        self._check(self.lib.vslam_rgbd_process_host(self.h, _p(left, C.c_uint8), C.c_int32(_row_bytes(left, 2)), _p(depth, C.c_uint16), C.c_int32(depth.shape[1])))
        fi = FrameInfo()
        nt = C.c_int32()
        self._check(self.lib.vslam_rgbd_get_frame_info(self.h, C.byref(fi), C.byref(nt)))
        return fi, nt.value

    def submit(self, left, depth):
        """First half of process(): copies the frame in and enqueues it.  The arrays are kept alive until wait()."""
        left = np.ascontiguousarray(left, np.uint8); depth = np.ascontiguousarray(depth, np.uint16)
        self._inflight = (left, depth)
        self._check(self.lib.vslam_rgbd_submit_host(self.h, _p(left, C.c_uint8), C.c_int32(_row_bytes(left, 2)), _p(depth, C.c_uint16), C.c_int32(depth.shape[1])))

    def wait(self):
        self._check(self.lib.vslam_rgbd_wait(self.h))
        self._inflight = None
        fi = FrameInfo()
        nt = C.c_int32()
        self._check(self.lib.vslam_rgbd_get_frame_info(self.h, C.byref(fi), C.byref(nt)))
        return fi, nt.value

    def points(self):
        cap = int(self.cfg.max_points) * 4
        n = C.c_int32()
        xy = np.zeros((cap, 2), np.float32); cam = np.zeros((cap, 3), np.float64); meta = np.zeros((cap, 4), np.int32); desc = np.zeros((cap, 32), np.uint8)
        self._check(self.lib.vslam_rgbd_get_points(self.h, C.c_int32(cap), C.byref(n), _p(xy, C.c_float), _p(cam, C.c_double), _p(meta, C.c_int32), _p(desc, C.c_uint8)))
        k = n.value
        return dict(xy=xy[:k].copy(), cam=cam[:k].copy(), meta=meta[:k].copy(), desc=desc[:k].copy())

    def destroy(self):
        if self.h:
            self.lib.vslam_rgbd_destroy(self.h)
            self.h = None


class RgbdBatch(_RgbdMapApi, _RgbdUndistortApi, _RgbdEqualizeApi, _RgbdBilateralApi, _RgbdMaskApi, _RgbdColorApi, _RgbdDownscaleApi, _RgbdSmoothApi, _RgbdMotionApi):
    """ctypes view of vslam_rgbd_create_batch / _process_batch_host: n_streams sequences of one camera and configuration in one context."""

    def __init__(self, api, cfg, params, n_streams, device=0):
        self.lib = api.lib
        self.cfg = cfg.copy()
        self.n = int(n_streams)
        self.lib.vslam_rgbd_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        rc = self.lib.vslam_rgbd_create_batch(C.byref(cfg), C.byref(params), C.c_int(device), C.c_int32(self.n), C.byref(self.h))
        if rc != OK:
            raise VslamError(rc, self.lib.vslam_rgbd_last_error(None).decode())

    def _check(self, rc):
        if rc != OK:
            raise VslamError(rc, self.lib.vslam_rgbd_last_error(self.h).decode())

    def reset(self):
        self._check(self.lib.vslam_rgbd_reset(self.h))

    def submit(self, left, depth):
        """left: [n_streams, rows, stride] uint8, depth: [n_streams, rows, stride] uint16 (kept alive until wait())."""
        left = np.ascontiguousarray(left, np.uint8); depth = np.ascontiguousarray(depth, np.uint16)
        assert left.shape[0] == self.n and depth.shape[0] == self.n
        self._inflight = (left, depth)
        self._check(self.lib.vslam_rgbd_submit_batch_host(self.h, _p(left, C.c_uint8), C.c_int32(_row_bytes(left, 3)), C.c_size_t(left.shape[1] * _row_bytes(left, 3)),
                                                          _p(depth, C.c_uint16), C.c_int32(depth.shape[2]), C.c_size_t(depth.shape[1] * depth.shape[2])))

    def submit_device(self, left_ptr, left_row_stride, left_stream_stride, depth_ptr, depth_row_stride, depth_stream_stride):
        """Images already in HBM: device addresses (e.g. torch tensors' data_ptr()), strides in bytes / depth in elements."""
        self._check(self.lib.vslam_rgbd_submit_batch_device(self.h, C.c_void_p(left_ptr), C.c_int32(left_row_stride), C.c_size_t(left_stream_stride),
                                                            C.c_void_p(depth_ptr), C.c_int32(depth_row_stride), C.c_size_t(depth_stream_stride)))

    def wait(self, infos=True):
        self._check(self.lib.vslam_rgbd_wait(self.h))
        self._inflight = None
        return [self.frame_info(s) for s in range(self.n)] if infos else None

    def process(self, left, depth):
        self.submit(left, depth)
        return self.wait()

    def frame_info(self, s):
        fi = FrameInfo()
        nt = C.c_int32()
        self._check(self.lib.vslam_rgbd_get_frame_info_stream(self.h, C.c_int32(s), C.byref(fi), C.byref(nt)))
        return fi, nt.value

    def points(self, s):
        cap = int(self.cfg.max_points) * 4
        n = C.c_int32()
        xy = np.zeros((cap, 2), np.float32); cam = np.zeros((cap, 3), np.float64); meta = np.zeros((cap, 4), np.int32); desc = np.zeros((cap, 32), np.uint8)
        self._check(self.lib.vslam_rgbd_get_points_stream(self.h, C.c_int32(s), C.c_int32(cap), C.byref(n), _p(xy, C.c_float), _p(cam, C.c_double), _p(meta, C.c_int32),
                                                          _p(desc, C.c_uint8)))
        k = n.value
        return dict(xy=xy[:k].copy(), cam=cam[:k].copy(), meta=meta[:k].copy(), desc=desc[:k].copy())

    def destroy(self):
        if self.h:
            self.lib.vslam_rgbd_destroy(self.h)
            self.h = None
