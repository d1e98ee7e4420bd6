"""Python host binding of libakaze_hip.so (the C ABI in include/akaze_hip.h).

Mirrors the reference crate's public interface for the hot path — same names, argument
meaning and error behaviour (the reference panics; here an AkazeError is raised):

    akaze::extract_features   (akaze/src/lib.rs:167-194)   -> extract_features()
    akaze::match_features     (akaze/src/lib.rs:252-275)   -> match_features()  (descriptor part)
    types::evolution::Config  (akaze/src/types/evolution.rs:8-55) -> Config
    pub mod ops / types::image                              -> ops.* on torch CUDA tensors

torch is used only as the owner of device memory and streams; all compute is in the HIP
library.  There is no CPU fallback: if libakaze_hip.so is missing or no gfx950 GPU is
visible, constructing a Context raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("AKAZE_HIP_LIB") or os.path.join(_PKG, "libakaze_hip.so")  # override: kernel tuning A/B builds

AKZ_KEEP_ALL_PLANES = 1
AKZ_NO_HOST_DESCRIPTORS = 2
AKZ_NO_DETECT = 4
AKZ_INPUT_READY = 8
AKZ_ERR_BUFFER = -7

PLANES = ["Lt", "Lsmooth", "Lx", "Ly", "Lxx", "Lyy", "Lxy", "Lflow", "Lstep", "Ldet"]

# akz_frame_format
FRAME_GRAY8, FRAME_RGB8, FRAME_BGR8, FRAME_RGBA8, FRAME_BGRA8, FRAME_RGB8_PLANAR = range(6)
KR_FRAME_LUMA = 12  # akz_kernel_row.kind of k_frame_luma (stage 10)
KR_MASK_CANDIDATES = 13  # ... of k_mask_candidates (stage 5, nms)


class AkazeError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"akaze_hip status {status}: {msg}")
        self.status = status


class Config(C.Structure):
    """types::evolution::Config (akaze/src/types/evolution.rs:8-38); Config() == Config::default()."""
    _fields_ = [
        ("num_sublevels", C.c_uint32),
        ("max_octave_evolution", C.c_uint32),
        ("base_scale_offset", C.c_double),
        ("initial_contrast", C.c_double),
        ("contrast_percentile", C.c_double),
        ("contrast_factor_num_bins", C.c_uint64),
        ("derivative_factor", C.c_double),
        ("detector_threshold", C.c_double),
        ("descriptor_channels", C.c_uint64),
        ("descriptor_pattern_size", C.c_uint64),
    ]

    def __init__(self, **kw):
        super().__init__()
        lib().akz_config_default(C.byref(self))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


STAGES = ["blur0", "contrast", "prep", "fed", "detector", "nms", "host_kp", "orient", "mldb", "total"]


class FrameLayout(C.Structure):
    """akz_frame_layout: frames as their producer holds them.  Strides in bytes; 0 = tight."""
    _fields_ = [("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("row_pitch", C.c_uint64),
                ("frame_stride", C.c_uint64), ("plane_stride", C.c_uint64)]


def frame_layout_of(shape, strides, layout="hwc", order="rgb"):
    """(FrameLayout, n, batched) of a uint8 array / tensor of `shape` whose `strides` are in bytes.  layout: "hw" ([N,]H,W:
    luma), "hwc" ([N,]H,W,C with C = 3 or 4: interleaved) or "chw" ([N,]3,H,W: planar R, G, B); order: "rgb" or "bgr"
    (interleaved only).  The innermost pixel must be dense; row, plane and frame strides are free as long as rows, planes and
    frames do not overlap.  ValueError names the stride the layout cannot express."""
    rank = {"hw": 2, "hwc": 3, "chw": 3}.get(layout)
    if rank is None:
        raise ValueError('layout must be "hw", "hwc" or "chw"')
    if order not in ("rgb", "bgr"):
        raise ValueError('order must be "rgb" or "bgr"')
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) not in (rank, rank + 1):
        raise ValueError(f'layout "{layout}" takes {rank} or {rank + 1} dimensions, got {len(shape)}')
    batched = len(shape) == rank + 1
    n, fstride = (shape[0], strides[0]) if batched else (1, 0)
    dims, st = shape[-rank:], strides[-rank:]
    if layout == "hw":
        (h, w), (sh, sw), c, sc, plane = dims, st, 1, 1, 0
        fmt = FRAME_GRAY8
    elif layout == "hwc":
        (h, w, c), (sh, sw, sc), plane = dims, st, 0
        if c not in (3, 4):
            raise ValueError(f"interleaved frames have 3 or 4 channels, got {c}")
        fmt = {(3, "rgb"): FRAME_RGB8, (3, "bgr"): FRAME_BGR8, (4, "rgb"): FRAME_RGBA8, (4, "bgr"): FRAME_BGRA8}[(c, order)]
    else:
        (c, h, w), (plane, sh, sw), sc = dims, st, 1
        if c != 3:
            raise ValueError(f"planar frames have 3 planes, got {c}")
        if order != "rgb":
            raise ValueError("planar frames are R, G, B planes (akz_frame_format has no planar BGR)")
        fmt, c = FRAME_RGB8_PLANAR, 1
    if n < 1 or h < 1 or w < 1:
        raise ValueError("empty frames")
    if layout == "hwc" and sc != 1:
        raise ValueError(f"channel stride {sc}: the channels of a pixel must be adjacent bytes")
    if w > 1 and sw != c:
        raise ValueError(f"pixel stride {sw}: the pixels of a row must be dense (stride {c})")
    tight_row = w * c
    if h > 1 and sh < tight_row:
        raise ValueError(f"row stride {sh} is smaller than a row ({tight_row} bytes)")
    row_pitch = sh if h > 1 else tight_row
    tight_plane = row_pitch * h
    if layout == "chw":
        if plane < tight_plane:
            raise ValueError(f"plane stride {plane} is smaller than a plane ({tight_plane} bytes)")
        tight_frame = 3 * plane
    else:
        tight_frame = tight_plane
    if n > 1 and fstride < tight_frame:
        raise ValueError(f"frame stride {fstride} is smaller than a frame ({tight_frame} bytes)")
    return FrameLayout(fmt, w, h, row_pitch, fstride if n > 1 else 0, plane), n, batched


class KernelRow(C.Structure):
    """akz_kernel_row (akaze_hip_debug.h)"""
    _fields_ = [("stage", C.c_uint32), ("kind", C.c_uint32), ("param", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("n", C.c_uint32), ("launches", C.c_uint64), ("px", C.c_uint64), ("px_steps", C.c_uint64), ("ms", C.c_double)]


KERNEL_ROW_KINDS = {1: "k_level_march", 2: "k_fed_own", 3: "k_octave_resident", 4: "k_detector_tiled", 5: "k_detector_march",
                    6: "k_jpeg_idct", 7: "k_jpeg_luma", 8: "jpeg_coef_h2d", 9: "k_sort_rows", 10: "k_bucket_sort", 11: "rocprim_radix_sort",
                    12: "k_frame_luma", 13: "k_mask_candidates", 14: "k_bank_gather", 15: "k_bank_select"}


class ScratchAudit(C.Structure):
    """akz_scratch_audit (akaze_hip_debug.h)"""
    _fields_ = [("name", C.c_char * 32), ("claimed_bytes", C.c_uint64), ("first_bad", C.c_int64)]


class Gate(C.Structure):
    """akz_gate (akaze_hip_debug.h)"""
    _fields_ = [("name", C.c_char_p), ("value", C.c_double), ("unit", C.c_char_p), ("meaning", C.c_char_p)]


def gates():
    """akz_debug_gates: the table of every size / host-thread gate (csrc/akz_gates.hpp) as a list of dicts; needs no GPU."""
    p, n = C.c_void_p(), C.c_uint64()
    _check(lib().akz_debug_gates(C.byref(p), C.byref(n)))
    rows = C.cast(p, C.POINTER(Gate))
    return [dict(name=rows[i].name.decode(), value=rows[i].value, unit=rows[i].unit.decode(), meaning=rows[i].meaning.decode())
            for i in range(n.value)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * 10), ("fed_launches", C.c_uint64), ("fed_px_steps", C.c_uint64),
                ("calls", C.c_uint64), ("pixels", C.c_uint64), ("det_launches", C.c_uint64), ("det_px", C.c_uint64), ("fused_px", C.c_uint64),
                ("placement_probed", C.c_uint32), ("placement_early_stages", C.c_uint32), ("placement_replaced", C.c_uint32),
                ("placement_shared", C.c_uint32), ("placement_retries", C.c_uint32), ("placement_reserved", C.c_uint32)]

    def as_dict(self):
        d = {k: self.ms[i] for i, k in enumerate(STAGES)}
        d.update(fed_launches=self.fed_launches, fed_px_steps=self.fed_px_steps, calls=self.calls,
                 pixels=self.pixels, det_launches=self.det_launches, det_px=self.det_px, fused_px=self.fused_px,
                 placement={"probed": bool(self.placement_probed), "early_stages_on": "copy stream" if self.placement_early_stages == 2 else "caller's stream",
                            "streams_replaced": self.placement_replaced, "streams_still_shared": self.placement_shared,
                            "measurements_repeated": self.placement_retries})
        return d


KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"),
     ("octave", "<u8"), ("class_id", "<u8"), ("angle", "<f4"), ("_pad", "<u4")])
MATCH_DTYPE = np.dtype([("index_0", "<u8"), ("index_1", "<u8"), ("distance", "<f8")])


class FeatureSet(C.Structure):
    """akz_feature_set: host keypoints and descriptors of one set (akz_match_features_pairs)."""
    _fields_ = [("keypoints", C.c_void_p), ("n_keypoints", C.c_uint64), ("descriptors", C.c_void_p),
                ("n_descriptors", C.c_uint64)]

BUDGET_STRONGEST, BUDGET_SPREAD = 0, 1  # AKZ_BUDGET_*


class KeypointBudget(C.Structure):
    """akz_keypoint_budget: at most max_keypoints of a set, the strongest (BUDGET_STRONGEST) or the best spread (BUDGET_SPREAD:
    adaptive non-maximal suppression, robust in (0, 1])."""
    _fields_ = [("max_keypoints", C.c_uint64), ("mode", C.c_uint32), ("robust", C.c_float)]


class RansacOptions(C.Structure):
    """akz_ransac_options: the options of the seeded RANSAC (remove_outliers_seeded, match_features_seeded(_pairs)).  A new
    object holds akz_ransac_options_default -- fundamental matrix, ratio 0.86, 1 000 trials, epsilon_inliers 0.02, confidence
    0.99, seed (42, 69), stream_base 0, no refit, no guided stage -- then the keyword arguments (seed: a pair)."""
    _fields_ = [("struct_size", C.c_uint32), ("model_kind", C.c_int32), ("lowes_ratio", C.c_double), ("max_trials", C.c_uint64),
                ("epsilon_inliers", C.c_float), ("refine_iterations", C.c_uint32), ("confidence", C.c_double),
                ("seed", C.c_uint64 * 2), ("stream_base", C.c_uint64), ("guided", C.c_int32), ("guided_radius", C.c_float),
                ("guided_lowes_ratio", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().akz_ransac_options_default(C.byref(self))
        for k, v in kw.items():
            if k == "seed":
                self.seed[0], self.seed[1] = v
            elif k not in dict(self._fields_):
                raise TypeError(f"no option {k!r}")
            else:
                setattr(self, k, v)

    def copy(self, **kw):
        o = RansacOptions()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(self))
        for k, v in kw.items():
            if k == "seed":
                o.seed[0], o.seed[1] = v
            else:
                setattr(o, k, v)
        return o


class Camera(C.Structure):
    """akz_camera: a pinhole in pixels, K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]; no skew, no distortion."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]

    def matrix(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])

    @classmethod
    def of(cls, k):
        """a Camera, (fx, fy, cx, cy) or a 3 x 3 K (its skew entry is not read) -> Camera"""
        if isinstance(k, cls):
            return k
        a = np.asarray(k, np.float64)
        return cls(a[0, 0], a[1, 1], a[0, 2], a[1, 2]) if a.shape == (3, 3) else cls(*[float(v) for v in a.reshape(4)])


class Pose(C.Structure):
    """akz_pose: the relative pose of a pair (x1 = R x0 + t, |t| = 1) with the statement's by-products.  found = 0: no pose --
    r, t and winner are zero."""
    _fields_ = [("r", C.c_float * 9), ("t", C.c_float * 3), ("sigma", C.c_float * 3), ("in_front", C.c_uint32 * 4),
                ("winner", C.c_uint32), ("found", C.c_int32)]

    @property
    def R(self):
        return np.ctypeslib.as_array(self.r).reshape(3, 3)

    @property
    def T(self):
        return np.ctypeslib.as_array(self.t)

    @property
    def singular_values(self):
        return np.ctypeslib.as_array(self.sigma)

    @property
    def counts(self):
        return np.ctypeslib.as_array(self.in_front)

    def words(self):
        """the record as 21 uint32 words (what the GPU call promises bit for bit)"""
        return np.frombuffer(bytes(self), np.uint32).copy()


class ResectionProblem(C.Structure):
    """akz_resection_problem: n 2D-3D correspondences (points 3 n floats, pixels 2 n floats) and their camera."""
    _fields_ = [("points", C.POINTER(C.c_float)), ("pixels", C.POINTER(C.c_float)), ("n", C.c_uint64), ("camera", Camera)]


class Resection(C.Structure):
    """akz_resection: the absolute pose of a camera against known points (x_cam = R X + t).  found = 0: no pose -- every field
    is zero."""
    _fields_ = [("r", C.c_float * 9), ("t", C.c_float * 3), ("sigma", C.c_float * 3), ("found", C.c_int32)]

    @property
    def R(self):
        return np.ctypeslib.as_array(self.r).reshape(3, 3)

    @property
    def T(self):
        return np.ctypeslib.as_array(self.t)

    @property
    def singular_values(self):
        return np.ctypeslib.as_array(self.sigma)

    def words(self):
        """the record as 16 uint32 words (what the GPU call promises bit for bit)"""
        return np.frombuffer(bytes(self), np.uint32).copy()


class _ResectionArgs:
    """The arguments of the resection calls, stated once: problems -- a list of (points [n, 3], pixels [n, 2], camera) -- as
    float32 arrays kept alive here and an akz_resection_problem array; the outputs `tail` = kept (uint32, room for every
    correspondence, problem p's at the sum of the sizes before it), n_kept, poses, iterations, trials_run (one per problem); and
    results(): per problem (kept indices, Resection, accepted fits, trials run)."""

    def __init__(self, problems):
        self.arrays = [(np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3)),
                        np.ascontiguousarray(np.asarray(pix, np.float32).reshape(-1, 2)), Camera.of(cam)) for pts, pix, cam in problems]
        for pts, pix, _ in self.arrays:
            if len(pts) != len(pix):
                raise ValueError(f"{len(pts)} points but {len(pix)} pixels")
        n = len(self.arrays)
        fp = C.POINTER(C.c_float)
        self.problems = (ResectionProblem * max(1, n))(*[ResectionProblem(pts.ctypes.data_as(fp), pix.ctypes.data_as(fp), len(pts), cam)
                                                        for pts, pix, cam in self.arrays])
        self.sizes = [len(pts) for pts, _, _ in self.arrays]
        self.kept = np.zeros(max(1, sum(self.sizes)), np.uint32)
        self.n_kept = np.zeros(max(1, n), np.uint64)
        self.poses = (Resection * max(1, n))()
        self.its = np.zeros(max(1, n), np.uint32)
        self.trials = np.zeros(max(1, n), np.uint64)

    def tail(self):
        """the output pointers in header order: kept, n_kept, poses, iterations, trials_run"""
        return (C.cast(self.kept.ctypes.data, C.c_void_p), self.n_kept.ctypes.data_as(C.POINTER(C.c_uint64)), C.cast(self.poses, C.c_void_p),
                self.its.ctypes.data_as(C.POINTER(C.c_uint32)), self.trials.ctypes.data_as(C.POINTER(C.c_uint64)))

    def results(self):
        res, off = [], 0
        for p, n in enumerate(self.sizes):
            res.append((self.kept[off:off + int(self.n_kept[p])].copy(), Resection.from_buffer_copy(self.poses[p]), int(self.its[p]),
                        int(self.trials[p])))
            off += n
        return res


def _match_name(model, refined, guided, pairs):
    """akz_match_features{,_homography,_fundamental}{,_refined}{,_guided}{,_pairs}; model: "", "_homography" or "_fundamental"."""
    return "akz_match_features" + model + "_refined" * bool(refined) + "_guided" * bool(guided) + "_pairs" * bool(pairs)


def _match_run(head, scalars, refine, guided, out, model, iterations):
    """The argument run of those eighteen functions, stated once -- for the ctypes types of lib()'s table and for the values of a
    call (_match_pair, _match_pairs) alike: the head (a pair's, _PairArgs, or the sets', _PairsArgs), then lowes_ratio,
    ransac_trials, ransac_epsilon_inliers, [refine_iterations], [guided_radius, guided_lowes_ratio], out, n_out, [model, found],
    [iterations].  A part in brackets is () where the function has none."""
    return (*head, *scalars, *refine, *guided, *out, *model, *iterations)


_lib = None


def lib():
    """Load libakaze_hip.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C akaze-rust_amd). There is no CPU fallback.")
    # torch bundles its own HIP runtime (libamdhip64.so.7).  Import it first so that this library's
    # NEEDED libamdhip64.so.7 binds to the copy torch already loaded: two HIP/HSA runtimes in one
    # process do not both see the GPU.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32, f64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
    pu32, pu64, pf64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    fp = C.POINTER(C.c_float)
    sig = {
        "akz_abi_version": ([], i32),
        "akz_last_error": ([], C.c_char_p),
        "akz_config_default": ([C.POINTER(Config)], None),
        "akz_ctx_create": ([i32, vp, C.POINTER(vp)], i32),
        "akz_ctx_destroy": ([vp], i32),
        "akz_stream_create": ([i32, C.POINTER(vp)], i32),
        "akz_stream_destroy": ([i32, vp], i32),
        "akz_ctx_synchronize": ([vp], i32),
        "akz_ctx_stream": ([vp], vp),
        "akz_device_malloc": ([vp, C.c_size_t, C.POINTER(vp)], i32),
        "akz_device_free": ([vp, vp], i32),
        "akz_memcpy_h2d": ([vp, vp, vp, C.c_size_t], i32),
        "akz_memcpy_d2h": ([vp, vp, vp, C.c_size_t], i32),
        "akz_fed_tau_by_process_time": ([f64, i32, f64, i32, pf64, u64, pu64], i32),
        "akz_gaussian_kernel": ([C.c_float, u64, fp], i32),
        "akz_scharr_kernels": ([u32, fp, fp], i32),
        "akz_plan_num_levels": ([u32, u32, C.POINTER(Config), pu64], i32),
        "akz_plan_level_info": ([u32, u32, C.POINTER(Config), u64, pf64, pf64, pu32, pu32, pu32, pu32, pu32, pu32,
                                 pu64, pf64, u64], i32),
        "akz_op_horizontal_filter": ([vp, vp, vp, u32, u32, u32, fp, u32], i32),
        "akz_op_vertical_filter": ([vp, vp, vp, u32, u32, u32, fp, u32], i32),
        "akz_op_gaussian_blur": ([vp, vp, vp, u32, u32, u32, C.c_float], i32),
        "akz_op_gaussian_blur_u8": ([vp, vp, vp, u32, u32, u32, C.c_float], i32),
        "akz_op_half_size": ([vp, vp, vp, u32, u32, u32], i32),
        "akz_op_scharr": ([vp, vp, vp, u32, u32, u32, i32, i32, u32], i32),
        "akz_debug_rcp_f64_to_f32": ([vp, vp, vp, u64], i32),
        "akz_debug_kernel_rows": ([vp, vp, u32, vp, i32], i32),
        "akz_debug_gates": ([C.POINTER(vp), pu64], i32),
        "akz_debug_device_libm": ([vp, C.POINTER(i32), C.POINTER(i32)], i32),
        "akz_debug_set_device_libm": ([vp, i32], i32),
        "akz_debug_libm_eval": ([vp, vp, vp, vp, u64, i32], i32),
        "akz_ctx_calibrate_gates": ([vp, pu64, pu64, C.POINTER(C.c_double)], i32),
        "akz_op_pm_g2": ([vp, vp, vp, vp, u32, u32, u32, vp], i32),
        "akz_op_contrast_factor": ([vp, vp, u32, u32, u32, f64, f64, u64, vp], i32),
        "akz_op_flow": ([vp, vp, vp, u32, u32, u32, vp, u32], i32),
        "akz_op_fed_steps": ([vp, vp, vp, vp, u32, u32, u32, pf64, u32], i32),
        "akz_op_detector_response": ([vp, vp, u32, vp, vp, vp, vp, vp, vp, u32, u32, u32], i32),
        "akz_extract_gray_u8": ([vp, vp, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_gray_f32": ([vp, vp, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_device_u8": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_device_f32": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_begin_device_u8": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_begin_device_f32": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_luma_from_frames_host": ([vp, C.POINTER(FrameLayout), u32, vp], i32),
        "akz_luma_from_frames_device": ([vp, vp, C.POINTER(FrameLayout), u32, vp], i32),
        "akz_extract_device_frames": ([vp, vp, C.POINTER(FrameLayout), u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_begin_device_frames": ([vp, vp, C.POINTER(FrameLayout), u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_device_frames_masked": ([vp, vp, C.POINTER(FrameLayout), u32, vp, C.POINTER(FrameLayout), u32, C.POINTER(Config), u32,
                                              C.POINTER(vp)], i32),
        "akz_extract_begin_device_frames_masked": ([vp, vp, C.POINTER(FrameLayout), u32, vp, C.POINTER(FrameLayout), u32, C.POINTER(Config),
                                                    u32, C.POINTER(vp)], i32),
        "akz_extract_gray_u8_masked": ([vp, vp, vp, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_debug_mask_candidates": ([vp, vp, u32, vp, vp, C.POINTER(FrameLayout), u32, u32, u32, C.POINTER(Config), u32, vp], i32),
        "akz_debug_mask_counts": ([vp, pu64], i32),
        "akz_extract_begin_host_u8": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_begin_host_f32": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_extract_finish": ([vp, C.POINTER(vp)], i32),
        "akz_extract_from_planes": ([vp, u32, u32, C.POINTER(Config), C.POINTER(vp), u64, u32, C.POINTER(vp)], i32),
        "akz_random_color": ([vp], i32),
        "akz_draw_circle": ([vp, u32, u32, C.c_float, C.c_float, vp, C.c_float], i32),
        "akz_draw_line": ([vp, u32, u32, C.c_float, C.c_float, C.c_float, C.c_float, vp, C.c_float], i32),
        "akz_job_abandon": ([vp], i32),
        "akz_result_free": ([vp], i32),
        "akz_result_num_images": ([vp, pu64], i32),
        "akz_result_counts": ([vp, u64, pu64, pu64, pu64], i32),
        "akz_result_keypoints": ([vp, u64, vp], i32),
        "akz_result_descriptors": ([vp, u64, vp], i32),
        "akz_result_device_descriptors": ([vp, u64, C.POINTER(vp), pu64], i32),
        "akz_result_contrast": ([vp, u64, pf64], i32),
        "akz_result_copy_device_descriptors": ([vp, vp, u64, pu64], i32),
        "akz_result_level_info": ([vp, u64, pf64, pf64, pu32, pu32, pu32, pu32, pu32, pu64, pf64, u64], i32),
        "akz_fetch_plane": ([vp, u64, u64, i32, vp, pu64], i32),
        "akz_fetch_pyramid": ([vp, u64, vp, u64, pu64], i32),
        "akz_result_device_plane": ([vp, u64, u64, i32, C.POINTER(vp)], i32),
        "akz_descriptor_match": ([vp, vp, u64, vp, u64, u64, u64, f64, vp, pu64], i32),
        "akz_descriptor_match_device": ([vp, vp, u64, vp, u64, u64, f64, vp, vp], i32),
        "akz_ctx_graph_probe": ([vp, vp, u32, u32, u32, C.POINTER(Config), u32, u32, pf64, pf64, pu64], i32),
        "akz_debug_march_bands": ([i32, u32, u32, u32, i32, C.POINTER(i32), u32, pu32], i32),
        "akz_ctx_set_lanes": ([vp, u32], i32),
        "akz_ctx_set_eager_finish": ([vp, i32], i32),
        "akz_fed_kernel_name": ([], C.c_char_p),
        "akz_ctx_set_host_threads": ([vp, u32], i32),
        "akz_debug_set_match_chunks": ([vp, u32, u32], i32),
        "akz_debug_set_host_sort": ([vp, i32], i32),
        "akz_debug_set_alloc_fill": ([vp, i32], i32),
        "akz_debug_audit_scratch": ([vp, vp, u32, pu32], i32),
        "akz_debug_resource_counts": ([pu64], i32),
        "akz_debug_set_select": ([vp, i32], i32),
        "akz_debug_select_info": ([vp, C.POINTER(C.c_int)], i32),
        "akz_debug_set_schedule": ([vp, i32, i32], i32),
        "akz_debug_detector_set_cells": ([i32, pu32, pu32, u32, u32, C.POINTER(i32), u32, C.POINTER(i32), pu32], i32),
        "akz_debug_stream_placement": ([vp, C.POINTER(i32)], i32),
        "akz_detector_kernel_name": ([], C.c_char_p),
        "akz_remove_outliers": ([vp, u64, vp, u64, vp, u64, u64, C.c_float, C.c_float, vp, pu64], i32),
        "akz_estimate_fundamental_matrix": ([vp, u64, vp, u64, vp, C.c_float, fp, C.POINTER(i32)], i32),
        "akz_debug_ransac_samples": ([u64, u64, u64, u64, pu64], i32),
        "akz_debug_ransac_samples_k": ([u64, u64, u64, u64, i32, pu64], i32),
        "akz_estimate_homography": ([vp, u64, vp, u64, vp, C.c_float, fp, C.POINTER(i32)], i32),
        "akz_remove_outliers_homography": ([vp, u64, vp, u64, vp, u64, u64, C.c_float, C.c_float, vp, pu64, fp, C.POINTER(i32)], i32),
        "akz_refine_homography": ([vp, u64, vp, u64, vp, u64, fp, C.c_float, C.c_uint32, vp, pu64, fp, C.POINTER(C.c_uint32)], i32),
        "akz_descriptor_match_guided_host": ([vp, u64, vp, u64, vp, u64, vp, u64, u64, i32, fp, C.c_float, u64, f64, vp, pu64], i32),
        "akz_descriptor_match_guided": ([vp, vp, u64, vp, u64, vp, u64, vp, u64, u64, i32, fp, C.c_float, u64, f64, vp, pu64], i32),
        "akz_descriptor_match_guided_pairs": ([vp, vp, u64, vp, u64, u64, i32, fp, C.c_float, u64, f64, vp, pu64], i32),
        "akz_remove_outliers_fundamental": ([vp, u64, vp, u64, vp, u64, u64, C.c_float, C.c_float, vp, pu64, fp, C.POINTER(i32)], i32),
        "akz_refine_fundamental_matrix": ([vp, u64, vp, u64, vp, u64, fp, C.c_float, C.c_uint32, vp, pu64, fp, C.POINTER(C.c_uint32)], i32),
        "akz_ransac_options_default": ([C.POINTER(RansacOptions)], None),
        "akz_draw_sample_seeded": ([u64, u64, u64, u64, u64, i32, pu64], i32),
        "akz_ransac_required_inliers": ([u64, i32, u64, f64, pu64], i32),
        "akz_remove_outliers_seeded": ([vp, u64, vp, u64, vp, u64, C.POINTER(RansacOptions), u64, vp, pu64, fp, C.POINTER(i32),
                                        C.POINTER(C.c_uint32), pu64], i32),
        "akz_estimate_fundamental_normalised": ([vp, u64, vp, u64, vp, fp, C.POINTER(i32)], i32),
        "akz_refine_fundamental_normalised": ([vp, u64, vp, u64, vp, u64, fp, C.c_float, C.c_uint32, vp, pu64, fp,
                                               C.POINTER(C.c_uint32)], i32),
        "akz_match_features_seeded_pairs": ([vp, vp, u64, vp, u64, u64, C.POINTER(RansacOptions), vp, pu64, fp, C.POINTER(i32),
                                             C.POINTER(C.c_uint32), pu64], i32),
        "akz_match_features_seeded_cross_pairs": ([vp, vp, u64, vp, u64, u64, C.POINTER(RansacOptions), vp, pu64, fp, C.POINTER(i32),
                                                   C.POINTER(C.c_uint32), pu64], i32),
        "akz_recover_pose_host": ([vp, u64, vp, u64, vp, u64, fp, C.POINTER(Camera), C.POINTER(Camera), vp, pu64, C.POINTER(Pose), fp], i32),
        "akz_match_features_seeded_pose_pairs": ([vp, vp, u64, vp, vp, u64, u64, C.POINTER(RansacOptions), i32, vp, pu64, fp,
                                                  C.POINTER(i32), C.POINTER(C.c_uint32), pu64, vp, fp], i32),
        "akz_estimate_resection": ([fp, fp, C.POINTER(Camera), C.POINTER(Resection), C.POINTER(i32)], i32),
        "akz_refine_resection": ([C.POINTER(ResectionProblem), C.POINTER(Resection), C.c_float, u32, vp, pu64, C.POINTER(Resection), pu32], i32),
        "akz_resection_seeded_host": ([C.POINTER(ResectionProblem), C.POINTER(RansacOptions), u64, vp, pu64, vp, pu32, pu64], i32),
        "akz_resection_seeded_problems": ([vp, C.POINTER(ResectionProblem), u64, C.POINTER(RansacOptions), vp, pu64, vp, pu32, pu64], i32),
        "akz_bank_create_from_results": ([vp, C.POINTER(vp), u64, C.POINTER(vp)], i32),
        "akz_bank_create_from_sets": ([vp, vp, u64, u64, C.POINTER(vp)], i32),
        "akz_bank_info": ([vp, pu64, pu64, pu64], i32),
        "akz_bank_set_info": ([vp, u64, pu64, pu64, pu64], i32),
        "akz_bank_device": ([vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)], i32),
        "akz_bank_free": ([vp], i32),
        "akz_match_features_seeded_bank_pairs": ([vp, vp, vp, u64, C.POINTER(RansacOptions), i32, vp, pu64, fp, C.POINTER(i32),
                                                  C.POINTER(C.c_uint32), pu64], i32),
        "akz_match_features_seeded_pose_bank_pairs": ([vp, vp, vp, vp, u64, C.POINTER(RansacOptions), i32, vp, pu64, fp, C.POINTER(i32),
                                                       C.POINTER(C.c_uint32), pu64, vp, fp], i32),
        "akz_debug_bank_gather": ([vp, vp, u64, u64, vp], i32),
        "akz_bank_create_from_results_budget": ([vp, C.POINTER(vp), u64, C.POINTER(KeypointBudget), C.POINTER(vp)], i32),
        "akz_bank_create_from_sets_budget": ([vp, vp, u64, u64, C.POINTER(KeypointBudget), C.POINTER(vp)], i32),
        "akz_bank_set_indices": ([vp, u64, pu64], i32),
        "akz_debug_bank_select": ([vp, vp, vp, vp, u64, pu64, pu64, pu32, u64, vp, vp, vp, vp], i32),
        "akz_descriptor_match_cross_host": ([vp, u64, vp, u64, u64, u64, f64, vp, pu64], i32),
        "akz_descriptor_match_cross": ([vp, vp, u64, vp, u64, u64, u64, f64, vp, pu64], i32),
        "akz_descriptor_match_cross_device": ([vp, vp, u64, vp, u64, u64, f64, vp, vp], i32),
        "akz_descriptor_match_knn_host": ([vp, u64, vp, u64, u64, u64, u64, vp, vp], i32),
        "akz_descriptor_match_knn": ([vp, vp, u64, vp, u64, u64, u64, u64, vp, vp], i32),
        "akz_descriptor_match_knn_device": ([vp, vp, u64, vp, u64, u64, u64, vp, vp], i32),
        "akz_debug_set_knn_chunks": ([vp, u32], i32),
        "akz_keypoint_budget_host": ([vp, u64, C.POINTER(KeypointBudget), vp, pu64, vp], i32),
        "akz_keypoint_budget_sets": ([vp, vp, u64, C.POINTER(KeypointBudget), vp, vp, vp], i32),
        "akz_debug_keypoint_budget_split": ([vp, i32, pf64], i32),
        "akz_debug_resection_split": ([vp, i32, pf64], i32),
        "akz_debug_keypoint_budget_tiles": ([pu32, pu32], i32),
        "akz_debug_match_pairs_split": ([vp, i32, pf64], i32),
        "akz_debug_match_tile_rows": ([C.POINTER(C.c_uint32)], i32),
        "akz_debug_match_seed_rows": ([u32, C.POINTER(C.c_uint32)], i32),
        "akz_write_features": ([C.c_char_p, vp, u64, vp, u64], i32),
        "akz_read_features": ([C.c_char_p, vp, vp, u64, u64, pu64, pu64, pu64], i32),
        "akz_write_matches": ([C.c_char_p, vp, u64], i32),
        "akz_read_matches": ([C.c_char_p, vp, u64, pu64], i32),
        "akz_host_select_keypoints": ([u32, u32, C.POINTER(Config), vp, u64, vp, u64, pu64, pu64], i32),
        "akz_result_describe_keypoints": ([vp, u64, vp, u64, i32, vp], i32),
        "akz_random_seed": ([u64, u64], i32),
        "akz_image_load": ([C.c_char_p, pu32, pu32, pu32, C.POINTER(vp)], i32),
        "akz_image_load_luma": ([C.c_char_p, pu32, pu32, C.POINTER(vp)], i32),
        "akz_image_load_rgb": ([C.c_char_p, pu32, pu32, C.POINTER(vp)], i32),
        "akz_image_free": ([vp], None),
        "akz_extract_features_file": ([vp, C.c_char_p, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_image_load_luma_device": ([vp, C.c_char_p, vp, u64, pu32, pu32], i32),
        "akz_extract_features_files": ([vp, C.POINTER(C.c_char_p), u64, C.POINTER(Config), u32, C.POINTER(vp)], i32),
        "akz_config_to_json": ([C.POINTER(Config), C.c_char_p, u64, pu64], i32),
        "akz_config_from_json": ([C.c_char_p, C.POINTER(Config)], i32),
        "akz_image_save_png": ([C.c_char_p, vp, u32, u32, u32], i32),
        "akz_image_save_plane_png": ([C.c_char_p, vp, u32, u32], i32),
        "akz_write_evolutions": ([vp, u64, C.c_char_p], i32),
        "akz_draw_keypoints": ([vp, u32, u32, vp, u64], i32),
        "akz_draw_matches": ([vp, u32, u32, vp, u32, u32, vp, u64, vp, u64, vp, u64, pu32, pu32, C.POINTER(vp)], i32),
        "akz_ctx_set_profiling": ([vp, i32], i32),
        "akz_ctx_set_fed_mode": ([vp, i32], i32),
        "akz_ctx_set_match_mode": ([vp, i32], i32),
        "akz_ctx_set_candidate_hint": ([vp, u32], i32),
        "akz_descriptor_match_sets_device": ([vp, vp, u64, vp, C.POINTER(u64), u64, u64, f64, vp, vp], i32),
        "akz_descriptor_match_sets_mutual_device": ([vp, vp, u64, vp, C.POINTER(u64), u64, u64, f64, vp, vp, vp, vp], i32),
        "akz_ctx_set_detector_mode": ([vp, i32], i32),
        "akz_ctx_set_prep_mode": ([vp, i32], i32),
        "akz_ctx_get_profile": ([vp, C.POINTER(Profile), i32], i32),
        "akz_ctx_get_profile2": ([vp, C.POINTER(Profile), u64, i32], i32),
        "akz_ctx_warmup": ([vp], i32),
        "akz_debug_placement_verdict": ([C.c_float, C.c_float, C.c_float, C.c_float], i32),
        "akz_synth_frame_u8": ([vp, u32, u32, u64, C.c_int32, C.c_int32], i32),
        "akz_comm_unique_id": ([vp], i32),
        "akz_comm_create": ([i32, vp, i32, i32, C.POINTER(vp)], i32),
        "akz_comm_create_external": ([i32, i32, i32, C.POINTER(vp)], i32),
        "akz_gather_blocks": ([vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)], i32),
        "akz_gather_deliver": ([vp, vp], i32),
        "akz_comm_destroy": ([vp], i32),
        "akz_comm_set_timeout": ([vp, f64], i32),
        "akz_comm_place_streams": ([vp, vp], i32),
        "akz_comm_info": ([vp, C.POINTER(i32), C.POINTER(i32)], i32),
        "akz_gather_descriptors": ([vp, vp, u64, C.POINTER(vp), pu64], i32),
        "akz_gather_begin": ([vp, C.POINTER(vp), u64, u64, C.POINTER(vp)], i32),
        "akz_gather_begin_rows": ([vp, vp, u64, u64, vp, C.POINTER(vp)], i32),
        "akz_gather_begin_image_rows": ([vp, vp, pu64, u64, u64, vp, C.POINTER(vp)], i32),
        "akz_pairs_plan": ([vp, C.POINTER(vp)], i32),
        "akz_pairs_lead_sets": ([vp, u64, pu64, u64, pu64], i32),
        "akz_gather_image_rows": ([vp, i32, pu64, u64, pu64], i32),
        "akz_match_all_pairs": ([vp, vp, u64, C.c_double, C.POINTER(vp)], i32),
        "akz_pairs_info": ([vp, pu64, pu64, pu64], i32),
        "akz_pairs_image_rows": ([vp, u64, pu64, C.POINTER(i32)], i32),
        "akz_pairs_holder": ([vp, u64, u64, C.POINTER(i32)], i32),
        "akz_pairs_matches": ([vp, u64, u64, vp, u64, pu64], i32),
        "akz_pairs_free": ([vp], i32),
        "akz_pairs_totals": ([vp, pu64, pu64, pu64], i32),
        "akz_gather_stream_wait": ([vp, vp], i32),
        "akz_gather_finish": ([vp, C.POINTER(vp), pu64, pu64, pu64], i32),
        "akz_gather_free": ([vp], i32),
    }
    # the eighteen akz_match_features* rows, from their parts (_match_run): one of two heads, the scalars, the outputs
    pair_head = (vp, vp, u64, vp, u64, vp, u64, vp, u64, u64)  # ctx, (keypoints, n, descriptors, n) of set 0, of set 1, desc_bytes
    sets_head = (vp, vp, u64, vp, u64, u64)                    # ctx, sets, n_sets, pairs, n_pairs, desc_bytes
    for model in ("", "_homography", "_fundamental"):
        for refined, guided in ((0, 0), (1, 0), (0, 1), (1, 1)) if model else ((0, 0),):
            for pairs in (0, 1):
                sig[_match_name(model, refined, guided, pairs)] = (list(_match_run(
                    sets_head if pairs else pair_head, (f64, u64, C.c_float), (u32,) * refined, (C.c_float, f64) * guided, (vp, pu64),
                    (fp, C.POINTER(i32)) if model else (), (pu32,) * refined)), i32)
    for name, (args, res) in sig.items():
        fn = getattr(L, name)  # AttributeError here == a symbol of include/akaze_hip.h is missing
        fn.argtypes = args
        fn.restype = res
    L._declared = sorted(sig)
    _lib = L
    return L


def mask_layout_of(mask, n, h, w):
    """(FrameLayout, n_masks) of a detection mask for n frames of h x w: a uint8 or bool array / torch tensor [H, W] (one mask for
    every frame) or [N, H, W], any row and frame strides, dense pixels -- frame_layout_of(..., "hw").  ValueError on another dtype
    or shape."""
    dtype = str(getattr(mask, "dtype", None)).replace("torch.", "")
    if dtype not in ("uint8", "bool"):
        raise ValueError(f"a mask must be uint8 or bool, got {dtype}")
    shape = tuple(int(v) for v in mask.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"a mask is [H, W] or [N, H, W], got {len(shape)} dimensions")
    if shape[-2:] != (h, w):
        raise ValueError(f"the mask is {shape[-1]} x {shape[-2]} but the frames are {w} x {h}")
    if len(shape) == 3 and shape[0] != n:
        raise ValueError(f"{shape[0]} masks for {n} frames (give one per frame, or one [H, W] mask for all)")
    strides = mask.stride() if callable(getattr(mask, "stride", None)) else mask.strides  # (both dtypes have one-byte elements)
    ml, n_masks, _ = frame_layout_of(shape, strides, "hw")
    return ml, n_masks


def debug_resource_counts():
    """akz_debug_resource_counts: what the library holds process-wide -> dict(device_blocks, device_bytes, pinned_blocks,
    pinned_bytes, events, streams)."""
    out = (C.c_uint64 * 6)()
    _check(lib().akz_debug_resource_counts(out))
    return dict(zip(("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams"), map(int, out)))


def _check(status):
    if status != 0:
        raise AkazeError(status, lib().akz_last_error().decode("utf-8", "replace"))


# ------------------------------------------------------------------------------------------
# host-side planning helpers (no GPU needed)
# ------------------------------------------------------------------------------------------
def fed_tau_by_process_time(T, M=1, tau_max=0.25, reordering=True):
    """ops::fed_tau::fed_tau_by_process_time (akaze/src/ops/fed_tau.rs:27-30)."""
    n = C.c_uint64()
    _check(lib().akz_fed_tau_by_process_time(T, M, tau_max, int(reordering), None, 0, C.byref(n)))
    out = np.zeros(n.value, np.float64)
    _check(lib().akz_fed_tau_by_process_time(T, M, tau_max, int(reordering),
                                             out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
    return out


def gaussian_kernel(sigma, kernel_size):
    out = np.zeros(kernel_size, np.float32)
    _check(lib().akz_gaussian_kernel(sigma, kernel_size, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def scharr_kernels(scale):
    n = 2 * scale + 1
    m, o = np.zeros(n, np.float32), np.zeros(n, np.float32)
    fp = C.POINTER(C.c_float)
    _check(lib().akz_scharr_kernels(scale, m.ctypes.data_as(fp), o.ctypes.data_as(fp)))
    return m, o


def plan_levels(w, h, cfg=None):
    """types::evolution::allocate_evolutions (akaze/src/types/evolution.rs:135-161) + level sizes."""
    cfg = cfg or Config()
    n = C.c_uint64()
    _check(lib().akz_plan_num_levels(w, h, C.byref(cfg), C.byref(n)))
    out = []
    for lvl in range(n.value):
        et, es = C.c_double(), C.c_double()
        o, s, ss, lw, lh, ds = (C.c_uint32() for _ in range(6))
        nt = C.c_uint64()
        tau = np.zeros(8192, np.float64)
        _check(lib().akz_plan_level_info(w, h, C.byref(cfg), lvl, C.byref(et), C.byref(es), C.byref(o), C.byref(s),
                                         C.byref(ss), C.byref(lw), C.byref(lh), C.byref(ds), C.byref(nt),
                                         tau.ctypes.data_as(C.POINTER(C.c_double)), len(tau)))
        out.append(dict(etime=et.value, esigma=es.value, octave=o.value, sublevel=s.value, sigma_size=ss.value,
                        w=lw.value, h=lh.value, det_sigma=ds.value, tau=tau[:nt.value].copy()))
    return out


CANDIDATE_DTYPE = np.dtype([("level", "<u4"), ("idx", "<u4"), ("v", "<f4"), ("xp", "<f4"), ("xm", "<f4"),
                            ("yp", "<f4"), ("ym", "<f4"), ("_pad", "<u4")])
# the same 32 bytes with the last word named for what the device's lists hold there: the image of the batch (akz_debug_mask_candidates)
CANDIDATE_IMG_DTYPE = np.dtype(CANDIDATE_DTYPE.descr[:-1] + [("img", "<u4")])


def host_select_keypoints(w, h, cfg, cands):
    """Host part of detect_keypoints (scale_space_extrema.rs:43-178) on NMS candidates; no GPU needed.
    Returns (keypoints without angle, number of extrema before the sub-pixel step)."""
    cands = np.ascontiguousarray(cands, CANDIDATE_DTYPE)
    out = np.zeros(max(1, len(cands)), KEYPOINT_DTYPE)
    n, ne = C.c_uint64(), C.c_uint64()
    _check(lib().akz_host_select_keypoints(w, h, C.byref(cfg), cands.ctypes.data_as(C.c_void_p), len(cands),
                                           out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), C.byref(ne)))
    return out[:n.value].copy(), ne.value


def synth_frame(w, h, frame_index=0, shift=(0, 0)):
    """Deterministic synthetic 8-bit luma frame; host utility."""
    out = np.empty((h, w), np.uint8)
    _check(lib().akz_synth_frame_u8(out.ctypes.data_as(C.c_void_p), w, h, frame_index, shift[0], shift[1]))
    return out


def _extract_flags(keep_all_planes, host_descriptors=True, input_ready=False):
    """the AKZ_* flags word of the extract calls"""
    return (AKZ_KEEP_ALL_PLANES if keep_all_planes else 0) | (0 if host_descriptors else AKZ_NO_HOST_DESCRIPTORS) | \
           (AKZ_INPUT_READY if input_ready else 0)


class _OneResult:
    """The outputs of a call over one pair or one match list -- out (room for `rows` records), n_out, a 9-float model, found,
    iterations -- and the slice and the reshape afterwards (tail: out, n_out; model_out: model, found)."""

    def __init__(self, rows):
        self.out = np.zeros(max(1, rows), MATCH_DTYPE)
        self.n, self.found, self.it = C.c_uint64(), C.c_int(), C.c_uint32()
        self.model = np.zeros(9, np.float32)
        self.tail = (self.out.ctypes.data_as(C.c_void_p), C.byref(self.n))
        self.model_out = (self.model.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self.found))

    def list(self):
        return self.out[:self.n.value].copy()

    def found_model(self):
        return self.model.reshape(3, 3) if self.found.value else None


class _PairArgs(_OneResult):
    """One pair of host sets (head: [keypoints_0, n,] descriptors_0, n, [keypoints_1, n,] descriptors_1, n, desc_bytes -- the
    keypoints unless only the descriptors are given), kept alive here.  A descriptor array has rows only if it is 2-D; desc_bytes
    is the width of the first one that has rows, else 61; two widths are refused.  null_empty: a side without rows goes as NULL."""

    def __init__(self, descriptors_0, descriptors_1, keypoints_0=None, keypoints_1=None, null_empty=False):
        if keypoints_0 is not None:
            self.k0 = np.ascontiguousarray(keypoints_0, KEYPOINT_DTYPE)
            self.k1 = np.ascontiguousarray(keypoints_1, KEYPOINT_DTYPE)
        self.d0 = np.ascontiguousarray(descriptors_0, np.uint8)
        self.d1 = np.ascontiguousarray(descriptors_1, np.uint8)
        self.n0 = len(self.d0) if self.d0.ndim == 2 else 0
        self.n1 = len(self.d1) if self.d1.ndim == 2 else 0
        if self.n0 and self.n1 and self.d0.shape[1] != self.d1.shape[1]:
            raise ValueError(f"descriptor lengths differ: {self.d0.shape[1]} and {self.d1.shape[1]} bytes")
        self.desc_bytes = self.d0.shape[1] if self.n0 else (self.d1.shape[1] if self.n1 else 61)
        side0 = (self.d0.ctypes.data_as(C.c_void_p) if self.n0 or not null_empty else None, self.n0)
        side1 = (self.d1.ctypes.data_as(C.c_void_p) if self.n1 or not null_empty else None, self.n1)
        if keypoints_0 is not None:
            side0 = (self.k0.ctypes.data_as(C.c_void_p), len(self.k0), *side0)
            side1 = (self.k1.ctypes.data_as(C.c_void_p), len(self.k1), *side1)
        self.head = (*side0, *side1, self.desc_bytes)
        super().__init__(self.n0)


class _MatchList(_OneResult):
    """What the host calls over (keypoints_0, keypoints_1, matches) share (head: keypoints_0, n, keypoints_1, n, matches,
    n_matches[, the model given]), kept alive here."""

    def __init__(self, keypoints_0, keypoints_1, matches, model=None):
        self.k0 = np.ascontiguousarray(keypoints_0, KEYPOINT_DTYPE)
        self.k1 = np.ascontiguousarray(keypoints_1, KEYPOINT_DTYPE)
        self.m = np.ascontiguousarray(matches, MATCH_DTYPE)
        self.head = (self.k0.ctypes.data_as(C.c_void_p), len(self.k0), self.k1.ctypes.data_as(C.c_void_p), len(self.k1),
                     self.m.ctypes.data_as(C.c_void_p), len(self.m))
        if model is not None:
            self.model_in = np.ascontiguousarray(np.asarray(model, np.float32).reshape(9))
            self.head += (self.model_in.ctypes.data_as(C.POINTER(C.c_float)),)
        super().__init__(len(self.m))


def _pack_sets(features, keypoints_only=False):
    """A sequence of (keypoints, descriptors) host sets as an akz_feature_set array -> (the array, the arrays it points into
    (keypoints, descriptors), the descriptor rows of every set, desc_bytes).  keypoints_only (akz_keypoint_budget_sets): a set may
    be a bare keypoint array, and no descriptor is read."""
    if keypoints_only:
        ks = [np.ascontiguousarray(f[0] if isinstance(f, (tuple, list)) else f, KEYPOINT_DTYPE) for f in features]
        ds, rows, nb = [None] * len(ks), [0] * len(ks), 61
    else:
        ks = [np.ascontiguousarray(k, KEYPOINT_DTYPE) for k, _ in features]
        ds = [np.ascontiguousarray(d, np.uint8) for _, d in features]
        nbs = {d.shape[1] for d in ds if d.ndim == 2 and len(d)}
        if len(nbs) > 1:
            raise ValueError(f"descriptor lengths differ: {sorted(nbs)} bytes")
        nb = nbs.pop() if nbs else 61
        rows = [len(d) if d.ndim == 2 else 0 for d in ds]
    sets = (FeatureSet * max(1, len(ks)))()
    for i, (k, d, nd) in enumerate(zip(ks, ds, rows)):
        sets[i] = FeatureSet(k.ctypes.data_as(C.c_void_p) if len(k) else None, len(k), d.ctypes.data_as(C.c_void_p) if nd else None, nd)
    return sets, (ks, ds), rows, nb


class _PairsArgs:
    """What the pairs calls share: the akz_feature_set array, the pair list and the outputs (head: ctx, sets, n_sets, pairs,
    n_pairs, desc_bytes; tail: out, n_out), and the split of `out` into one list per pair afterwards."""

    def __init__(self, ctx, features, pairs, bank_ok=False):
        self.bank = features if isinstance(features, FeatureBank) else None
        if self.bank is not None and not bank_ok:
            raise TypeError("this call takes host feature sets; a FeatureBank goes to the seeded pairs calls")
        if self.bank is not None and self.bank.ctx is not ctx:
            raise ValueError("the FeatureBank belongs to another context")
        if self.bank is not None:  # (head: ctx, bank, pairs, n_pairs -- the sets stay where they are)
            info = self.bank.info()
            self.n_sets = info["n_sets"]
            self.pr = np.ascontiguousarray(np.asarray(pairs, np.uint64).reshape(-1, 2))
            # (an index beyond the bank is the library's to refuse: it gets no room here)
            self.rows = [info["sets"][int(a)]["n_descriptors"] if int(a) < self.n_sets else 0 for a in self.pr[:, 0]]
            self.out = np.zeros(max(1, sum(self.rows)), MATCH_DTYPE)
            self.n = np.zeros(max(1, len(self.pr)), np.uint64)
            self.head = (ctx._h, self.bank._h, self.pr.ctypes.data_as(C.c_void_p), len(self.pr))
            self.tail = (self.out.ctypes.data_as(C.c_void_p), self.n.ctypes.data_as(C.POINTER(C.c_uint64)))
            return
        if isinstance(features, (str, bytes)) or not hasattr(features, "__iter__"):
            raise TypeError(f"features must be a FeatureBank or a sequence of (keypoints, descriptors), got {type(features).__name__}")
        self.sets, self.keep, set_rows, nb = _pack_sets(features)
        self.pr = np.ascontiguousarray(np.asarray(pairs, np.uint64).reshape(-1, 2))
        if len(set_rows) == 0 and len(self.pr):
            raise IndexError("pair refers to a set that does not exist")
        self.rows = [set_rows[int(a)] for a in self.pr[:, 0]] if len(set_rows) else []
        self.n_sets = len(set_rows)
        self.out = np.zeros(max(1, sum(self.rows)), MATCH_DTYPE)
        self.n = np.zeros(max(1, len(self.pr)), np.uint64)
        self.head = (ctx._h, C.cast(self.sets, C.c_void_p), self.n_sets, self.pr.ctypes.data_as(C.c_void_p), len(self.pr), nb)
        self.tail = (self.out.ctypes.data_as(C.c_void_p), self.n.ctypes.data_as(C.POINTER(C.c_uint64)))

    def models(self):
        self.h = np.zeros((max(1, len(self.pr)), 9), np.float32)
        self.found = np.zeros(max(1, len(self.pr)), np.int32)
        return self.h.ctypes.data_as(C.POINTER(C.c_float)), self.found.ctypes.data_as(C.POINTER(C.c_int32))

    def lists(self):
        res, at = [], 0
        for p, r in enumerate(self.rows):
            res.append(self.out[at:at + int(self.n[p])].copy())
            at += r
        return res

    def lists_and_models(self):
        return [(m, self.h[p].reshape(3, 3).copy() if self.found[p] else None) for p, m in enumerate(self.lists())]

    def iterations(self):
        self.it = np.zeros(max(1, len(self.pr)), np.uint32)
        return self.it.ctypes.data_as(C.POINTER(C.c_uint32))

    def refined(self):
        return (*self.models(), self.iterations())

    def lists_models_iterations(self):
        return [(m, h, int(self.it[p])) for p, (m, h) in enumerate(self.lists_and_models())]


def _match_pairs(ctx, model, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations=None, guided=None):
    """The nine Context.match_features*_pairs calls: akz_match_features{model}[_refined][_guided]_pairs (_match_name) -- _refined
    with refine_iterations, _guided with guided = (guided_radius, guided_lowes_ratio).  One list per pair for model "", else one
    (list, model or None) per pair, with refine_iterations one (list, model or None, accepted fits)."""
    a = _PairsArgs(ctx, features, pairs)
    refined = refine_iterations is not None
    fn = getattr(lib(), _match_name(model, refined, guided, True))
    _check(fn(*_match_run(a.head, (lowes_ratio, ransac_trials, ransac_epsilon_inliers), (refine_iterations,) if refined else (),
                          guided or (), a.tail, a.models() if model else (), (a.iterations(),) if refined else ())))
    return a.lists_models_iterations() if refined else a.lists_and_models() if model else a.lists()


# ------------------------------------------------------------------------------------------
# GPU context
# ------------------------------------------------------------------------------------------
class Context:
    """One GPU + one HIP stream.  Not thread-safe; one per host thread / per rank."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        _check(lib().akz_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = int(device)

    def close(self):
        if self._h:
            lib().akz_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().akz_ctx_synchronize(self._h))

    @property
    def stream(self):
        return lib().akz_ctx_stream(self._h)

    def set_fed_mode(self, mode):
        """2 = k_fed_own, temporally fused (default), 0 = k_fed_step, one launch per step."""
        _check(lib().akz_ctx_set_fed_mode(self._h, int(mode)))

    def set_candidate_hint(self, per_image):
        """Room for extrema candidates per image in the next extraction (a list that overflows is enlarged and the
        extrema pass repeated by finish: same results)."""
        _check(lib().akz_ctx_set_candidate_hint(self._h, int(per_image)))

    def set_lanes(self, lanes):
        """Deal jobs below 2.4 Mpx to `lanes` child contexts in turn (1 = off): the launch chains of consecutive single
        frames then overlap on the chip."""
        _check(lib().akz_ctx_set_lanes(self._h, int(lanes)))

    def set_eager_finish(self, on=True):
        """With lanes: the finish half of every job dealt to a lane starts on that lane's own thread as soon as the job
        has been begun; `finish()` then only collects the result (same results)."""
        _check(lib().akz_ctx_set_eager_finish(self._h, 1 if on else 0))

    def debug_set_select(self, mode):
        """akz_debug_set_select: keypoint selection on the device (2), on the host from the device's neighbour lists (1 / True),
        from the host's grids (0 / False), automatic (None)."""
        _check(lib().akz_debug_set_select(self._h, -1 if mode is None else (2 if mode == 2 and mode is not True else (1 if mode else 0))))

    def debug_set_schedule(self, key, value):
        """akz_debug_set_schedule: schedule variants of a large batch (measurement hook, identical results)."""
        _check(lib().akz_debug_set_schedule(self._h, int(key), int(value)))

    def debug_stream_placement(self):
        """akz_debug_stream_placement: what the context's stream-placement probe found."""
        info = (C.c_int32 * 4)()
        _check(lib().akz_debug_stream_placement(self._h, info))
        return {"probed": bool(info[0]), "early_stages": ("context stream", "own stream", "copy stream")[info[1]],
                "streams_replaced": int(info[2]), "streams_sharing_a_queue": int(info[3])}

    def set_match_mode(self, mode):
        """2 = automatic (default), 1 = matrix-core matcher, 0 = popcount matcher."""
        _check(lib().akz_ctx_set_match_mode(self._h, int(mode)))

    def set_detector_mode(self, mode):
        """2 = automatic (default: column march for large launches, one LDS-tiled kernel for small ones), 5 = column
        march, 4 = one LDS-tiled kernel, 0 = LDS-tiled kernel pair."""
        _check(lib().akz_ctx_set_detector_mode(self._h, int(mode)))

    def set_prep_mode(self, mode):
        """Level preparation: 2 = automatic (default: fused with the first diffusion steps for large launches), 3 = fused
        wherever supported, 1 = streaming kernel, 0 = LDS-tiled kernel."""
        _check(lib().akz_ctx_set_prep_mode(self._h, int(mode)))

    def warmup(self):
        """akz_ctx_warmup: the stream-placement probe now (idle streams, no capture) instead of inside the first large batch."""
        _check(lib().akz_ctx_warmup(self._h))

    def set_profiling(self, on=True):
        """0/False off, 1/True every stage, 2 light (FED spans + host-clock stages only)."""
        _check(lib().akz_ctx_set_profiling(self._h, int(on)))

    def get_profile(self, reset=True):
        p = Profile()
        _check(lib().akz_ctx_get_profile2(self._h, C.byref(p), C.sizeof(Profile), int(reset)))
        return p.as_dict()

    def debug_device_libm(self):
        """akz_debug_device_libm -> (available, last_job): 0 = the host's libm, 1 / 2 = the device's FMA / SSE2 forms of glibc's
        atan2f / cosf / sinf (csrc/akz_libm.hpp), proven equal to this process's libm by a self-test."""
        a, b = C.c_int32(), C.c_int32()
        _check(lib().akz_debug_device_libm(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_set_device_libm(self, on):
        """False: angles and their cosines / sines always from the host's libm; True / None: automatic."""
        _check(lib().akz_debug_set_device_libm(self._h, 0 if on is False else -1))

    def debug_libm_eval(self, a, b, fma=True):
        """(atan2f(a, b), cosf(a), sinf(a)) per element as the device forms them: torch CUDA float32 tensors -> [n, 3]"""
        import torch
        out = torch.empty((a.numel(), 3), dtype=torch.float32, device=a.device)
        _check(lib().akz_debug_libm_eval(self._h, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), int(bool(fma))))
        return out

    def calibrate_gates(self):
        """akz_ctx_calibrate_gates: the two job gates from timings on this machine -> (sync_px, async_px, ms[5][4])"""
        a, b = C.c_uint64(), C.c_uint64()
        ms = (C.c_double * 20)()
        _check(lib().akz_ctx_calibrate_gates(self._h, C.byref(a), C.byref(b), ms))
        return a.value, b.value, [[ms[i * 4 + k] for k in range(4)] for i in range(5)]

    def kernel_rows(self, reset=True):
        """akz_debug_kernel_rows: the FED / detector spans by kernel variant and launch shape (profiling must be on)."""
        n = C.c_uint32()
        rows = (KernelRow * 256)()
        _check(lib().akz_debug_kernel_rows(self._h, C.cast(rows, C.c_void_p), 256, C.cast(C.pointer(n), C.c_void_p), int(reset)))
        out = []
        for r in rows[:min(n.value, 256)]:
            if r.launches == 0:
                continue
            name = KERNEL_ROW_KINDS.get(r.kind, str(r.kind))
            if r.kind == 1:
                name += f"<{r.param & 15}{', Lstep' if r.param & 32 else ''}{', HALF' if r.param & 16 else ''}>"
            elif r.kind in (4, 5):
                name += f"<{r.param}>"
            out.append(dict(kernel=name, kind=r.kind, param=r.param, w=r.w, h=r.h, n=r.n, launches=int(r.launches), px=int(r.px),
                            px_steps=int(r.px_steps), ms=float(r.ms)))
        return out

    def set_host_threads(self, threads):
        """akz_ctx_set_host_threads: host threads of the finish half (0 = automatic)."""
        _check(lib().akz_ctx_set_host_threads(self._h, int(threads)))

    def debug_select_info(self):
        """akz_debug_select_info: (where the last job's selection ran: 0 grids / 1 lists / 2 device, most rounds of an image,
        images that fell back to the host, candidates)."""
        info = (C.c_int * 8)()
        _check(lib().akz_debug_select_info(self._h, info))
        return tuple(info)

    def debug_set_host_sort(self, on):
        """akz_debug_set_host_sort: candidates bucketed and sorted on the host instead of the device sort."""
        _check(lib().akz_debug_set_host_sort(self._h, -1 if on is None else (1 if on else 0)))

    def debug_set_alloc_fill(self, on=True):
        """akz_debug_set_alloc_fill: every device allocation of the context from now on is filled with 0xA5 bytes (identical results)."""
        _check(lib().akz_debug_set_alloc_fill(self._h, int(bool(on))))

    def debug_audit_scratch(self):
        """akz_debug_audit_scratch: every raised scratch claim checked on the device -> [dict(name, claimed_bytes, first_bad)],
        first_bad None where the claimed range holds what the claim says (or nothing is claimed)."""
        n = C.c_uint32()
        rows = (ScratchAudit * 32)()
        _check(lib().akz_debug_audit_scratch(self._h, C.cast(rows, C.c_void_p), 32, C.byref(n)))
        return [dict(name=r.name.decode(), claimed_bytes=int(r.claimed_bytes), first_bad=None if r.first_bad < 0 else int(r.first_bad))
                for r in rows[:min(n.value, 32)]]

    def debug_set_match_chunks(self, pair_chunks=0, set_chunks=0):
        """akz_debug_set_match_chunks (include/akaze_hip_debug.h): force the matcher's chunk counts; 0 = automatic."""
        _check(lib().akz_debug_set_match_chunks(self._h, int(pair_chunks), int(set_chunks)))

    def graph_probe(self, frames, options=None, keep_all_planes=True, reps=50):
        """akz_ctx_graph_probe: (ms per hipGraph launch of the begin phase, ms per plain enqueue of it, graph nodes)."""
        options = options or Config()
        t = frames if frames.dim() == 3 else frames.unsqueeze(0)
        n, h, w = t.shape
        g, p, nodes = C.c_double(), C.c_double(), C.c_uint64()
        _check(lib().akz_ctx_graph_probe(self._h, C.c_void_p(t.data_ptr()), w, h, n, C.byref(options),
                                         AKZ_KEEP_ALL_PLANES if keep_all_planes else 0, reps, C.byref(g), C.byref(p),
                                         C.byref(nodes)))
        return g.value, p.value, nodes.value

    # ---- the hot path --------------------------------------------------------------------
    def extract_features(self, image, options=None, keep_all_planes=True, host_descriptors=True):
        """akaze::extract_features on an in-memory luma image (2-D uint8 or float32 numpy array, or a
        torch CUDA tensor of shape [H, W] or [N, H, W]).  Returns an ExtractResult."""
        options = options or Config()
        flags = _extract_flags(keep_all_planes, host_descriptors)
        res = C.c_void_p()
        L = lib()
        if isinstance(image, np.ndarray):
            img = np.ascontiguousarray(image)
            if img.ndim != 2:
                raise ValueError("host images must be 2-D (one luma plane)")
            h, w = img.shape
            if img.dtype == np.uint8:
                _check(L.akz_extract_gray_u8(self._h, img.ctypes.data_as(C.c_void_p), w, h, C.byref(options), flags,
                                             C.byref(res)))
            else:
                img = img.astype(np.float32, copy=False)
                _check(L.akz_extract_gray_f32(self._h, img.ctypes.data_as(C.c_void_p), w, h, C.byref(options), flags,
                                              C.byref(res)))
        else:  # torch CUDA tensor
            import torch
            t = image
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
                raise ValueError("device images must be contiguous torch CUDA tensors")
            if t.dim() == 2:
                t = t.unsqueeze(0)
            n, h, w = t.shape
            if t.dtype == torch.uint8:
                fn = L.akz_extract_device_u8
            elif t.dtype == torch.float32:
                fn = L.akz_extract_device_f32
            else:
                raise ValueError("uint8 or float32 images only")
            _check(fn(self._h, C.c_void_p(t.data_ptr()), w, h, n, C.byref(options), flags, C.byref(res)))
        return ExtractResult(self, res)

    def extract_features_file(self, path, options=None, keep_all_planes=True):
        """akaze::extract_features(input_image_path, options) — akaze/src/lib.rs:167-194."""
        cfg = options or Config()
        res = C.c_void_p()
        _check(lib().akz_extract_features_file(self._h, os.fsencode(path), C.byref(cfg), _extract_flags(keep_all_planes), C.byref(res)))
        return ExtractResult(self, res)

    def extract_features_files(self, paths, options=None, keep_all_planes=True):
        """akz_extract_features_files: one batch job over files of one size (image i of the result = paths[i])."""
        cfg = options or Config()
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        res = C.c_void_p()
        _check(lib().akz_extract_features_files(self._h, arr, len(paths), C.byref(cfg), _extract_flags(keep_all_planes), C.byref(res)))
        return ExtractResult(self, res)

    def load_luma_device(self, path):
        """akz_image_load_luma_device: load_image_luma(path) as a (h, w) uint8 torch CUDA tensor (a JPEG is reconstructed
        on the device)."""
        import torch
        w, h = C.c_uint32(), C.c_uint32()
        st = lib().akz_image_load_luma_device(self._h, os.fsencode(path), None, 0, C.byref(w), C.byref(h))
        if st != AKZ_ERR_BUFFER:
            _check(st)
        out = torch.empty((h.value, w.value), dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.current_stream(out.device).synchronize()  # (the allocation is ordered on torch's stream, the work on ours)
        _check(lib().akz_image_load_luma_device(self._h, os.fsencode(path), C.c_void_p(out.data_ptr()), out.numel(),
                                                C.byref(w), C.byref(h)))
        return out

    def extract_from_planes(self, w, h, planes, options=None, detect=True):
        """ops::scale_space_extrema::detect_keypoints / ops::descriptors::extract_descriptors on evolutions the caller
        holds: planes[level][name] -> 2-D float32 array (names of PLANES; missing ones are skipped; Lt, Lx, Ly and —
        for detection — Ldet are required).  Returns an ExtractResult."""
        options = options or Config()
        n = len(planes)
        keep = []
        tab = (C.c_void_p * (n * 10))()
        for l, lv in enumerate(planes):
            for p, name in enumerate(PLANES):
                a = lv.get(name)
                if a is None or a.size == 0:
                    continue
                a = np.ascontiguousarray(a, np.float32)
                keep.append(a)
                tab[l * 10 + p] = a.ctypes.data
        res = C.c_void_p()
        _check(lib().akz_extract_from_planes(self._h, w, h, C.byref(options), tab, n, 0 if detect else AKZ_NO_DETECT,
                                             C.byref(res)))
        return ExtractResult(self, res)

    def extract_begin(self, frames, options=None, keep_all_planes=True, host_descriptors=True, input_ready=False):
        """First half of extract_features on a torch CUDA tensor [N, H, W] (uint8 or float32): enqueue the
        GPU work up to the extrema candidates and return a Job without synchronising.  input_ready=True (AKZ_INPUT_READY):
        the frames are complete in device memory now (nothing pending on any stream writes them): the first stages of a
        large batch then run ahead, under the kernels of the batch begun before."""
        import torch
        options = options or Config()
        flags = _extract_flags(keep_all_planes, host_descriptors, input_ready)
        t = frames
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
            raise ValueError("device images must be contiguous torch CUDA tensors")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        n, h, w = t.shape
        fn = lib().akz_extract_begin_device_u8 if t.dtype == torch.uint8 else lib().akz_extract_begin_device_f32
        job = C.c_void_p()
        _check(fn(self._h, C.c_void_p(t.data_ptr()), w, h, n, C.byref(options), flags, C.byref(job)))
        return Job(self, job, t)

    def _device_frames(self, t, layout, order):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
            raise ValueError("device frames must be uint8 torch CUDA tensors")
        return frame_layout_of(t.shape, t.stride(), layout, order)

    def luma_from_frames(self, t, layout="hwc", order="rgb", out=None):
        """akz_luma_from_frames_device: to_luma of the frames of a uint8 torch CUDA view (frame_layout_of: crops, pitched
        and non-contiguous batches pass with no copy) as a [N, H, W] uint8 CUDA tensor ([H, W] for one unbatched frame),
        enqueued on the context's stream.  out: a contiguous uint8 CUDA tensor of N*H*W elements to write instead (any
        alignment)."""
        import torch
        fl, n, batched = self._device_frames(t, layout, order)
        shape = (n, fl.height, fl.width) if batched else (fl.height, fl.width)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=t.device)
        elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * fl.height * fl.width):
            raise ValueError("out must be a contiguous uint8 CUDA tensor of N*H*W elements")
        _check(lib().akz_luma_from_frames_device(self._h, C.c_void_p(t.data_ptr()), C.byref(fl), n, C.c_void_p(out.data_ptr())))
        return out.view(shape)

    def _device_mask(self, mask, n, fl):
        import torch
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
            raise ValueError("a device mask must be a uint8 or bool torch CUDA tensor")
        return mask_layout_of(mask, n, fl.height, fl.width)

    def extract_frames(self, t, layout="hwc", order="rgb", options=None, keep_all_planes=True, host_descriptors=True, mask=None):
        """akz_extract_device_frames: extract_features on the luma of colour, pitched or cropped device frames -- the
        result of extract_features(luma_from_frames(t)), bit for bit.  Keypoint coordinates are relative to the view.
        mask (akz_extract_device_frames_masked): a uint8 or bool CUDA tensor [H, W] (shared) or [N, H, W], any row and frame
        strides; nonzero = detect here.  Masked pixels raise no extrema candidates (include/akaze_hip.h)."""
        options = options or Config()
        flags = _extract_flags(keep_all_planes, host_descriptors)
        fl, n, _ = self._device_frames(t, layout, order)
        res = C.c_void_p()
        if mask is None:
            _check(lib().akz_extract_device_frames(self._h, C.c_void_p(t.data_ptr()), C.byref(fl), n, C.byref(options), flags,
                                                   C.byref(res)))
        else:
            ml, n_masks = self._device_mask(mask, n, fl)
            _check(lib().akz_extract_device_frames_masked(self._h, C.c_void_p(t.data_ptr()), C.byref(fl), n, C.c_void_p(mask.data_ptr()),
                                                          C.byref(ml), n_masks, C.byref(options), flags, C.byref(res)))
        return ExtractResult(self, res)

    def extract_frames_begin(self, t, layout="hwc", order="rgb", options=None, keep_all_planes=True, host_descriptors=True,
                             input_ready=False, mask=None):
        """akz_extract_begin_device_frames: the first half of extract_frames, returning a Job without synchronising.
        input_ready=True (AKZ_INPUT_READY): the frames (and the mask) are complete in device memory now; the conversion then
        runs on the context's copy stream, under the kernels of the batch begun before.  mask: as extract_frames.  The Job keeps
        the tensor and the mask alive."""
        options = options or Config()
        flags = _extract_flags(keep_all_planes, host_descriptors, input_ready)
        fl, n, _ = self._device_frames(t, layout, order)
        job = C.c_void_p()
        if mask is None:
            _check(lib().akz_extract_begin_device_frames(self._h, C.c_void_p(t.data_ptr()), C.byref(fl), n, C.byref(options),
                                                         flags, C.byref(job)))
            return Job(self, job, t)
        ml, n_masks = self._device_mask(mask, n, fl)
        _check(lib().akz_extract_begin_device_frames_masked(self._h, C.c_void_p(t.data_ptr()), C.byref(fl), n, C.c_void_p(mask.data_ptr()),
                                                            C.byref(ml), n_masks, C.byref(options), flags, C.byref(job)))
        return Job(self, job, (t, mask))

    def extract_features_masked(self, image, mask, options=None, keep_all_planes=True):
        """akz_extract_gray_u8_masked: extract_features of a HOST uint8 [H, W] image with a host mask of its size (uint8 or bool,
        nonzero = detect here)."""
        options = options or Config()
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("a masked host image must be a uint8 [H, W] array")
        m = np.asarray(mask)
        if m.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"a mask must be uint8 or bool, got {m.dtype}")
        if m.shape != img.shape:
            raise ValueError(f"the mask is {m.shape} but the image is {img.shape}")
        m = np.ascontiguousarray(m).view(np.uint8)
        res = C.c_void_p()
        _check(lib().akz_extract_gray_u8_masked(self._h, img.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), img.shape[1],
                                                img.shape[0], C.byref(options), _extract_flags(keep_all_planes), C.byref(res)))
        return ExtractResult(self, res)

    def debug_mask_candidates(self, records, capacity, counts, mask, w, h, n, kept, options=None):
        """akz_debug_mask_candidates: k_mask_candidates alone, enqueued on the context's stream.  records / kept: CUDA tensors of
        capacity x 32 bytes (CANDIDATE_IMG_DTYPE); counts: a CUDA tensor of four int32 / uint32 words, [0] = the list's length; mask:
        as extract_frames."""
        options = options or Config()
        ml, n_masks = mask_layout_of(mask, n, h, w)
        _check(lib().akz_debug_mask_candidates(self._h, C.c_void_p(records.data_ptr()), capacity, C.c_void_p(counts.data_ptr()),
                                               C.c_void_p(mask.data_ptr()), C.byref(ml), n_masks, w, h, C.byref(options), n,
                                               C.c_void_p(kept.data_ptr())))

    def debug_mask_counts(self):
        """akz_debug_mask_counts of the last finished masked job -> dict(unfiltered, kept, redone)."""
        out = (C.c_uint64 * 3)()
        _check(lib().akz_debug_mask_counts(self._h, out))
        return dict(unfiltered=int(out[0]), kept=int(out[1]), redone=int(out[2]))

    def extract_begin_host(self, frames, options=None, keep_all_planes=True, host_descriptors=True):
        """extract_begin for frames in HOST memory (akz_extract_begin_host_*): a numpy array or a torch CPU tensor
        [N, H, W] (uint8 or float32), ideally pinned (torch .pin_memory()): the upload runs on the context's copy
        stream, under the kernels of the batch begun before.  The Job keeps the frames alive until it is finished."""
        import torch
        options = options or Config()
        flags = _extract_flags(keep_all_planes, host_descriptors)
        t = frames
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if not (isinstance(t, torch.Tensor) and not t.is_cuda and t.is_contiguous()):
            raise ValueError("host images must be contiguous numpy arrays or torch CPU tensors")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError("host images must be uint8 or float32")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        n, h, w = t.shape
        fn = lib().akz_extract_begin_host_u8 if t.dtype == torch.uint8 else lib().akz_extract_begin_host_f32
        job = C.c_void_p()
        _check(fn(self._h, C.c_void_p(t.data_ptr()), w, h, n, C.byref(options), flags, C.byref(job)))
        return Job(self, job, t)

    def descriptor_match(self, d0, d1, distance_threshold=10000, lowes_ratio=0.86):
        """ops::feature_matching::descriptor_match (akaze/src/ops/feature_matching.rs:23-94)."""
        return _descriptor_pair(lib().akz_descriptor_match, (self._h,), d0, d1, distance_threshold, lowes_ratio)

    def match_features_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers):
        """match_features (lib.rs:252-275) over many pairs in one call (akz_match_features_pairs): features is a list of
        (keypoints, descriptors) arrays (KEYPOINT_DTYPE / uint8 [n, desc_bytes]), pairs a sequence of (first, second) indices
        into it.  Returns one MATCH_DTYPE array per pair, each equal to what match_features returns for that pair when the
        pairs are matched in order on this thread."""
        return _match_pairs(self, "", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers)

    def match_features_homography_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers):
        """match_features_homography over many pairs in one call (akz_match_features_homography_pairs), arguments as for
        match_features_pairs.  Returns one (matches, H or None) per pair, each equal to what match_features_homography returns
        for that pair when the pairs are matched in order on this thread."""
        return _match_pairs(self, "_homography", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers)

    def match_features_homography_guided_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                               guided_radius, guided_lowes_ratio):
        """match_features_homography_pairs, then the guided scan with every H found
        (akz_match_features_homography_guided_pairs).  Returns one (matches, H or None) per pair: with an H the list of
        descriptor_match_guided(pair, GUIDED_HOMOGRAPHY, H, guided_radius, 10000, guided_lowes_ratio), without one the list
        of match_features_homography_pairs."""
        return _match_pairs(self, "_homography", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                            guided=(guided_radius, guided_lowes_ratio))

    def match_features_homography_refined_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                refine_iterations):
        """match_features_homography_pairs with the refit of every H found on its inliers
        (akz_match_features_homography_refined_pairs).  Returns one (matches, H or None, accepted fits) per pair, each equal
        to what match_features_homography_refined returns for that pair when the pairs are matched in order on this thread."""
        return _match_pairs(self, "_homography", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations)

    def match_features_homography_refined_guided_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                       refine_iterations, guided_radius, guided_lowes_ratio):
        """match_features_homography_refined_pairs, then the guided scan with every REFINED H
        (akz_match_features_homography_refined_guided_pairs).  Returns one (matches, H or None, accepted fits) per pair."""
        return _match_pairs(self, "_homography", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations,
                            (guided_radius, guided_lowes_ratio))

    def match_features_fundamental_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers):
        """match_features_pairs with the fundamental matrix that filtered every pair (akz_match_features_fundamental_pairs).
        Returns one (matches, F or None) per pair: the list of match_features_pairs, F the RANSAC winner."""
        return _match_pairs(self, "_fundamental", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers)

    def match_features_fundamental_refined_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                 refine_iterations):
        """match_features_fundamental_pairs with the refit of every F found on its inliers
        (akz_match_features_fundamental_refined_pairs).  Returns one (matches, F or None, accepted fits) per pair, each equal
        to what match_features_fundamental_refined returns for that pair when the pairs are matched in order on this thread."""
        return _match_pairs(self, "_fundamental", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations)

    def match_features_fundamental_guided_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                guided_radius, guided_lowes_ratio):
        """match_features_fundamental_pairs, then the guided scan with every F found
        (akz_match_features_fundamental_guided_pairs).  Returns one (matches, F or None) per pair: with an F the list of
        descriptor_match_guided(pair, GUIDED_FUNDAMENTAL, F, guided_radius, 10000, guided_lowes_ratio), without one the list
        of match_features_fundamental_pairs."""
        return _match_pairs(self, "_fundamental", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                            guided=(guided_radius, guided_lowes_ratio))

    def match_features_fundamental_refined_guided_pairs(self, features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                        refine_iterations, guided_radius, guided_lowes_ratio):
        """match_features_fundamental_refined_pairs, then the guided scan with every REFINED F
        (akz_match_features_fundamental_refined_guided_pairs).  Returns one (matches, F or None, accepted fits) per pair."""
        return _match_pairs(self, "_fundamental", features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations,
                            (guided_radius, guided_lowes_ratio))

    def feature_bank(self, results_or_features, budget=None):
        """A FeatureBank of this context: feature sets kept on the device in the layout the pairs calls scan.  From one
        ExtractResult or a sequence of them (akz_bank_create_from_results: every image of every result is a set, in order; the
        descriptor rows never leave the device, and the results may be closed at once), or from a sequence of (keypoints,
        descriptors) host sets (akz_bank_create_from_sets: packed and uploaded once).  Pass it as `features` to
        match_features_seeded_pairs / match_features_seeded_pose_pairs; close() it when done.
        budget: a KeypointBudget cuts every set as keypoint_budget_host would, on the device (akz_bank_create_from_results_budget /
        _from_sets_budget): the bank equals feature_bank of the sliced host sets, and FeatureBank.indices() names the keypoints kept."""
        src = results_or_features
        if budget is not None and not isinstance(budget, KeypointBudget):
            raise TypeError(f"budget must be a KeypointBudget or None, got {type(budget).__name__}")
        if isinstance(src, ExtractResult):
            src = [src]
        if isinstance(src, (str, bytes, FeatureBank)) or not hasattr(src, "__len__"):
            raise TypeError(f"feature_bank takes ExtractResult objects or (keypoints, descriptors) sets, got {type(src).__name__}")
        h = C.c_void_p()
        if len(src) and all(isinstance(r, ExtractResult) for r in src):
            arr = (C.c_void_p * len(src))(*[r._h for r in src])
            if budget is not None:
                _check(lib().akz_bank_create_from_results_budget(self._h, arr, len(src), C.byref(budget), C.byref(h)))
            else:
                _check(lib().akz_bank_create_from_results(self._h, arr, len(src), C.byref(h)))
            return FeatureBank(self, h)
        if any(isinstance(r, ExtractResult) for r in src):
            raise TypeError("feature_bank takes results or host sets, not a mixture")
        for f in src:
            if not (isinstance(f, (tuple, list)) and len(f) == 2):
                raise TypeError(f"a host set is (keypoints, descriptors), got {type(f).__name__}")
        sets, keep, rows, nb = _pack_sets(src)
        if budget is not None:
            _check(lib().akz_bank_create_from_sets_budget(self._h, C.cast(sets, C.c_void_p), len(rows), nb, C.byref(budget), C.byref(h)))
        else:
            _check(lib().akz_bank_create_from_sets(self._h, C.cast(sets, C.c_void_p), len(rows), nb, C.byref(h)))
        return FeatureBank(self, h)

    def debug_bank_gather(self, src, desc_bytes, dst):
        """akz_debug_bank_gather: k_bank_gather alone over the rows of the torch CUDA uint8 tensor src [rows, 64] into dst (same shape);
        complete on return."""
        import torch
        torch.cuda.current_stream(src.device).synchronize()
        _check(lib().akz_debug_bank_gather(self._h, C.c_void_p(src.data_ptr()), int(src.shape[0]), int(desc_bytes), C.c_void_p(dst.data_ptr())))

    def debug_bank_select(self, src, sx, sy, n, keep, indices, desc_bytes, rows, x, y, index):
        """akz_debug_bank_select: k_bank_select alone.  src [sum n, 64] uint8, sx, sy [sum n] float32: torch CUDA tensors, the sets'
        sources packed one behind the other; n, keep: per set; indices: the kept indices of every set one behind the other (the
        hook refuses lists that do not ascend or reach n).  rows [>= sum keep, 64] uint8, x, y float32 and index int32 /
        uint32 [>= sum keep]: torch CUDA tensors that receive the selection; complete on return."""
        import torch
        torch.cuda.current_stream(src.device).synchronize()
        n, keep = np.ascontiguousarray(n, np.uint64), np.ascontiguousarray(keep, np.uint64)
        idx = np.ascontiguousarray(indices, np.uint32)
        _check(lib().akz_debug_bank_select(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(sx.data_ptr()), C.c_void_p(sy.data_ptr()), len(n),
                                           n.ctypes.data_as(C.POINTER(C.c_uint64)), keep.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           idx.ctypes.data_as(C.POINTER(C.c_uint32)), int(desc_bytes), C.c_void_p(rows.data_ptr()),
                                           C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(index.data_ptr())))

    def match_features_seeded_pairs(self, features, pairs, options=None, cross_check=False):
        """match_features over many pairs with the seeded RANSAC (akz_match_features_seeded_pairs): the trial kernel draws its
        own samples from (options.seed, options.stream_base + pair, trial) and options.confidence stops a pair's trials on the
        device; the thread's random source is not touched.  Returns one (matches, model or None, accepted fits, trials run) per
        pair, each equal to remove_outliers_seeded on that pair's raw list with stream = stream_base + pair (then the guided
        scan, if options.guided).  cross_check: the raw list is descriptor_match_cross_host(pair, 10000, options.lowes_ratio)
        -- a match must be the best in both directions -- (akz_match_features_seeded_cross_pairs); the guided scan stays
        one-directional.  features: a list of (keypoints, descriptors) per set, or a FeatureBank of this context
        (akz_match_features_seeded_bank_pairs: the same results, no set is packed or uploaded)."""
        a = _PairsArgs(self, features, pairs, bank_ok=True)
        opt = options if options is not None else RansacOptions()
        tr = np.zeros(max(1, len(a.pr)), np.uint64)
        if a.bank is not None:  # (the bank call takes cross_check as an argument, the host-set calls are two functions)
            fn, cross = lib().akz_match_features_seeded_bank_pairs, (int(bool(cross_check)),)
        else:
            fn, cross = lib().akz_match_features_seeded_cross_pairs if cross_check else lib().akz_match_features_seeded_pairs, ()
        _check(fn(*a.head, C.byref(opt), *cross, *a.tail, *a.refined(), tr.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [(m, h, it, int(tr[p])) for p, (m, h, it) in enumerate(a.lists_models_iterations())]

    def match_features_seeded_pose_pairs(self, features, cameras, pairs, options=None, cross_check=False, points=False):
        """match_features_seeded_pairs with the pose stage behind it (akz_match_features_seeded_pose_pairs): cameras holds one
        Camera (or (fx, fy, cx, cy), or a 3 x 3 K) per feature set.  Returns one (matches, model or None, accepted fits, trials
        run, Pose) per pair -- with points=True a sixth entry, the [len(matches), 3] float32 structure in camera 0's frame at
        |t| = 1, or None without a pose -- each equal to remove_outliers_seeded on that pair's raw list followed, where a model
        was found, by recover_pose_host with that list and model.  options.guided and the homography kind are refused.
        features may be a FeatureBank of this context (akz_match_features_seeded_pose_bank_pairs), with one camera per set of it."""
        a = _PairsArgs(self, features, pairs, bank_ok=True)
        opt = options if options is not None else RansacOptions()
        if len(cameras) != a.n_sets:
            raise ValueError(f"{a.n_sets} feature sets but {len(cameras)} cameras")
        cams = (Camera * max(1, a.n_sets))(*[Camera.of(k) for k in cameras])
        tr = np.zeros(max(1, len(a.pr)), np.uint64)
        poses = (Pose * max(1, len(a.pr)))()
        pts = np.zeros((len(a.out), 3), np.float32) if points else None
        fn, at_cams = (lib().akz_match_features_seeded_pose_bank_pairs, 2) if a.bank is not None else (lib().akz_match_features_seeded_pose_pairs, 3)
        _check(fn(*a.head[:at_cams], C.cast(cams, C.c_void_p), *a.head[at_cams:], C.byref(opt), int(bool(cross_check)),
                  *a.tail, *a.refined(), tr.ctypes.data_as(C.POINTER(C.c_uint64)),
                  C.cast(poses, C.c_void_p), pts.ctypes.data_as(C.POINTER(C.c_float)) if points else None))
        res, at = [], 0
        for p, (m, h, it) in enumerate(a.lists_models_iterations()):
            pose = Pose.from_buffer_copy(poses[p])
            row = (m, h, it, int(tr[p]), pose)
            if points:
                row += (pts[at:at + len(m)].copy() if pose.found else None,)
            res.append(row)
            at += a.rows[p]
        return res

    def resection_seeded(self, problems, options):
        """Absolute pose by the seeded 6-point resection RANSAC over many problems in one call (akz_resection_seeded_problems):
        problems is a list of (points [n, 3], pixels [n, 2], camera), options a RansacOptions with model_kind RANSAC_RESECTION and
        epsilon_inliers in pixels.  Returns one (kept indices ascending, Resection, accepted fits, trials run) per problem, each
        equal to resection_seeded_host(problem, options, stream=options.stream_base + p) bit for bit."""
        a = _ResectionArgs(problems)
        _check(lib().akz_resection_seeded_problems(self._h, a.problems, len(a.sizes), C.byref(options), *a.tail()))
        return a.results()

    def descriptor_match_guided_pairs(self, features, pairs, models, kind, radius, distance_threshold=10000, lowes_ratio=0.86):
        """Guided matching over many pairs in one call (akz_descriptor_match_guided_pairs): features and pairs as for
        match_features_pairs, models one 3x3 (or 9) float32 model per pair, kind GUIDED_HOMOGRAPHY or GUIDED_FUNDAMENTAL.
        Returns one MATCH_DTYPE array per pair, each equal to descriptor_match_guided on that pair."""
        a = _PairsArgs(self, features, pairs)
        md = np.ascontiguousarray(np.asarray(models, np.float32).reshape(-1, 9))
        if len(md) != len(a.pr):
            raise ValueError(f"{len(a.pr)} pairs but {len(md)} models")
        if len(md) == 0:
            md = np.zeros((1, 9), np.float32)
        _check(lib().akz_descriptor_match_guided_pairs(*a.head, int(kind), md.ctypes.data_as(C.POINTER(C.c_float)), radius,
                                                       distance_threshold, lowes_ratio, *a.tail))
        return a.lists()

    def descriptor_match_sets_device(self, q, train, rows, distance_threshold=10000, lowes_ratio=0.86):
        """One query set against several train sets in one launch: q [n0, 64] uint8 CUDA tensor, train the sets'
        64-byte rows one after the other ([sum(rows), 64]), rows the row count of every set.  Returns (matches
        [n_sets, n0, 24] uint8 — akz_match records, set k's first counts[k] are valid, index_1 relative to the
        set — and counts [n_sets] int64), the same as one descriptor_match_device call per set."""
        import torch
        n0, ns = int(q.shape[0]), len(rows)
        out = torch.empty((ns, max(n0, 1), 24), dtype=torch.uint8, device=q.device)
        if n0 == 0:
            out = out[:, :0]
        cnt = torch.zeros(max(ns, 1), dtype=torch.int64, device=q.device)
        arr = (C.c_uint64 * max(ns, 1))(*[int(r) for r in rows])
        _check(lib().akz_descriptor_match_sets_device(self._h, C.c_void_p(q.data_ptr()) if n0 else None, n0,
                                                      C.c_void_p(train.data_ptr()) if sum(rows) else None, arr, ns,
                                                      distance_threshold, lowes_ratio, C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(cnt.data_ptr())))
        return out, cnt[:ns]

    def descriptor_match_sets_mutual_device(self, q, train, rows, distance_threshold=10000, lowes_ratio=0.86):
        """descriptor_match_sets_device plus the opposite direction of every block from the same pass: returns (matches,
        counts, col_matches [sum(rows), 24] uint8 -- set k's list starts at row sum(rows[:k]) --, col_counts [n_sets])."""
        import torch
        n0, ns, tot = int(q.shape[0]), len(rows), int(sum(rows))
        out = torch.empty((ns, max(n0, 1), 24), dtype=torch.uint8, device=q.device)
        if n0 == 0:
            out = out[:, :0]
        cnt = torch.zeros(max(ns, 1), dtype=torch.int64, device=q.device)
        cout = torch.empty((max(tot, 1), 24), dtype=torch.uint8, device=q.device)
        ccnt = torch.zeros(max(ns, 1), dtype=torch.int64, device=q.device)
        arr = (C.c_uint64 * max(ns, 1))(*[int(r) for r in rows])
        _check(lib().akz_descriptor_match_sets_mutual_device(
            self._h, C.c_void_p(q.data_ptr()) if n0 else None, n0, C.c_void_p(train.data_ptr()) if tot else None, arr, ns,
            distance_threshold, lowes_ratio, C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(cout.data_ptr()),
            C.c_void_p(ccnt.data_ptr())))
        return out, cnt[:ns], cout[:tot], ccnt[:ns]

    def descriptor_match_cross(self, d0, d1, distance_threshold=10000, lowes_ratio=0.86):
        """Cross-checked descriptor_match (akz_descriptor_match_cross): the records of descriptor_match(d0, d1) whose train row,
        matched the other way round, comes back to the same query row.  Equal to descriptor_match_cross_host."""
        return _descriptor_pair(lib().akz_descriptor_match_cross, (self._h,), d0, d1, distance_threshold, lowes_ratio)

    def descriptor_match_cross_device(self, d0, d1, distance_threshold=10000, lowes_ratio=0.86):
        """descriptor_match_cross on torch CUDA uint8 tensors of 64-byte descriptor rows (akz_descriptor_match_cross_device);
        returns (matches tensor view, count) as descriptor_match_device does."""
        return self._device_pair(lib().akz_descriptor_match_cross_device, d0, d1, distance_threshold, lowes_ratio)

    def descriptor_match_knn(self, d0, d1, k, distance_threshold=10000):
        """k-nearest-neighbour matching on the GPU (akz_descriptor_match_knn): for every row of d0 its k nearest rows of d1 below
        the threshold, ordered by (distance, index) -> (records of shape (n0, k) in MATCH_DTYPE, counts of shape (n0,) uint32).
        Slots beyond a row's count hold index_1 = 2^64 - 1 and distance = inf.  Equal to descriptor_match_knn_host; rows of at
        most 61 bytes."""
        return _knn_pair(lib().akz_descriptor_match_knn, (self._h,), d0, d1, k, distance_threshold)

    def descriptor_match_knn_device(self, d0, d1, k, distance_threshold=10000):
        """descriptor_match_knn on torch CUDA uint8 tensors of 64-byte descriptor rows (akz_descriptor_match_knn_device; bytes
        61..63 are not compared) -> (records: uint8 tensor (n0, k, 24), one akz_match per slot; counts: int32 tensor (n0,) holding
        the uint32 counts), both on the device, enqueued on the context's stream."""
        import torch
        n0, n1 = d0.shape[0], d1.shape[0]
        out = torch.empty((n0, int(k), 24), dtype=torch.uint8, device=d0.device)
        cnt = torch.empty((n0,), dtype=torch.int32, device=d0.device)
        _check(lib().akz_descriptor_match_knn_device(self._h, C.c_void_p(d0.data_ptr()) if n0 else None, n0,
                                                     C.c_void_p(d1.data_ptr()) if n1 else None, n1, int(k), distance_threshold,
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())))
        return out, cnt

    def set_knn_chunks(self, n=0):
        """akz_debug_set_knn_chunks (include/akaze_hip_debug.h): force the train chunks of the k-NN scan; 0 = automatic."""
        _check(lib().akz_debug_set_knn_chunks(self._h, int(n)))

    def keypoint_budget_sets(self, features, max_keypoints, mode=BUDGET_SPREAD, robust=0.9):
        """The keypoint budget over many sets in one call on the GPU (akz_keypoint_budget_sets): features as for the pairs calls,
        a sequence of (keypoints, descriptors) -- only the keypoints are read, a bare keypoint array will do.  Returns one
        (indices uint64 ascending, radius2 float32 [n] or None in BUDGET_STRONGEST mode) per set, each equal to
        keypoint_budget_host on that set."""
        sets, (ks, _), _, _ = _pack_sets(features, keypoints_only=True)
        total = sum(len(k) for k in ks)
        opt = KeypointBudget(int(max_keypoints), int(mode), float(robust))
        idx = np.zeros(max(1, total), np.uint64)
        n = np.zeros(max(1, len(ks)), np.uint64)
        rad = np.zeros(max(1, total), np.float32) if mode == BUDGET_SPREAD else None
        _check(lib().akz_keypoint_budget_sets(self._h, C.cast(sets, C.c_void_p), len(ks), C.byref(opt), idx.ctypes.data_as(C.c_void_p),
                                              n.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p) if rad is not None else None))
        res, at = [], 0
        for s, k in enumerate(ks):
            res.append((idx[at:at + int(n[s])].copy(), rad[at:at + len(k)].copy() if rad is not None else None))
            at += len(k)
        return res

    def debug_keypoint_budget_split(self, enable=True):
        """akz_debug_keypoint_budget_split (include/akaze_hip_debug.h): time the later keypoint_budget_sets calls; returns the last
        timed call's (upload, kernels, download) in ms."""
        ms = (C.c_double * 3)()
        _check(lib().akz_debug_keypoint_budget_split(self._h, int(bool(enable)), ms))
        return tuple(ms)

    def descriptor_match_device(self, d0, d1, distance_threshold=10000, lowes_ratio=0.86):
        """Same on torch CUDA uint8 tensors of 64-byte descriptor rows; returns (matches tensor view, count)."""
        return self._device_pair(lib().akz_descriptor_match_device, d0, d1, distance_threshold, lowes_ratio)

    def _device_pair(self, fn, d0, d1, distance_threshold, lowes_ratio):
        import torch
        n0, n1 = d0.shape[0], d1.shape[0]
        out = torch.empty((max(n0, 1), 24), dtype=torch.uint8, device=d0.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=d0.device)
        _check(fn(self._h, C.c_void_p(d0.data_ptr()), n0, C.c_void_p(d1.data_ptr()), n1, distance_threshold, lowes_ratio,
                  C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())))
        return out, cnt

    # ---- per-op entry points on torch CUDA float32 tensors [N, H, W] or [H, W] -----------
    def _nhw(self, t):
        if t.dim() == 2:
            return 1, t.shape[0], t.shape[1]
        return t.shape[0], t.shape[1], t.shape[2]

    def _taps(self, taps):
        taps = np.ascontiguousarray(taps, np.float32)
        return taps, taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps)

    def horizontal_filter(self, img, taps):
        import torch
        n, h, w = self._nhw(img)
        out = torch.empty_like(img)
        k, pk, nk = self._taps(taps)
        _check(lib().akz_op_horizontal_filter(self._h, img.data_ptr(), out.data_ptr(), w, h, n, pk, nk))
        return out

    def vertical_filter(self, img, taps):
        import torch
        n, h, w = self._nhw(img)
        out = torch.empty_like(img)
        k, pk, nk = self._taps(taps)
        _check(lib().akz_op_vertical_filter(self._h, img.data_ptr(), out.data_ptr(), w, h, n, pk, nk))
        return out

    def gaussian_blur(self, img, sigma):
        import torch
        n, h, w = self._nhw(img)
        out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        fn = lib().akz_op_gaussian_blur_u8 if img.dtype == torch.uint8 else lib().akz_op_gaussian_blur
        _check(fn(self._h, img.data_ptr(), out.data_ptr(), w, h, n, sigma))
        return out

    def half_size(self, img):
        import torch
        n, h, w = self._nhw(img)
        shape = (h // 2, w // 2) if img.dim() == 2 else (n, h // 2, w // 2)
        out = torch.empty(shape, dtype=torch.float32, device=img.device)
        _check(lib().akz_op_half_size(self._h, img.data_ptr(), out.data_ptr(), w, h, n))
        return out

    def scharr(self, img, x_order, y_order, sigma_size):
        import torch
        n, h, w = self._nhw(img)
        out = torch.empty_like(img)
        _check(lib().akz_op_scharr(self._h, img.data_ptr(), out.data_ptr(), w, h, n, int(x_order), int(y_order),
                                   sigma_size))
        return out

    def debug_rcp_f64_to_f32(self, x):
        """(1.0 / x) as f32 for a CUDA float64 tensor, the way pm_g2 forms it inside the level kernels"""
        import torch
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _check(lib().akz_debug_rcp_f64_to_f32(self._h, x.data_ptr(), out.data_ptr(), x.numel()))
        return out

    def pm_g2(self, lx, ly, k):
        """k: python float or a torch CUDA float64 tensor with one value per image."""
        import torch
        n, h, w = self._nhw(lx)
        out = torch.empty_like(lx)
        kt = k if isinstance(k, torch.Tensor) else torch.full((n,), float(k), dtype=torch.float64, device=lx.device)
        _check(lib().akz_op_pm_g2(self._h, lx.data_ptr(), ly.data_ptr(), out.data_ptr(), w, h, n, kt.data_ptr()))
        return out

    def contrast_factor(self, img, percentile=0.7, gscale=1.0, nbins=300):
        import torch
        n, h, w = self._nhw(img)
        out = torch.zeros(n, dtype=torch.float64, device=img.device)
        _check(lib().akz_op_contrast_factor(self._h, img.data_ptr(), w, h, n, percentile, gscale, nbins,
                                            out.data_ptr()))
        return out

    def flow(self, lsmooth, k, k_scale_pow=0):
        import torch
        n, h, w = self._nhw(lsmooth)
        out = torch.empty_like(lsmooth)
        kt = k if isinstance(k, torch.Tensor) else torch.full((n,), float(k), dtype=torch.float64,
                                                              device=lsmooth.device)
        _check(lib().akz_op_flow(self._h, lsmooth.data_ptr(), out.data_ptr(), w, h, n, kt.data_ptr(), k_scale_pow))
        return out

    def fed_steps(self, lt, lflow, taus, want_lstep=False):
        """calculate_step for each tau, in place on `lt` (as the reference mutates evolution.Lt)."""
        import torch
        n, h, w = self._nhw(lt)
        taus = np.ascontiguousarray(taus, np.float64)
        lstep = torch.zeros_like(lt) if want_lstep else None
        _check(lib().akz_op_fed_steps(self._h, lt.data_ptr(), lflow.data_ptr(), lstep.data_ptr() if want_lstep else None,
                                      w, h, n, taus.ctypes.data_as(C.POINTER(C.c_double)), len(taus)))
        return lstep

    def detector_response(self, lsmooth, sigma_size, keep_second=True):
        import torch
        n, h, w = self._nhw(lsmooth)
        names = ["Lx", "Ly", "Lxx", "Lyy", "Lxy", "Ldet"]
        outs = {k: torch.empty_like(lsmooth) for k in names if keep_second or k in ("Lx", "Ly", "Ldet")}
        p = lambda k: outs[k].data_ptr() if k in outs else None
        _check(lib().akz_op_detector_response(self._h, lsmooth.data_ptr(), sigma_size, p("Lx"), p("Ly"), p("Lxx"),
                                              p("Lyy"), p("Lxy"), p("Ldet"), w, h, n))
        return outs


class Job:
    """An extraction in flight (akz_extract_begin_*); finish() exactly once."""

    def __init__(self, ctx, handle, frames):
        self._ctx, self._h, self._frames = ctx, handle, frames  # keep the frames alive

    def finish(self):
        res = C.c_void_p()
        h, self._h = self._h, None
        _check(lib().akz_extract_finish(h, C.byref(res)))
        self._frames = None
        return ExtractResult(self._ctx, res)

    def abandon(self):
        """Drop the extraction without a result (akz_job_abandon)."""
        if getattr(self, "_h", None):
            lib().akz_job_abandon(self._h)
            self._h = None
        self._frames = None

    def __del__(self):
        self.abandon()


class FeatureBank:
    """An akz_bank: feature sets resident on the device (Context.feature_bank).  Immutable; close() returns its device block."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle

    def close(self):
        if self._h:
            lib().akz_bank_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """dict(n_sets, desc_bytes, rows, sets=[dict(n_keypoints, n_descriptors, row0) per set])"""
        n, nb, rows = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().akz_bank_info(self._h, C.byref(n), C.byref(nb), C.byref(rows)))
        sets = []
        for k in range(n.value):
            nk, nd, r0 = C.c_uint64(), C.c_uint64(), C.c_uint64()
            _check(lib().akz_bank_set_info(self._h, k, C.byref(nk), C.byref(nd), C.byref(r0)))
            sets.append(dict(n_keypoints=nk.value, n_descriptors=nd.value, row0=r0.value))
        return dict(n_sets=n.value, desc_bytes=nb.value, rows=rows.value, sets=sets)

    def indices(self, set=None):
        """akz_bank_set_indices: for every row of set `set`, the index in its source set of the keypoint it came from, a uint64
        array -- what keypoint_budget_host kept for a bank made with a budget, arange otherwise; set=None: a list of them, one
        per set.  It carries a match record's index_0 / index_1 over the bank back to the extraction result."""
        sets = self.info()["sets"]
        if set is None:
            return [self.indices(k) for k in range(len(sets))]
        if not 0 <= int(set) < len(sets):
            raise IndexError(f"set index {set} >= n_sets {len(sets)}")
        out = np.zeros(sets[int(set)]["n_keypoints"], np.uint64)
        _check(lib().akz_bank_set_indices(self._h, int(set), out.ctypes.data_as(C.POINTER(C.c_uint64)) if len(out) else None))
        return out

    def device(self):
        """(address of the rows [rows, 64] uint8, of x [rows] float32, of y [rows] float32) on the device; read-only, valid until close()."""
        r, x, y = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().akz_bank_device(self._h, C.byref(r), C.byref(x), C.byref(y)))
        return r.value, x.value, y.value

    def download(self):
        """The three device buffers as numpy arrays (rows [rows, 64] uint8, x, y float32): a copy, for inspection."""
        n = self.info()["rows"]
        r, x, y = self.device()
        rows, hx, hy = np.zeros((n, 64), np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32)
        if n:
            for dst, src in ((rows, r), (hx, x), (hy, y)):
                copy_raw(dst.ctypes.data, src, dst.nbytes, 2)
        return rows, hx, hy


class ExtractResult:
    """(Vec<EvolutionStep>, Vec<Keypoint>, Vec<Descriptor>) of akaze::extract_features, per image of the
    batch; EvolutionStep images stay on the GPU and are fetched lazily."""

    def __init__(self, ctx, handle):
        self._ctx = ctx
        self._h = handle
        n = C.c_uint64()
        _check(lib().akz_result_num_images(handle, C.byref(n)))
        self.num_images = n.value

    def close(self):
        if self._h:
            lib().akz_result_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self, img=0):
        nl, nk, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().akz_result_counts(self._h, img, C.byref(nl), C.byref(nk), C.byref(nb)))
        return nl.value, nk.value, nb.value

    def keypoints(self, img=0):
        _, nk, _ = self.counts(img)
        out = np.zeros(nk, KEYPOINT_DTYPE)
        _check(lib().akz_result_keypoints(self._h, img, out.ctypes.data_as(C.c_void_p)))
        return out

    def descriptors(self, img=0):
        _, nk, nb = self.counts(img)
        out = np.zeros((nk, nb), np.uint8)
        _check(lib().akz_result_descriptors(self._h, img, out.ctypes.data_as(C.c_void_p)))
        return out

    def device_descriptors(self, img=0):
        """(device address, rows) of the 64-byte descriptor rows of image `img`."""
        p, n = C.c_void_p(), C.c_uint64()
        _check(lib().akz_result_device_descriptors(self._h, img, C.byref(p), C.byref(n)))
        return p.value, n.value

    def copy_device_descriptors(self, dst):
        """D2D copy of every image's 64-byte descriptor rows into the torch CUDA uint8 tensor dst [rows, 64].  The copy runs on a
        stream of the context's own and is complete on return; what torch itself still has queued for `dst` (the fill of a
        torch.zeros) is waited for first, or it could land after the copy."""
        import torch
        torch.cuda.current_stream(dst.device).synchronize()
        n = C.c_uint64()
        _check(lib().akz_result_copy_device_descriptors(self._h, C.c_void_p(dst.data_ptr()), dst.shape[0],
                                                        C.byref(n)))
        return n.value

    def describe_keypoints(self, keypoints, img=0, compute_orientation=True):
        """compute_main_orientation + extract_descriptors for caller-supplied keypoints on the retained pyramid.
        Returns (keypoints with the angle filled in, descriptors[n, desc_bytes])."""
        kp = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE).copy()
        nb = self.counts(img)[2] or ((6 + 36 + 120) * 3 + 7) // 8
        desc = np.zeros((len(kp), nb), np.uint8)
        _check(lib().akz_result_describe_keypoints(self._h, img, kp.ctypes.data, len(kp), int(bool(compute_orientation)),
                                                   desc.ctypes.data))
        return kp, desc

    def write_evolutions(self, directory, img=0):
        """types::evolution::write_evolutions: one normalised PNG per plane and level."""
        os.makedirs(directory, exist_ok=True)
        _check(lib().akz_write_evolutions(self._h, img, os.fsencode(directory)))

    def contrast(self, img=0):
        k = C.c_double()
        _check(lib().akz_result_contrast(self._h, img, C.byref(k)))
        return k.value

    def level_info(self, lvl):
        et, es = C.c_double(), C.c_double()
        o, s, ss, w, h = (C.c_uint32() for _ in range(5))
        nt = C.c_uint64()
        tau = np.zeros(8192, np.float64)
        _check(lib().akz_result_level_info(self._h, lvl, C.byref(et), C.byref(es), C.byref(o), C.byref(s),
                                           C.byref(ss), C.byref(w), C.byref(h), C.byref(nt),
                                           tau.ctypes.data_as(C.POINTER(C.c_double)), len(tau)))
        return dict(etime=et.value, esigma=es.value, octave=o.value, sublevel=s.value, sigma_size=ss.value,
                    w=w.value, h=h.value, tau=tau[:nt.value].copy())

    def plane(self, lvl, name, img=0):
        pid = PLANES.index(name) if isinstance(name, str) else int(name)
        n = C.c_uint64()
        _check(lib().akz_fetch_plane(self._h, img, lvl, pid, None, C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 0), np.float32)
        info = self.level_info(lvl)
        out = np.empty((info["h"], info["w"]), np.float32)
        _check(lib().akz_fetch_plane(self._h, img, lvl, pid, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def pyramid(self, img=0, planes=None, out=None):
        """Vec<EvolutionStep> of image `img` in one call (akz_fetch_pyramid): one dict per level, {plane name: 2-D float32
        array}, for the names in `planes` (all of PLANES by default).  The arrays are views into one contiguous float32
        buffer: `out` if given (e.g. pinned memory, torch.empty(n, pin_memory=True).numpy(); at least
        pyramid_floats(img, planes) elements), else a fresh np.empty.  Level 0's Lflow / Lstep are (0, 0) arrays.
        Pass a pinned or a reused `out` when fetching frame after frame: a fresh buffer's pages are first touched by the
        copy out of staging, which halves the rate (profiles/r07_pyramid_fetch.json)."""
        shapes = self._pyramid_shapes(img, planes)
        nl = len(shapes)
        total = sum(h * w for sh in shapes for h, w in sh.values())
        if out is None:
            buf = np.empty(total, np.float32)
        else:
            buf = out if isinstance(out, np.ndarray) else out.numpy()
            if buf.dtype != np.float32 or not buf.flags.c_contiguous or buf.size < total:
                raise ValueError(f"out must be a C-contiguous float32 buffer of at least {total} elements")
            buf = buf.reshape(-1)
        ptrs = (C.c_void_p * (nl * 10))()
        levels, off = [], 0
        for lvl, sh in enumerate(shapes):
            views = {}
            for name, (h, w) in sh.items():
                views[name] = buf[off:off + h * w].reshape(h, w)
                if h * w:
                    ptrs[lvl * 10 + PLANES.index(name)] = buf.ctypes.data + off * 4
                off += h * w
            levels.append(views)
        nbytes = C.c_uint64()
        _check(lib().akz_fetch_pyramid(self._h, img, ptrs, nl * 10, C.byref(nbytes)))
        return levels

    def pyramid_floats(self, img=0, planes=None):
        """Elements of the buffer pyramid(img, planes) fills."""
        return sum(h * w for sh in self._pyramid_shapes(img, planes) for h, w in sh.values())

    def _pyramid_shapes(self, img, planes):
        want = set(PLANES) if planes is None else {planes} if isinstance(planes, str) else set(planes)
        if want - set(PLANES):
            raise ValueError(f"unknown planes {sorted(want - set(PLANES))} (names of {PLANES})")
        names = [name for name in PLANES if name in want]  # the buffer follows akz_plane order
        shapes = []
        for lvl in range(self.counts(img)[0]):
            info = self.level_info(lvl)
            shapes.append({name: (0, 0) if lvl == 0 and name in ("Lflow", "Lstep") else (info["h"], info["w"])
                           for name in names})
        return shapes


# ------------------------------------------------------------------------------------------
# module-level mirror of the reference's free functions
# ------------------------------------------------------------------------------------------
_default_ctx = None


def _take(ptr, n, dtype=np.uint8):
    """Copy n bytes out of a buffer the library allocated, then release it."""
    try:
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,)).copy().view(dtype)
    finally:
        lib().akz_image_free(ptr)


def load_image(path):
    """image::open(path): (h, w) uint8 for luma files, (h, w, 3) for colour ones."""
    w, h, ch, px = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_void_p()
    _check(lib().akz_image_load(os.fsencode(path), C.byref(w), C.byref(h), C.byref(ch), C.byref(px)))
    a = _take(px, w.value * h.value * ch.value)
    return a.reshape(h.value, w.value) if ch.value == 1 else a.reshape(h.value, w.value, 3)


def load_image_luma(path):
    """image::open(path).to_luma(): (h, w) uint8 — the input of create_unit_float_image."""
    w, h, px = C.c_uint32(), C.c_uint32(), C.c_void_p()
    _check(lib().akz_image_load_luma(os.fsencode(path), C.byref(w), C.byref(h), C.byref(px)))
    return _take(px, w.value * h.value).reshape(h.value, w.value)


def load_image_rgb(path):
    w, h, px = C.c_uint32(), C.c_uint32(), C.c_void_p()
    _check(lib().akz_image_load_rgb(os.fsencode(path), C.byref(w), C.byref(h), C.byref(px)))
    return _take(px, w.value * h.value * 3).reshape(h.value, w.value, 3)


def luma_from_frames_host(array, layout="hwc", order="rgb"):
    """akz_luma_from_frames_host: to_luma of the frames of a uint8 numpy array or view (frame_layout_of) as a packed
    [N, H, W] array ([H, W] for one unbatched frame).  No GPU call."""
    a = np.asarray(array)
    if a.dtype != np.uint8:
        raise ValueError("frames must be uint8")
    fl, n, batched = frame_layout_of(a.shape, a.strides, layout, order)
    out = np.empty((n, fl.height, fl.width) if batched else (fl.height, fl.width), np.uint8)
    _check(lib().akz_luma_from_frames_host(C.c_void_p(a.ctypes.data), C.byref(fl), n, C.c_void_p(out.ctypes.data)))
    return out


def save_png(path, pixels):
    a = np.ascontiguousarray(pixels, np.uint8)
    ch = 1 if a.ndim == 2 else a.shape[2]
    _check(lib().akz_image_save_png(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], ch))


def save_plane_png(path, plane):
    """types::image::save: min/max normalise, scale to 8 bit, write."""
    a = np.ascontiguousarray(plane, np.float32)
    _check(lib().akz_image_save_plane_png(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


def config_to_json(cfg=None):
    cfg = cfg or Config()
    n = C.c_uint64()
    buf = C.create_string_buffer(1024)
    _check(lib().akz_config_to_json(C.byref(cfg), buf, 1024, C.byref(n)))
    return buf.value.decode()


def config_from_json(text, base=None):
    cfg = base or Config()
    _check(lib().akz_config_from_json(text.encode(), C.byref(cfg)))
    return cfg


def random_seed(s0=42, s1=69):
    """random::default().seed([s0, s1]) for the calling thread: restarts the stream that RANSAC sampling and the
    drawing colours consume ([42, 69] is the state a fresh thread starts with)."""
    _check(lib().akz_random_seed(s0, s1))


def draw_keypoints(rgb, keypoints):
    """types::keypoint::draw_keypoints: returns a new RGB image with the keypoints blended in."""
    out = np.ascontiguousarray(rgb, np.uint8).copy()
    kp = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    _check(lib().akz_draw_keypoints(out.ctypes.data, out.shape[1], out.shape[0], kp.ctypes.data, len(kp)))
    return out


def draw_matches(rgb0, rgb1, keypoints_0, keypoints_1, matches):
    a, b = np.ascontiguousarray(rgb0, np.uint8), np.ascontiguousarray(rgb1, np.uint8)
    k0, k1 = np.ascontiguousarray(keypoints_0, KEYPOINT_DTYPE), np.ascontiguousarray(keypoints_1, KEYPOINT_DTYPE)
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    w, h, px = C.c_uint32(), C.c_uint32(), C.c_void_p()
    _check(lib().akz_draw_matches(a.ctypes.data, a.shape[1], a.shape[0], b.ctypes.data, b.shape[1], b.shape[0],
                                  k0.ctypes.data, len(k0), k1.ctypes.data, len(k1), m.ctypes.data, len(m),
                                  C.byref(w), C.byref(h), C.byref(px)))
    return _take(px, w.value * h.value * 3).reshape(h.value, w.value, 3)


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def extract_features(image, options=None, ctx=None, mask=None):
    """akaze::extract_features(image, options) -> (evolutions, keypoints, descriptors).
    `evolutions` is the ExtractResult (planes fetched lazily), keypoints a structured array,
    descriptors an [n, 61] uint8 array.  mask: a host uint8 / bool array of the image's size, nonzero = detect here
    (akz_extract_gray_u8_masked; the image is then a host uint8 array)."""
    if mask is not None:
        r = (ctx or default_context()).extract_features_masked(image, mask, options)
        return r, r.keypoints(0), r.descriptors(0)
    r = (ctx or default_context()).extract_features(image, options)
    return r, r.keypoints(0), r.descriptors(0)


def serialize_features_to_file(keypoints, descriptors, path):
    """akaze_util::serialize_features_to_file (akaze-util/src/lib.rs:17-30): ".json" -> serde_json, else bincode."""
    k = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    d = np.ascontiguousarray(descriptors, np.uint8).reshape(len(k), -1) if len(k) else np.zeros((0, 61), np.uint8)
    _check(lib().akz_write_features(os.fsencode(path), k.ctypes.data_as(C.c_void_p), len(k),
                                    d.ctypes.data_as(C.c_void_p), d.shape[1]))


def deserialize_features_from_file(path):
    """akaze_util::deserialize_features_from_file (lib.rs:33-42) -> (keypoints, descriptors[n, bytes])."""
    nk, nd, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().akz_read_features(os.fsencode(path), None, None, 0, 0, C.byref(nk), C.byref(nd), C.byref(nb)))
    k = np.zeros(nk.value, KEYPOINT_DTYPE)
    d = np.zeros((nd.value, nb.value), np.uint8)
    _check(lib().akz_read_features(os.fsencode(path), k.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                   max(1, len(k)), max(1, d.size), C.byref(nk), C.byref(nd), C.byref(nb)))
    return k, d


def serialize_matches_to_file(matches, path):
    """akaze_util::serialize_matches_to_file (lib.rs:44-53)."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    _check(lib().akz_write_matches(os.fsencode(path), m.ctypes.data_as(C.c_void_p), len(m)))


def deserialize_matches_from_file(path):
    """akaze_util::deserialize_matches_from_file (lib.rs:56-67)."""
    n = C.c_uint64()
    _check(lib().akz_read_matches(os.fsencode(path), None, 0, C.byref(n)))
    m = np.zeros(n.value, MATCH_DTYPE)
    _check(lib().akz_read_matches(os.fsencode(path), m.ctypes.data_as(C.c_void_p), max(1, len(m)), C.byref(n)))
    return m


def estimate_fundamental_matrix(keypoints_0, keypoints_1, matches8, epsilon):
    """ops::estimate_fundamental_matrix::estimate_fundamental_matrix (:17-69): 3x3 float32 matrix or None."""
    a = _MatchList(keypoints_0, keypoints_1, matches8)
    if len(a.m) != 8:
        raise ValueError("exactly 8 matches")
    _check(lib().akz_estimate_fundamental_matrix(*a.head[:5], epsilon, *a.model_out))  # (a sample's size is fixed: no n_matches)
    return a.found_model()


def remove_outliers(keypoints_0, keypoints_1, matches, num_trials, epsilon_model, epsilon_inlier):
    """ops::estimate_fundamental_matrix::remove_outliers (estimate_fundamental_matrix.rs:99-165); host only."""
    a = _MatchList(keypoints_0, keypoints_1, matches)
    _check(lib().akz_remove_outliers(*a.head, num_trials, epsilon_model, epsilon_inlier, *a.tail))
    return a.list()


def match_features(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials=None,
                   ransac_epsilon_inliers=None, ctx=None):
    """akaze::match_features (lib.rs:252-275): descriptor_match(d0, d1, 10000, ratio) on the GPU, then — when
    ransac_trials / ransac_epsilon_inliers are given, as in the reference signature — the RANSAC
    fundamental-matrix filter on the host.  Without them only the (bit-exact) descriptor stage runs."""
    c = ctx or default_context()
    if ransac_trials is None:
        return c.descriptor_match(descriptors_0, descriptors_1, 10000, lowes_ratio)
    return _match_pair("", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                       ctx=c)


def _match_pair(model, keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                refine_iterations=None, guided=None, ctx=None):
    """The nine single-pair calls akz_match_features{model}[_refined][_guided] (_match_name), as _match_pairs states their
    pairs forms -> matches for model "", else (matches, model or None), with refine_iterations (matches, model or None, accepted
    fits)."""
    c = ctx or default_context()
    a = _PairArgs(descriptors_0, descriptors_1, keypoints_0, keypoints_1)
    refined = refine_iterations is not None
    fn = getattr(lib(), _match_name(model, refined, guided, False))
    _check(fn(*_match_run((c._h, *a.head), (lowes_ratio, ransac_trials, ransac_epsilon_inliers), (refine_iterations,) if refined else (),
                          guided or (), a.tail, a.model_out if model else (), (C.byref(a.it),) if refined else ())))
    if not model:
        return a.list()
    return (a.list(), a.found_model(), a.it.value) if refined else (a.list(), a.found_model())


def match_features_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, ctx=None):
    """Context.match_features_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers)


# ---- homography RANSAC (an addition; include/akaze_hip.h) ----------------------------------------------------
HOMOGRAPHY_EPSILON_MODEL = 1e-6  # AKZ_HOMOGRAPHY_EPSILON_MODEL: the epsilon_model of the context calls


def estimate_homography(keypoints_0, keypoints_1, matches4, epsilon):
    """The 4-point homography of exactly 4 matches (akz_estimate_homography): 3x3 float32 H with H[2, 2] = 1, or None."""
    a = _MatchList(keypoints_0, keypoints_1, matches4)
    if len(a.m) != 4:
        raise ValueError("exactly 4 matches")
    _check(lib().akz_estimate_homography(*a.head[:5], epsilon, *a.model_out))  # (a sample's size is fixed: no n_matches)
    return a.found_model()


def remove_outliers_homography(keypoints_0, keypoints_1, matches, num_trials, epsilon_model, epsilon_inlier):
    """The homography RANSAC on the host (akz_remove_outliers_homography) -> (matches kept, H or None)."""
    a = _MatchList(keypoints_0, keypoints_1, matches)
    _check(lib().akz_remove_outliers_homography(*a.head, num_trials, epsilon_model, epsilon_inlier, *a.tail, *a.model_out))
    return a.list(), a.found_model()


def match_features_homography(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                              ransac_epsilon_inliers, ctx=None):
    """descriptor_match(d0, d1, 10000, ratio), then the homography RANSAC, all on the GPU (akz_match_features_homography)
    -> (matches kept, H or None); equal to remove_outliers_homography(k0, k1, that list, ransac_trials,
    HOMOGRAPHY_EPSILON_MODEL, ransac_epsilon_inliers) from the same random state."""
    return _match_pair("_homography", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, ctx=ctx)


def match_features_homography_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, ctx=None):
    """Context.match_features_homography_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_homography_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                      ransac_epsilon_inliers)


# ---- guided matching (an addition; include/akaze_hip.h) -------------------------------------------------------
GUIDED_HOMOGRAPHY = 0   # AKZ_GUIDED_HOMOGRAPHY: the model is H, the gate a disc around the transferred point
GUIDED_FUNDAMENTAL = 1  # AKZ_GUIDED_FUNDAMENTAL: the model is F, the gate a band around the epipolar line


def _guided_pair(fn, first, keypoints_0, descriptors_0, keypoints_1, descriptors_1, model, kind, radius, distance_threshold,
                 lowes_ratio):
    a = _PairArgs(descriptors_0, descriptors_1, keypoints_0, keypoints_1)
    md = np.ascontiguousarray(np.asarray(model, np.float32).reshape(9))
    _check(fn(*first, *a.head, int(kind), md.ctypes.data_as(C.POINTER(C.c_float)), radius, distance_threshold, lowes_ratio, *a.tail))
    return a.list()


def descriptor_match_guided_host(keypoints_0, descriptors_0, keypoints_1, descriptors_1, model, kind, radius,
                                 distance_threshold=10000, lowes_ratio=0.86):
    """descriptor_match in which descriptor j of set 1 competes for descriptor i of set 0 only if keypoint j lies within
    `radius` pixels of where the model sends keypoint i (kind GUIDED_HOMOGRAPHY: model = H, the transferred point;
    GUIDED_FUNDAMENTAL: model = F, the epipolar line).  The plain host statement (akz_descriptor_match_guided_host)."""
    return _guided_pair(lib().akz_descriptor_match_guided_host, (), keypoints_0, descriptors_0, keypoints_1, descriptors_1, model, kind,
                        radius, distance_threshold, lowes_ratio)


def descriptor_match_guided(keypoints_0, descriptors_0, keypoints_1, descriptors_1, model, kind, radius, distance_threshold=10000,
                            lowes_ratio=0.86, ctx=None):
    """descriptor_match_guided_host on the GPU (akz_descriptor_match_guided): the same list, bit for bit."""
    c = ctx or default_context()
    return _guided_pair(lib().akz_descriptor_match_guided, (c._h,), keypoints_0, descriptors_0, keypoints_1, descriptors_1, model, kind,
                        radius, distance_threshold, lowes_ratio)


def descriptor_match_guided_pairs(features, pairs, models, kind, radius, distance_threshold=10000, lowes_ratio=0.86, ctx=None):
    """Context.descriptor_match_guided_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).descriptor_match_guided_pairs(features, pairs, models, kind, radius, distance_threshold,
                                                                    lowes_ratio)


def match_features_homography_guided(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                     ransac_epsilon_inliers, guided_radius, guided_lowes_ratio, ctx=None):
    """match_features_homography, then the guided scan with the H it found (akz_match_features_homography_guided) ->
    (matches, H or None): with an H the guided list, without one the list of match_features_homography."""
    return _match_pair("_homography", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, guided=(guided_radius, guided_lowes_ratio), ctx=ctx)


def match_features_homography_guided_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, guided_radius,
                                           guided_lowes_ratio, ctx=None):
    """Context.match_features_homography_guided_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_homography_guided_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                             ransac_epsilon_inliers, guided_radius, guided_lowes_ratio)


# ---- the refit of the RANSAC homography on its inliers (an addition; include/akaze_hip.h) ---------------------
def refine_homography(keypoints_0, keypoints_1, matches, h, epsilon_inlier, max_iterations):
    """Local optimisation of the homography h over a raw match list on the host (akz_refine_homography): least-squares refits
    on the inliers and re-classification until the set stops growing -> (inliers in match order, 3x3 float32 H, accepted
    fits).  With 0 accepted fits H is h and the list its inliers."""
    return _refine(lib().akz_refine_homography, keypoints_0, keypoints_1, matches, h, epsilon_inlier, max_iterations)


def _refine(fn, keypoints_0, keypoints_1, matches, model, epsilon_inlier, max_iterations):
    """a refit on the host -> (inliers in match order, the 3x3 model, accepted fits)"""
    a = _MatchList(keypoints_0, keypoints_1, matches, model)
    _check(fn(*a.head, epsilon_inlier, max_iterations, *a.tail, a.model_out[0], C.byref(a.it)))
    return a.list(), a.model.reshape(3, 3), a.it.value


def match_features_homography_refined(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                      ransac_epsilon_inliers, refine_iterations, ctx=None):
    """match_features_homography with the refit of the H it found as one more stage on the GPU
    (akz_match_features_homography_refined) -> (matches, H or None, accepted fits): with an H what refine_homography gives on
    the raw descriptor_match list from the winner, without one the list of match_features_homography."""
    return _match_pair("_homography", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, refine_iterations, ctx=ctx)


def match_features_homography_refined_guided(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                             ransac_epsilon_inliers, refine_iterations, guided_radius, guided_lowes_ratio, ctx=None):
    """match_features_homography_refined, then the guided scan with the REFINED H
    (akz_match_features_homography_refined_guided) -> (matches, H or None, accepted fits)."""
    return _match_pair("_homography", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, refine_iterations, (guided_radius, guided_lowes_ratio), ctx)


def match_features_homography_refined_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations,
                                            ctx=None):
    """Context.match_features_homography_refined_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_homography_refined_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                              ransac_epsilon_inliers, refine_iterations)


def match_features_homography_refined_guided_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                   refine_iterations, guided_radius, guided_lowes_ratio, ctx=None):
    """Context.match_features_homography_refined_guided_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_homography_refined_guided_pairs(
        features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations, guided_radius, guided_lowes_ratio)


# ---- the RANSAC fundamental matrix handed back, refitted and guiding (an addition; include/akaze_hip.h) ---------
FUNDAMENTAL_REFIT_EPSILON = 1e-6  # AKZ_FUNDAMENTAL_REFIT_EPSILON: the rank rule of the refit


def remove_outliers_fundamental(keypoints_0, keypoints_1, matches, num_trials, epsilon_model, epsilon_inlier):
    """remove_outliers with the model that filtered (akz_remove_outliers_fundamental; host only) -> (matches kept, F or None):
    the list and the draws of remove_outliers, F the first trial with the most inliers (3x3 float32, p1^T F p0 = 0)."""
    a = _MatchList(keypoints_0, keypoints_1, matches)
    _check(lib().akz_remove_outliers_fundamental(*a.head, num_trials, epsilon_model, epsilon_inlier, *a.tail, *a.model_out))
    return a.list(), a.found_model()


def refine_fundamental_matrix(keypoints_0, keypoints_1, matches, f, epsilon_inlier, max_iterations):
    """Local optimisation of the fundamental matrix f over a raw match list on the host (akz_refine_fundamental_matrix):
    normalised least-squares refits on the inliers, rank 2 enforced, and re-classification until the set stops growing ->
    (inliers in match order, 3x3 float32 F of unit norm, accepted fits).  With 0 accepted fits F is f and the list its inliers."""
    return _refine(lib().akz_refine_fundamental_matrix, keypoints_0, keypoints_1, matches, f, epsilon_inlier, max_iterations)


def match_features_fundamental(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                               ransac_epsilon_inliers, ctx=None):
    """match_features with the fundamental matrix that filtered (akz_match_features_fundamental) -> (matches kept, F or None);
    equal to remove_outliers_fundamental(k0, k1, descriptor_match(d0, d1, 10000, ratio), ransac_trials, 0.05,
    ransac_epsilon_inliers) from the same random state."""
    return _match_pair("_fundamental", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, ctx=ctx)


def match_features_fundamental_guided(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                      ransac_epsilon_inliers, guided_radius, guided_lowes_ratio, ctx=None):
    """match_features_fundamental, then the guided scan with the F it found (akz_match_features_fundamental_guided) ->
    (matches, F or None): with an F the guided list, without one the list of match_features_fundamental."""
    return _match_pair("_fundamental", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, guided=(guided_radius, guided_lowes_ratio), ctx=ctx)


def match_features_fundamental_refined(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                       ransac_epsilon_inliers, refine_iterations, ctx=None):
    """match_features_fundamental with the refit of the F it found as one more stage on the GPU
    (akz_match_features_fundamental_refined) -> (matches, F or None, accepted fits): with an F what refine_fundamental_matrix
    gives on the raw descriptor_match list from the winner, without one the list of match_features_fundamental."""
    return _match_pair("_fundamental", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, refine_iterations, ctx=ctx)


def match_features_fundamental_refined_guided(keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                                              ransac_epsilon_inliers, refine_iterations, guided_radius, guided_lowes_ratio, ctx=None):
    """match_features_fundamental_refined, then the guided scan with the REFINED F
    (akz_match_features_fundamental_refined_guided) -> (matches, F or None, accepted fits)."""
    return _match_pair("_fundamental", keypoints_0, descriptors_0, keypoints_1, descriptors_1, lowes_ratio, ransac_trials,
                       ransac_epsilon_inliers, refine_iterations, (guided_radius, guided_lowes_ratio), ctx)


def match_features_fundamental_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, ctx=None):
    """Context.match_features_fundamental_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_fundamental_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                       ransac_epsilon_inliers)


def match_features_fundamental_refined_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations,
                                             ctx=None):
    """Context.match_features_fundamental_refined_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_fundamental_refined_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                               ransac_epsilon_inliers, refine_iterations)


def match_features_fundamental_guided_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, guided_radius,
                                            guided_lowes_ratio, ctx=None):
    """Context.match_features_fundamental_guided_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_fundamental_guided_pairs(features, pairs, lowes_ratio, ransac_trials,
                                                                              ransac_epsilon_inliers, guided_radius, guided_lowes_ratio)


def match_features_fundamental_refined_guided_pairs(features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                                    refine_iterations, guided_radius, guided_lowes_ratio, ctx=None):
    """Context.match_features_fundamental_refined_guided_pairs on ctx (default: the default context)."""
    return (ctx or default_context()).match_features_fundamental_refined_guided_pairs(
        features, pairs, lowes_ratio, ransac_trials, ransac_epsilon_inliers, refine_iterations, guided_radius, guided_lowes_ratio)


# ---- seeded RANSAC: samples drawn on the GPU, trials stopped by confidence (an addition; include/akaze_hip.h) ------
RANSAC_ROUND = 128            # AKZ_RANSAC_ROUND: trials per round of the seeded RANSAC
RANSAC_MAX_TRIALS = 1 << 24   # the largest max_trials it accepts


# AKZ_RANSAC_FUNDAMENTAL_NORMALISED: the third model_kind of the seeded calls (the guided calls refuse it) -- the normalised
# 8-point model with rank 2 enforced, epsilon_inliers a Sampson distance in pixels
RANSAC_FUNDAMENTAL_NORMALISED = 3


def estimate_fundamental_normalised(keypoints_0, keypoints_1, matches8):
    """The normalised 8-point fundamental matrix of exactly 8 matches, given in ascending order of their position in the list
    they were sampled from (akz_estimate_fundamental_normalised): 3x3 float32 F of unit norm and rank 2 with p1^T F p0 = 0, or
    None.  It equals one fit of refine_fundamental_matrix over those eight, bit for bit."""
    a = _MatchList(keypoints_0, keypoints_1, matches8)
    if len(a.m) != 8:
        raise ValueError("exactly 8 matches")
    _check(lib().akz_estimate_fundamental_normalised(*a.head[:5], *a.model_out))  # (a sample's size is fixed: no n_matches)
    return a.found_model()


def refine_fundamental_normalised(keypoints_0, keypoints_1, matches, f, epsilon_inlier, max_iterations):
    """refine_fundamental_matrix with the inlier rule of RANSAC_FUNDAMENTAL_NORMALISED: a Sampson distance below epsilon_inlier
    pixels (akz_refine_fundamental_normalised) -> (inliers in match order, 3x3 float32 F, accepted fits)."""
    return _refine(lib().akz_refine_fundamental_normalised, keypoints_0, keypoints_1, matches, f, epsilon_inlier, max_iterations)


def draw_sample_seeded(seed0, seed1, stream, trial, n_matches, k):
    """The sample of trial `trial` of `stream` over n_matches matches (akz_draw_sample_seeded): k (4, 6 or 8) ascending indices."""
    out = np.zeros(8, np.uint64)
    _check(lib().akz_draw_sample_seeded(seed0, seed1, stream, trial, n_matches, k, out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out[:k].copy()


def ransac_required_inliers(n_matches, k, trials, confidence):
    """The inlier count that stops a pair of n_matches matches after `trials` trials (akz_ransac_required_inliers)."""
    need = C.c_uint64()
    _check(lib().akz_ransac_required_inliers(n_matches, k, trials, confidence, C.byref(need)))
    return need.value


def remove_outliers_seeded(keypoints_0, keypoints_1, matches, options=None, stream=0):
    """The seeded RANSAC on the host (akz_remove_outliers_seeded; no GPU call) -> (matches kept, model or None, accepted fits,
    trials run): rounds of 128 trials whose samples are a function of (options.seed, stream, trial), stopped by
    options.confidence, then the filter and, with options.refine_iterations, the refit."""
    a = _MatchList(keypoints_0, keypoints_1, matches)
    opt = options if options is not None else RansacOptions()
    tr = C.c_uint64()
    _check(lib().akz_remove_outliers_seeded(*a.head, C.byref(opt), stream, *a.tail, *a.model_out, C.byref(a.it), C.byref(tr)))
    return a.list(), a.found_model(), a.it.value, tr.value


def _bank_context(features):
    """the context of a FeatureBank given as `features`, else None"""
    return features.ctx if isinstance(features, FeatureBank) else None


def match_features_seeded_pairs(features, pairs, options=None, ctx=None, cross_check=False):
    """Context.match_features_seeded_pairs on ctx (default: a FeatureBank's own context, else the default context)."""
    return (ctx or _bank_context(features) or default_context()).match_features_seeded_pairs(features, pairs, options, cross_check=cross_check)


def match_features_seeded(keypoints_0, descriptors_0, keypoints_1, descriptors_1, options=None, ctx=None, cross_check=False):
    """One pair through match_features_seeded_pairs (its stream: options.stream_base) -> (matches, model or None, accepted
    fits, trials run)."""
    return (ctx or default_context()).match_features_seeded_pairs([(keypoints_0, descriptors_0), (keypoints_1, descriptors_1)],
                                                                  [(0, 1)], options, cross_check=cross_check)[0]


def recover_pose_host(keypoints_0, keypoints_1, matches, f, camera_0, camera_1, points=False):
    """The relative pose behind a fundamental matrix on the host (akz_recover_pose_host; no GPU call): E = K1^T F K0, its four
    (R, t) candidates, the one with the most matches in front of both cameras -> (the matches in front under it, in order -- the
    input unchanged without a pose --, Pose) and, with points=True, the [kept, 3] float32 structure (None without a pose)."""
    a = _MatchList(keypoints_0, keypoints_1, matches, f)
    c0, c1 = Camera.of(camera_0), Camera.of(camera_1)
    pts = np.zeros((len(a.out), 3), np.float32) if points else None
    pose = Pose()
    _check(lib().akz_recover_pose_host(*a.head, C.byref(c0), C.byref(c1), *a.tail, C.byref(pose),
                                       pts.ctypes.data_as(C.POINTER(C.c_float)) if points else None))
    if points:
        return a.list(), pose, (pts[:a.n.value].copy() if pose.found else None)
    return a.list(), pose


def match_features_seeded_pose_pairs(features, cameras, pairs, options=None, ctx=None, cross_check=False, points=False):
    """Context.match_features_seeded_pose_pairs on ctx (default: a FeatureBank's own context, else the default context)."""
    return (ctx or _bank_context(features) or default_context()).match_features_seeded_pose_pairs(features, cameras, pairs, options,
                                                                                                  cross_check=cross_check, points=points)


def match_features_seeded_pose(keypoints_0, descriptors_0, camera_0, keypoints_1, descriptors_1, camera_1, options=None, ctx=None,
                               cross_check=False, points=False):
    """One pair through match_features_seeded_pose_pairs (its stream: options.stream_base) -> (matches, model or None, accepted
    fits, trials run, Pose[, points])."""
    return (ctx or default_context()).match_features_seeded_pose_pairs([(keypoints_0, descriptors_0), (keypoints_1, descriptors_1)],
                                                                       [camera_0, camera_1], [(0, 1)], options, cross_check=cross_check,
                                                                       points=points)[0]


# ---- absolute pose: seeded 6-point resection RANSAC (an addition; include/akaze_hip.h) ----------------------------
# AKZ_RANSAC_RESECTION: the model_kind of the resection calls and of no other -- x_cam = R X + t from 2D-3D correspondences,
# epsilon_inliers a reprojection error in pixels
RANSAC_RESECTION = 4


def estimate_resection(points6, pixels6, camera):
    """The resection model of exactly 6 correspondences, given in ascending order of their position in the problem they were
    sampled from (akz_estimate_resection) -> Resection; found = 0 (all zeros) where the sample has no model -- coplanar points
    among them: the DLT cannot do a plane."""
    pts = np.ascontiguousarray(np.asarray(points6, np.float32).reshape(-1, 3))
    pix = np.ascontiguousarray(np.asarray(pixels6, np.float32).reshape(-1, 2))
    if len(pts) != 6 or len(pix) != 6:
        raise ValueError("exactly 6 correspondences")
    fp, cam, pose = C.POINTER(C.c_float), Camera.of(camera), Resection()
    _check(lib().akz_estimate_resection(pts.ctypes.data_as(fp), pix.ctypes.data_as(fp), C.byref(cam), C.byref(pose), None))
    return pose


def refine_resection(points, pixels, camera, pose, epsilon, max_iterations):
    """The refit of a resection on its inliers, on the host (akz_refine_resection): the loop of refine_homography from pose's R
    and t with epsilon in pixels -> (kept indices ascending, Resection, accepted fits)."""
    a = _ResectionArgs([(points, pixels, camera)])
    kept, n_kept, out, its, _ = a.tail()
    _check(lib().akz_refine_resection(a.problems, C.byref(pose), epsilon, max_iterations, kept, n_kept, C.cast(out, C.POINTER(Resection)), its))
    return a.results()[0][:3]


def resection_seeded_host(points, pixels, camera, options, stream=0):
    """The seeded resection RANSAC of one problem on the host (akz_resection_seeded_host; no GPU call) -> (kept indices
    ascending, Resection, accepted fits, trials run)."""
    a = _ResectionArgs([(points, pixels, camera)])
    _check(lib().akz_resection_seeded_host(a.problems, C.byref(options), stream, *a.tail()))
    return a.results()[0]


def correspondences_2d3d(matches_ab, points_ab, matches_ac, keypoints_c):
    """The join that makes the pose call's points usable for a third image: matches_ab and points_ab are the kept matches of a
    pair (A, B) and their structure (match_features_seeded_pose_pairs(..., points=True)), matches_ac a match list of (A, C) and
    keypoints_c C's keypoints.  For every record of matches_ac whose index_0 occurs in matches_ab (its FIRST occurrence there),
    that record's point and C's pixel -> (points [k, 3] float32, pixels [k, 2] float32, the k record indices into matches_ab,
    the k record indices into matches_ac), in matches_ac's order."""
    first = {}
    for i, a in enumerate(np.asarray(matches_ab["index_0"], np.uint64).tolist()):
        first.setdefault(a, i)
    ab, ac = [], []
    for j, a in enumerate(np.asarray(matches_ac["index_0"], np.uint64).tolist()):
        if a in first:
            ab.append(first[a])
            ac.append(j)
    ab, ac = np.asarray(ab, np.int64), np.asarray(ac, np.int64)
    kc = np.asarray(keypoints_c)
    at = np.asarray(matches_ac["index_1"], np.int64)[ac]
    pix = np.stack([kc["x"][at], kc["y"][at]], axis=1).astype(np.float32) if len(ac) else np.zeros((0, 2), np.float32)
    pts = np.asarray(points_ab, np.float32).reshape(-1, 3)[ab]
    return np.ascontiguousarray(pts), np.ascontiguousarray(pix), ab, ac


def _descriptor_pair(fn, first, d0, d1, distance_threshold, lowes_ratio):
    """descriptor_match and its cross-checked forms over two host descriptor arrays -> the list"""
    a = _PairArgs(d0, d1)
    _check(fn(*first, *a.head, distance_threshold, lowes_ratio, *a.tail))
    return a.list()


def _knn_pair(fn, first, d0, d1, k, distance_threshold):
    a = _PairArgs(d0, d1, null_empty=True)
    k = int(k)
    out = np.zeros((a.n0, max(k, 0)), MATCH_DTYPE)
    counts = np.zeros(a.n0, np.uint32)
    pad_out = out if out.size else np.zeros(1, MATCH_DTYPE)        # (never written: there is no row to write for)
    pad_cnt = counts if counts.size else np.zeros(1, np.uint32)
    _check(fn(*first, *a.head, k, distance_threshold, pad_out.ctypes.data_as(C.c_void_p), pad_cnt.ctypes.data_as(C.c_void_p)))
    return out, counts


def descriptor_match_knn_host(d0, d1, k, distance_threshold=10000):
    """k-nearest-neighbour matching on the host (akz_descriptor_match_knn_host; no GPU call): for every row of d0 the rows of d1
    with hamming distance < distance_threshold, ordered by (distance, index), the first k of them -> (records (n0, k) in
    MATCH_DTYPE, counts (n0,) uint32); unused slots hold index_1 = 2^64 - 1 and distance = inf.  The statement that
    Context.descriptor_match_knn and descriptor_match_knn_device are held to."""
    return _knn_pair(lib().akz_descriptor_match_knn_host, (), d0, d1, k, distance_threshold)


def keypoint_budget_host(keypoints, max_keypoints, mode=BUDGET_SPREAD, robust=0.9):
    """The keypoint budget on the host (akz_keypoint_budget_host; no GPU call): the first min(max_keypoints, n) keypoints in the
    order (response descending, index ascending) of BUDGET_STRONGEST or (suppression radius descending, response descending,
    index ascending) of BUDGET_SPREAD, reported in ascending index order -> (indices uint64, radius2 float32 [n] or None in
    BUDGET_STRONGEST mode).  The statement that Context.keypoint_budget_sets is held to."""
    k = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    opt = KeypointBudget(int(max_keypoints), int(mode), float(robust))
    idx = np.zeros(max(1, len(k)), np.uint64)
    n = C.c_uint64()
    rad = np.zeros(max(1, len(k)), np.float32) if mode == BUDGET_SPREAD else None
    _check(lib().akz_keypoint_budget_host(k.ctypes.data_as(C.c_void_p) if len(k) else None, len(k), C.byref(opt),
                                          idx.ctypes.data_as(C.c_void_p), C.byref(n),
                                          rad.ctypes.data_as(C.c_void_p) if rad is not None else None))
    return idx[:n.value].copy(), (rad[:len(k)].copy() if rad is not None else None)


def keypoint_budget_tiles():
    """akz_debug_keypoint_budget_tiles: (queries per workgroup, keypoints per LDS stage) of the budget's tile walk."""
    q, t = C.c_uint32(), C.c_uint32()
    _check(lib().akz_debug_keypoint_budget_tiles(C.byref(q), C.byref(t)))
    return q.value, t.value


def limit_features(keypoints, descriptors, max_keypoints, mode=BUDGET_SPREAD, robust=0.9, ctx=None):
    """Cut a feature set to at most max_keypoints with Context.keypoint_budget_sets on ctx (default: the default context) ->
    (keypoints[idx], descriptors[idx], idx), in the detector's order and ready for every match_features* call."""
    k = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    d = np.asarray(descriptors)
    if len(d) != len(k):
        raise ValueError(f"{len(k)} keypoints but {len(d)} descriptors")
    idx, _ = (ctx or default_context()).keypoint_budget_sets([k], max_keypoints, mode, robust)[0]
    sel = idx.astype(np.int64)
    return k[sel].copy(), np.ascontiguousarray(d[sel]), idx


def descriptor_match_cross_host(d0, d1, distance_threshold=10000, lowes_ratio=0.86):
    """The cross-check on the host (akz_descriptor_match_cross_host; no GPU call): m of descriptor_match(d0, d1) is kept iff
    descriptor_match(d1, d0) holds the record with index_0 == m.index_1 and index_1 == m.index_0.  The statement that
    Context.descriptor_match_cross and the cross_check of the seeded calls are held to."""
    return _descriptor_pair(lib().akz_descriptor_match_cross_host, (), d0, d1, distance_threshold, lowes_ratio)


# ------------------------------------------------------------------------------------------
# multi-GPU: per-image sharding and the one exchange step of the path
# ------------------------------------------------------------------------------------------
def shard_frames(num_frames, rank, world_size):
    """Frame indices owned by `rank`: image i -> GPU i mod G; extraction needs no
    collective."""
    return list(range(rank, num_frames, world_size))


COMM_ID_BYTES = 128


def comm_unique_id():
    """akz_comm_unique_id: rank 0 creates it, every rank receives the same 128 bytes (any transport)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().akz_comm_unique_id(buf))
    return bytes(buf)


class Gather:
    """One exchange in flight (akz_gather_begin*): finish() waits on the host, stream_wait() makes a stream wait."""

    def __init__(self, comm, handle):
        self._comm, self._h = comm, handle
        comm._gathers.add(self)  # akz_comm_destroy deletes its gather objects: Comm.close() invalidates the handles

    def stream_wait(self, stream):
        _check(lib().akz_gather_stream_wait(self._h, C.c_void_p(stream)))

    def blocks(self):
        """akz_gather_blocks (external transport): (device address of this rank's block, device address where the blocks of
        all ranks go, bytes per block)."""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().akz_gather_blocks(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def deliver(self, stream=None):
        """akz_gather_deliver: every rank's block has been written where blocks() said, in the order of `stream`."""
        _check(lib().akz_gather_deliver(self._h, C.c_void_p(stream) if stream else None))

    def plan_all_pairs(self):
        """akz_pairs_plan: who matches what (akz_match_all_pairs' holder map and lead sets) without matching -- host arithmetic."""
        p = C.c_void_p()
        _check(lib().akz_pairs_plan(self._h, C.byref(p)))
        return Pairs(None, p)

    def exchange_over(self, group=None):
        """External transport over torch.distributed (any backend; gloo in the one-GPU rehearsals): this rank's block D2H,
        one all-gather of the fixed-size blocks, H2D, deliver.  Synchronous.  On a HOST communicator the blocks ARE host
        memory: the all-gather runs on them in place."""
        import torch
        import torch.distributed as dist
        send, recv, nbytes = self.blocks()
        world = self._comm.nranks
        if self._comm.host:
            h_send = torch.from_numpy(np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,)))
            h_recv = torch.from_numpy(np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(world * nbytes,)))
            if world == 1 and not dist.is_initialized():
                h_recv.copy_(h_send)
            else:
                dist.all_gather_into_tensor(h_recv, h_send, group=group)
            self.deliver()
            return
        if world == 1 and not dist.is_initialized():  # a single rank without a process group: its block is the job
            copy_raw(recv, send, nbytes, 3)
            self.deliver()
            return
        stage = self._comm.__dict__.setdefault("_stage", {})   # pinned staging, kept per block size (pinning costs milliseconds)
        if stage.get("nbytes") != nbytes:
            stage.update(nbytes=nbytes, send=torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
                         recv=torch.empty(world * nbytes, dtype=torch.uint8).pin_memory())
        h_send, h_recv = stage["send"], stage["recv"]
        copy_raw(h_send.data_ptr(), send, nbytes, 2)       # D2H
        dist.all_gather_into_tensor(h_recv, h_send, group=group)
        copy_raw(recv, h_recv.data_ptr(), world * nbytes, 1)  # H2D
        self.deliver()

    def finish(self, want_counts=True):
        """-> (device address of the blocks, rows per block, counts per rank, images per rank); rank r's descriptor
        rows start one 64-byte row into block r."""
        p, br = C.c_void_p(), C.c_uint64()
        n = self._comm.nranks
        cnt, img = (C.c_uint64 * n)(), (C.c_uint64 * n)()
        _check(lib().akz_gather_finish(self._h, C.byref(p), C.byref(br), cnt if want_counts else None,
                                       img if want_counts else None))
        return p.value, br.value, list(cnt), list(img)

    def image_rows(self, rank):
        """akz_gather_image_rows: rows of every image of `rank`'s shard (after finish())."""
        n = C.c_uint64()
        _check(lib().akz_gather_image_rows(self._h, int(rank), None, 0, C.byref(n)))
        out = (C.c_uint64 * max(1, n.value))()
        _check(lib().akz_gather_image_rows(self._h, int(rank), out, n.value, C.byref(n)))
        return [int(v) for v in out[:n.value]]

    def match_all_pairs(self, ctx, distance_threshold=10000, lowes_ratio=0.86):
        """akz_match_all_pairs (BASELINE configs[4]): every unordered image pair once, both directions, on the rank that owns
        the pair's lead image (Pairs.holder)."""
        p = C.c_void_p()
        _check(lib().akz_match_all_pairs(ctx._h, self._h, int(distance_threshold), float(lowes_ratio), C.byref(p)))
        return Pairs(ctx, p)

    def free(self):
        if self._h:
            lib().akz_gather_free(self._h)
            self._h = None
        self._comm._gathers.discard(self)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Pairs:
    """Result of akz_match_all_pairs: both match lists of every image pair this rank holds (Pairs.holder / held)."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle  # (the context must outlive the pairs object)
        n, f, o = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().akz_pairs_info(self._h, C.byref(n), C.byref(f), C.byref(o)))
        self.n_images, self.first_owned, self.n_owned = n.value, f.value, o.value

    def image_rows(self, image):
        r, o = C.c_uint64(), C.c_int32()
        _check(lib().akz_pairs_image_rows(self._h, int(image), C.byref(r), C.byref(o)))
        return r.value, o.value

    def count(self, query, image):
        n = C.c_uint64()
        _check(lib().akz_pairs_matches(self._h, int(query), int(image), None, 0, C.byref(n)))
        return n.value

    def matches(self, query, image):
        n = self.count(query, image)
        out = np.zeros(max(n, 1), MATCH_DTYPE)
        m = C.c_uint64()
        _check(lib().akz_pairs_matches(self._h, int(query), int(image), out.ctypes.data_as(C.c_void_p), n, C.byref(m)))
        return out[:m.value].copy()

    def holder(self, a, b):
        """akz_pairs_holder: the rank whose Pairs object holds both lists of the pair {a, b}."""
        r = C.c_int32()
        _check(lib().akz_pairs_holder(self._h, int(a), int(b), C.byref(r)))
        return r.value

    def held(self, rank):
        """ordered pairs (query, image) whose lists this rank holds"""
        return [(a, b) for a in range(self.n_images) for b in range(self.n_images) if a != b and self.holder(a, b) == rank]

    def lead_sets(self, lead_image):
        """akz_pairs_lead_sets: the images this rank matches `lead_image` (one it owns) against"""
        n = C.c_uint64()
        _check(lib().akz_pairs_lead_sets(self._h, int(lead_image), None, 0, C.byref(n)))
        out = (C.c_uint64 * max(1, n.value))()
        _check(lib().akz_pairs_lead_sets(self._h, int(lead_image), out, n.value, C.byref(n)))
        return [int(v) for v in out[:n.value]]

    def total_matches(self, rank=0):
        return sum(self.count(a, b) for a, b in self.held(rank))

    def totals(self):
        """akz_pairs_totals: (match lists held, records in them, descriptor pairs whose distance was formed); waits for the
        launches."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().akz_pairs_totals(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def free(self):
        if self._h:
            lib().akz_pairs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """Communicator of the descriptor exchange behind the C ABI (akz_comm_*): one per rank.  unique_id = the bytes of
    comm_unique_id() from rank 0: RCCL carries the blocks (akz_comm_create); unique_id = None: the caller does
    (akz_comm_create_external; Gather.blocks / Gather.deliver)."""

    HOST = -1  # AKZ_COMM_HOST: an external-transport communicator whose blocks and rows are HOST memory (no GPU call)

    def __init__(self, device, unique_id, rank, nranks):
        self._h = C.c_void_p()
        self.external = unique_id is None
        self.host = self.external and int(device) == Comm.HOST
        if self.external:
            _check(lib().akz_comm_create_external(int(device), int(rank), int(nranks), C.byref(self._h)))
        else:
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
            _check(lib().akz_comm_create(int(device), buf, int(rank), int(nranks), C.byref(self._h)))
        self.rank, self.nranks, self.device = int(rank), int(nranks), int(device)

    def set_timeout(self, seconds):
        """akz_comm_set_timeout: how long finish() waits for an exchange before AKZ_ERR_TIMEOUT (0: without limit)."""
        _check(lib().akz_comm_set_timeout(self._h, float(seconds)))

    def place_streams(self, ctx):
        """akz_comm_place_streams: the communicator's streams onto queues / pipes that the context's busy streams do not use
        (once, before the first step)."""
        _check(lib().akz_comm_place_streams(self._h, ctx._h))

    @property
    def _gathers(self):
        import weakref
        if "_gs" not in self.__dict__:
            self.__dict__["_gs"] = weakref.WeakSet()
        return self.__dict__["_gs"]

    def close(self):
        if self._h:
            for g in list(self._gathers):  # exchanges still held by the caller: retire them while their objects exist
                g.free()
            lib().akz_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gather_begin(self, results, cap_rows):
        """Enqueue the all-gather of the descriptor rows of `results` (ExtractResults of this rank, in order); returns
        once the local rows are copied, never waits for the collective."""
        arr = (C.c_void_p * max(1, len(results)))(*[r._h for r in results])
        g = C.c_void_p()
        _check(lib().akz_gather_begin(self._h, arr, len(results), int(cap_rows), C.byref(g)))
        return Gather(self, g)

    def gather_begin_rows(self, rows, cap_rows, producer_stream=None):
        """The same for a torch CUDA uint8 tensor [n, 64] that is complete in the order of producer_stream."""
        g = C.c_void_p()
        n = int(rows.shape[0])
        _check(lib().akz_gather_begin_rows(self._h, C.c_void_p(rows.data_ptr()) if n else None, n, int(cap_rows),
                                           C.c_void_p(producer_stream) if producer_stream else None, C.byref(g)))
        gg = Gather(self, g)
        gg._keep = rows
        return gg

    def gather_begin_image_rows(self, rows, rows_per_image, cap_rows, producer_stream=None):
        """akz_gather_begin_image_rows: the rows of several images back to back -- a torch CUDA uint8 tensor [n, 64], or, on a
        HOST communicator, a C-contiguous numpy uint8 array [n, 64]."""
        g = C.c_void_p()
        per = (C.c_uint64 * max(1, len(rows_per_image)))(*[int(v) for v in rows_per_image])
        n = int(rows.shape[0])
        assert n == sum(int(v) for v in rows_per_image)
        ptr = (rows.ctypes.data if self.host else rows.data_ptr()) if n else None
        _check(lib().akz_gather_begin_image_rows(self._h, C.c_void_p(ptr) if n else None, per, len(rows_per_image), int(cap_rows),
                                                 C.c_void_p(producer_stream) if producer_stream else None, C.byref(g)))
        gg = Gather(self, g)
        gg._keep = rows
        return gg

    def gather_descriptors(self, rows):
        """akz_gather_descriptors: synchronous; -> (torch uint8 [sum, 64] copy, counts)."""
        import torch
        n = int(rows.shape[0])
        p = C.c_void_p()
        cnt = (C.c_uint64 * self.nranks)()
        torch.cuda.current_stream(rows.device).synchronize()
        _check(lib().akz_gather_descriptors(self._h, C.c_void_p(rows.data_ptr()) if n else None, n, C.byref(p), cnt))
        counts = [int(v) for v in cnt]
        total = sum(counts)
        out = torch.empty((total, 64), dtype=torch.uint8, device=rows.device)
        if total:
            copy_d2d(out.data_ptr(), p.value, total * 64)
        return out, counts


_hip_memcpy = None
_hip_stream_sync = None


def copy_raw(dst, src, nbytes, kind):
    """hipMemcpy through the HIP runtime torch already loaded, COMPLETE on return (binding helper); kind 1 H2D, 2 D2H,
    3 D2D.  (A device-to-device hipMemcpy may return before the copy has run -- it is enqueued on the null stream, which work
    on a non-blocking stream does not wait for -- so that kind is followed by a synchronisation of the null stream.)"""
    global _hip_memcpy, _hip_stream_sync
    if _hip_memcpy is None:
        import torch
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        fn = hip.hipMemcpy
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        fn.restype = C.c_int
        sy = hip.hipStreamSynchronize
        sy.argtypes = [C.c_void_p]
        sy.restype = C.c_int
        _hip_memcpy, _hip_stream_sync = fn, sy
    if _hip_memcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, int(kind)) != 0:
        raise AkazeError(-2, "hipMemcpy failed")
    if int(kind) == 3 and _hip_stream_sync(None) != 0:
        raise AkazeError(-2, "hipStreamSynchronize failed")


def copy_d2d(dst, src, nbytes):
    """Synchronous device-to-device copy (binding helper)."""
    copy_raw(dst, src, nbytes, 3)


def gather_descriptor_rows(local_rows, group=None, cap_rows=None):
    """All-gather of 64-byte descriptor rows before a cross-image brute-force match: every rank
    contributes a [n_r, 64] uint8 tensor (any n_r >= 0).  Two collectives: the row counts, then the rows
    padded to a common capacity.  With the "nccl" backend this is RCCL over xGMI; tensors stay on the GPU.

    cap_rows=None: capacity = the largest shard (needs one host sync to read the counts); returns
    ([sum n_r, 64] rows in rank order, counts per rank as a list).
    cap_rows=int:  fixed capacity, NO host synchronisation — returns the padded [world, cap_rows, 64]
    tensor and the device tensor of counts; rows beyond a rank's count are zero.  A shard that does not fit
    contributes no rows: its count (> cap_rows, seen by every rank) says so and the caller repeats the
    exchange with a larger capacity on every rank."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    dev = local_rows.device
    n_local = int(local_rows.shape[0])
    cnt = torch.tensor([n_local], dtype=torch.int64, device=dev)
    cnts = torch.zeros(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(cnts, cnt, group=group)
    if cap_rows is not None:
        # a shard that does not fit still takes part (a rank that skipped the collective would leave its peers waiting
        # in it): it contributes no rows, and every rank sees the overflow in the gathered counts
        padded = torch.zeros((cap_rows, 64), dtype=torch.uint8, device=dev)
        if 0 < n_local <= cap_rows:
            padded[:n_local] = local_rows
        gathered = torch.empty((world * cap_rows, 64), dtype=torch.uint8, device=dev)
        dist.all_gather_into_tensor(gathered, padded, group=group)
        return gathered.view(world, cap_rows, 64), cnts
    counts = [int(v) for v in cnts.tolist()]
    cap = max(max(counts), 1)
    padded = torch.zeros((cap, 64), dtype=torch.uint8, device=dev)
    if n_local:
        padded[:n_local] = local_rows
    gathered = torch.empty((world * cap, 64), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(gathered, padded, group=group)
    rows = torch.cat([gathered[r * cap:r * cap + counts[r]] for r in range(world)], dim=0)
    return rows, counts


def gather_descriptor_sets(local_sets, group=None):
    """The exchange step of a cross-GPU all-pairs match (BASELINE configs[4]): every rank
    contributes the descriptor rows of ITS images ([n_i, 64] uint8 tensors, in its shard order); afterwards every
    rank holds every image's rows.  Three all-gathers (images per rank, rows per image, the rows); with the "nccl"
    backend they are RCCL over xGMI and the tensors stay on the GPU.

    Returns (sets, owners): one rows tensor per image of the whole job, rank-major, and the rank that owns it."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    dev = local_sets[0].device if local_sets else torch.device("cpu")
    n_img = torch.tensor([len(local_sets)], dtype=torch.int64, device=dev)
    imgs = torch.zeros(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(imgs, n_img, group=group)
    imgs = [int(v) for v in imgs.tolist()]
    cap = max(max(imgs), 1)
    mine = torch.zeros(cap, dtype=torch.int64, device=dev)
    if local_sets:
        mine[:len(local_sets)] = torch.tensor([int(t.shape[0]) for t in local_sets], dtype=torch.int64, device=dev)
    per_img = torch.zeros(world * cap, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(per_img, mine, group=group)
    per_img = per_img.view(world, cap).tolist()
    local = torch.cat(local_sets, dim=0) if local_sets else torch.zeros((0, 64), dtype=torch.uint8, device=dev)
    rows, _ = gather_descriptor_rows(local, group)
    sets, owners, pos = [], [], 0
    for r in range(world):
        for i in range(imgs[r]):
            n = int(per_img[r][i])
            sets.append(rows[pos:pos + n])
            owners.append(r)
            pos += n
    return sets, owners


def pairs_lead(a, b):
    """The image of the unordered pair {a, b} that serves as the query set of its block (akz_match_all_pairs' rule: the
    lower one if the indices differ by an odd number, else the higher one -- every image leads about half of its pairs)."""
    lo, hi = min(a, b), max(a, b)
    return lo if (hi - lo) & 1 else hi


def all_pairs_match(local_sets, match_fn, group=None, match_sets_fn=None):
    """Cross-GPU all-pairs Hamming match: after gather_descriptor_sets every UNORDERED image pair is matched once, in both
    directions, by the rank that owns the pair's lead image (pairs_lead); nothing else is exchanged.  match_fn(rows_i,
    rows_j) is Context.descriptor_match_device on the GPUs.  With match_sets_fn(rows_i, train_rows, rows_per_set) ->
    ([matches of rows_i against set 0, ...], [matches of set 0 against rows_i, ...]) (Context.
    descriptor_match_sets_mutual_device: one launch per lead image, both directions from one pass) match_fn is not called.

    Returns {(i, j): matches} for the ordered pairs this rank holds, i and j being global (rank-major) image indices."""
    import torch
    import torch.distributed as dist
    sets, owners = gather_descriptor_sets(local_sets, group)
    rank = dist.get_rank(group)
    out = {}
    for i, owner in enumerate(owners):
        if owner != rank:
            continue
        led = [j for j in range(len(sets)) if j != i and pairs_lead(i, j) == i]
        if not led:
            continue
        if match_sets_fn is not None:
            fwd, rev = match_sets_fn(sets[i], torch.cat([sets[j] for j in led], dim=0), [int(sets[j].shape[0]) for j in led])
            for k, j in enumerate(led):
                out[(i, j)] = fwd[k]
                out[(j, i)] = rev[k]
            continue
        for j in led:
            out[(i, j)] = match_fn(sets[i], sets[j])
            out[(j, i)] = match_fn(sets[j], sets[i])
    return out

