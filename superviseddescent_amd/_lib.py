"""ctypes binding of the C-ABI in ``include/sdm.h`` (libsdm_hip.so, gfx950 only).

There is deliberately no CPU fallback: :func:`lib` raises if the shared library was not built, and
:class:`Context` raises if no MI355X is visible.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDM_HIP_LIB") or os.path.join(_HERE, "lib", "libsdm_hip.so")

SDM_OK = 0
SDM_ERR_INVALID, SDM_ERR_NO_DEVICE, SDM_ERR_HIP, SDM_ERR_EMPTY_PATCH, SDM_ERR_NOT_SPD, SDM_ERR_COMM = \
    -1, -2, -3, -4, -5, -6
SDM_T_HOG, SDM_T_APPLY, SDM_T_GRAM, SDM_T_REG, SDM_T_FACTOR, SDM_T_BACKSOLVE, SDM_T_ALLREDUCE = range(7)
SDM_T_COUNT = 8
SDM_HOG_EXACT_ORDER, SDM_HOG_FAST, SDM_HOG_COLUMNS = 0, 1, 2
TIMING_NAMES = ["hog", "apply", "gram", "reg", "factor_solve", "backsolve", "allreduce", "_"]

# every symbol include/sdm.h declares (checked by tests/test_capi_symbols.py without a GPU)
EXPORTED = [
    "sdm_last_error", "sdm_device_count", "sdm_create", "sdm_destroy", "sdm_set_stream", "sdm_synchronize",
    "sdm_set_model_geometry", "sdm_set_hog_mode", "sdm_get_hog_info", "sdm_feature_dim", "sdm_upload_images_u8", "sdm_set_images_device",
    "sdm_set_sample_image_index", "sdm_set_x", "sdm_get_x", "sdm_set_x_device", "sdm_get_x_device",
    "sdm_hog_features", "sdm_get_patch_indices", "sdm_set_regressor", "sdm_get_regressor", "sdm_apply",
    "sdm_detect_batch", "sdm_detect_level", "sdm_set_targets", "sdm_gram_rhs", "sdm_set_allreduce", "sdm_set_allreduce_rccl", "sdm_allreduce_gram_rhs",
    "sdm_set_solve_sharding", "sdm_set_solve_sharding_rccl", "sdm_set_reduce_scatter", "sdm_set_reduce_scatter_rccl",
    "sdm_set_templates", "sdm_init_from_boxes", "sdm_normalised_errors", "sdm_solve", "sdm_set_solver", "sdm_last_rank", "sdm_solve_normal_equations", "sdm_solve_normal_equations_with", "sdm_train_level", "sdm_gram_device_ptr", "sdm_x_device_ptr", "sdm_features_device_ptr",
    "sdm_enable_timing", "sdm_get_timing", "sdm_debug_patch", "sdm_debug_hog_profile", "sdm_debug_gradient_table", "sdm_debug_update_f16", "sdm_debug_set_option",
    "sdm_debug_set_hog_packing", "sdm_debug_gram_fallbacks", "sdm_debug_update_fallbacks", "sdm_debug_hog_plan", "sdm_debug_hog_plan_cut", "sdm_debug_hog_plan_columns", "sdm_debug_hog_band_weights", "sdm_debug_hog_taps", "sdm_debug_hog_pair_taps", "sdm_debug_set_detect_path", "sdm_upload_images_bgr_u8", "sdm_debug_download_images",
    "sdm_pose_set_model", "sdm_pose_set_x", "sdm_pose_get_x", "sdm_pose_set_x_device", "sdm_pose_set_templates",
    "sdm_pose_templates_from_landmarks", "sdm_pose_set_targets", "sdm_pose_features", "sdm_pose_train_level",
    "sdm_pose_set_regressor", "sdm_pose_get_regressor", "sdm_pose_test",
    "sdm_track_configure", "sdm_track_start", "sdm_track_stop", "sdm_track_step", "sdm_track_get",
    "sdm_align_set_source", "sdm_align_crops", "sdm_align_set_source_frames", "sdm_align_crops_tensor", "sdm_align_crops_tensor_filtered",
    "sdm_train_level_sweep", "sdm_sweep_get_regressor",
    "sdm_set_frames_device", "sdm_set_frames_device_planes", "sdm_debug_download_image",
    "sdm_upright_configure", "sdm_detect_batch_upright", "sdm_upright_get", "sdm_track_configure_upright", "sdm_track_start_rolled",
    "sdm_track_configure_filter", "sdm_track_step_filtered", "sdm_track_get_filtered",
    "sdm_track_configure_motion", "sdm_track_get_motion",
    "sdm_warp_delaunay", "sdm_warp_set_mesh", "sdm_warp_get_labels", "sdm_warp_crops_tensor",
    "sdm_warp_crops_tensor_filtered",
    "sdm_align_paste_tensor", "sdm_align_paste_tensor_at",
    "sdm_warp_paste_tensor", "sdm_warp_paste_tensor_at",
    "sdm_align_paste_tensor_filtered", "sdm_align_paste_tensor_at_filtered",
    "sdm_align_paste_tensor_nv12", "sdm_align_paste_tensor_at_nv12",
    "sdm_warp_paste_tensor_nv12", "sdm_warp_paste_tensor_at_nv12",
    "sdm_warp_paste_tensor_filtered", "sdm_warp_paste_tensor_at_filtered",
    "sdm_align_region_mask", "sdm_align_region_mask_at",
]

# multi-stream tracking (include/sdm.h, sdm_track_*)
SDM_TRACK_FREE, SDM_TRACK_STARTED, SDM_TRACK_TRACKED, SDM_TRACK_LOST = 0, 1, 2, 3
SDM_TRACK_INIT_PREVIOUS, SDM_TRACK_INIT_REALIGN = 0, 1
SDM_TRACK_LOST_NONFINITE, SDM_TRACK_LOST_SMALL, SDM_TRACK_LOST_OUTSIDE, SDM_TRACK_LOST_SCALE = 1, 2, 4, 8

# the tracker's temporal landmark filter (include/sdm.h, "Tracking, filtered")
SDM_TRACK_FILTER_OFF, SDM_TRACK_FILTER_ONE_EURO = 0, 1

# the tracker's motion-compensated initialisation (include/sdm.h, "Tracking, motion-compensated")
SDM_TRACK_MOTION_OFF, SDM_TRACK_MOTION_SAD = 0, 1

# upright-normalised detect and tracking (include/sdm.h, "Rolled faces")
SDM_UPRIGHT_PARTIAL, SDM_UPRIGHT_NEAR_EDGE = 1, 2

# aligned face crops (include/sdm.h, sdm_align_*)
SDM_ALIGN_DEGENERATE, SDM_ALIGN_PARTIAL = 1, 2

# landmark region masks (include/sdm.h, "Landmark region masks"): a vertex is not finite or beyond 2^20 in the crop
SDM_REGION_NONFINITE = 16
REGION_MAX_POLYGONS, REGION_MAX_SIZE, REGION_MAX_POINTS = 8, 128, 256

# crops as network input tensors (include/sdm.h, sdm_align_crops_tensor)
SDM_ALIGN_U8, SDM_ALIGN_F16, SDM_ALIGN_F32 = 0, 1, 2
SDM_ALIGN_NHWC, SDM_ALIGN_NCHW = 0, 1
SDM_ALIGN_ORDER_BGR, SDM_ALIGN_ORDER_RGB = 0, 1
ALIGN_DTYPES = {"uint8": SDM_ALIGN_U8, "float16": SDM_ALIGN_F16, "float32": SDM_ALIGN_F32}
ALIGN_LAYOUTS = {"nhwc": SDM_ALIGN_NHWC, "nchw": SDM_ALIGN_NCHW}
ALIGN_ORDERS = {"bgr": SDM_ALIGN_ORDER_BGR, "rgb": SDM_ALIGN_ORDER_RGB}
# area-averaged sampling of minified rows (include/sdm.h, sdm_align_crops_tensor_filtered)
SDM_ALIGN_FILTER_BILINEAR, SDM_ALIGN_FILTER_AREA = 0, 1
ALIGN_FILTERS = {"bilinear": SDM_ALIGN_FILTER_BILINEAR, "area": SDM_ALIGN_FILTER_AREA}

# piecewise-affine warped faces (include/sdm.h, "Warped faces")
SDM_WARP_DEGENERATE, SDM_WARP_PARTIAL, SDM_WARP_FOLDED = 1, 2, 4
SDM_WARP_NO_TRIANGLE = 255

# frames on the device (include/sdm.h, sdm_set_frames_device)
SDM_FRAME_GRAY, SDM_FRAME_BGR, SDM_FRAME_RGB, SDM_FRAME_BGRA, SDM_FRAME_RGBA, SDM_FRAME_NV12 = range(6)
FRAME_FORMATS = {"gray": SDM_FRAME_GRAY, "bgr": SDM_FRAME_BGR, "rgb": SDM_FRAME_RGB, "bgra": SDM_FRAME_BGRA, "rgba": SDM_FRAME_RGBA,
                 "nv12": SDM_FRAME_NV12}
# planar colour, 3 x H x W (include/sdm.h, "Planar colour frames"): three planes of one byte per pixel, B G R or R G B
SDM_FRAME_BGR_PLANAR, SDM_FRAME_RGB_PLANAR = 16, 17
FRAME_FORMATS.update({"bgr_planar": SDM_FRAME_BGR_PLANAR, "rgb_planar": SDM_FRAME_RGB_PLANAR})
_FRAME_PLANAR = (SDM_FRAME_BGR_PLANAR, SDM_FRAME_RGB_PLANAR)
# YUV colour description and 10-bit surfaces (include/sdm.h): a YUV frame's name is base[:matrix][:range] -- "nv12:bt709",
# "nv12:bt601:full", "p010:bt2020", "p010" -- and its value the base or-ed with the matrix and range bits; "nv12" alone stays 5
SDM_FRAME_P010 = 7                                                        # (6 stays free: always refused as an unknown format)
_FRAME_YUV_BASES = {"nv12": SDM_FRAME_NV12, "p010": SDM_FRAME_P010}       # (FRAME_FORMATS stays the table of the 8-bit formats)
SDM_FRAME_YUV_BT601, SDM_FRAME_YUV_BT709, SDM_FRAME_YUV_BT2020, SDM_FRAME_YUV_FULL = 0x000, 0x100, 0x200, 0x1000
FRAME_MATRICES = {"bt601": SDM_FRAME_YUV_BT601, "bt709": SDM_FRAME_YUV_BT709, "bt2020": SDM_FRAME_YUV_BT2020}
FRAME_RANGES = {"limited": 0, "full": SDM_FRAME_YUV_FULL}


def frame_base(code: int) -> int:
    """SDM_FRAME_BASE of a format value."""
    return int(code) & 0xff


# (bytes per pixel of plane 0; a planar frame is not among the 1-byte frames an H x W tensor can be)
_FRAME_CHANNELS = {SDM_FRAME_GRAY: 1, SDM_FRAME_NV12: 1, SDM_FRAME_BGR: 3, SDM_FRAME_RGB: 3, SDM_FRAME_BGRA: 4, SDM_FRAME_RGBA: 4}


class SdmFrame(ctypes.Structure):
    """``sdm_frame``: one device-resident frame of sdm_set_frames_device."""

    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_int), ("height", ctypes.c_int), ("stride_bytes", ctypes.c_int),
                ("format", ctypes.c_int)]


class SdmAlignTensor(ctypes.Structure):
    """``sdm_align_tensor``: element type, layout, channels, order, per-channel scale and bias of sdm_align_crops_tensor."""

    _fields_ = [("dtype", ctypes.c_int), ("layout", ctypes.c_int), ("channels", ctypes.c_int), ("order", ctypes.c_int),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3), ("gray_shift", ctypes.c_int)]


class SdmAlignFilter(ctypes.Structure):
    """``sdm_align_filter``: the sampling of sdm_align_crops_tensor_filtered -- mode, the cap on the sub-samples per axis, the scale gate."""

    _fields_ = [("mode", ctypes.c_int), ("max_samples", ctypes.c_int), ("min_scale", ctypes.c_float)]


class SdmAlignPaste(ctypes.Structure):
    """``sdm_align_paste``: the crop-space opacity of sdm_align_paste_tensor -- a device pointer (None: 255 inside the crop) and whether
    there is one map per row."""

    _fields_ = [("alpha_dev", ctypes.c_void_p), ("alpha_per_row", ctypes.c_int)]


class SdmRegionMask(ctypes.Structure):
    """``sdm_region_mask``: the polygons' vertex counts (the holes last), which polygons are convex hulls, grow and feather."""

    _fields_ = [("sizes", ctypes.POINTER(ctypes.c_int)), ("n_polygons", ctypes.c_int), ("n_holes", ctypes.c_int),
                ("hull_bits", ctypes.c_uint), ("grow", ctypes.c_float), ("feather", ctypes.c_float)]


def region_mask(sizes, n_holes=0, hull=(), grow=0.0, feather=0.0):
    """The ``sdm_region_mask`` of the named options and what must stay alive beside it.  Pure host code.  ``sizes``: the vertex count of
    every polygon, the ``n_holes`` holes last; ``hull``: the positions of the polygons that are the convex hull of their points;
    ``grow`` / ``feather``: crop pixels.  The ranges are the library's to refuse; what cannot be expressed is refused here."""
    sizes = [int(v) for v in sizes]
    if not 1 <= len(sizes) <= REGION_MAX_POLYGONS:
        raise ValueError(f"a region has 1 to {REGION_MAX_POLYGONS} polygons, not {len(sizes)}")
    bits = 0
    for g in hull:
        if not 0 <= int(g) < len(sizes):
            raise ValueError(f"hull names polygon {g}: there are {len(sizes)}")
        bits |= 1 << int(g)
    arr = (ctypes.c_int * len(sizes))(*sizes)
    return SdmRegionMask(arr, len(sizes), int(n_holes), bits, float(grow), float(feather)), arr


def align_filter(mode="area", max_samples=16, min_scale=1.0) -> SdmAlignFilter:
    """The ``sdm_align_filter`` of the named options.  Pure host code.  ``mode``: "area" (a row whose similarity minifies averages
    S x S bilinear sub-samples per pixel, S the smallest integer with S^2 >= scale^2) | "bilinear" (S = 1 everywhere);
    ``max_samples``: the cap on S, 1 ... 16; ``min_scale`` (finite, >= 1): rows with scale^2 < min_scale^2 keep S = 1."""
    import math
    if not isinstance(mode, str) or mode.lower() not in ALIGN_FILTERS:
        raise ValueError(f"unknown filter mode {mode!r}: one of {sorted(ALIGN_FILTERS)}")
    if int(max_samples) != max_samples or not 1 <= int(max_samples) <= 16:
        raise ValueError("max_samples must be an integer in [1, 16]")
    if not math.isfinite(min_scale) or min_scale < 1:
        raise ValueError("min_scale must be finite and >= 1")
    return SdmAlignFilter(ALIGN_FILTERS[mode.lower()], int(max_samples), float(min_scale))


def _three(v, what):
    """A scalar or 3 values as 3 float64 numbers."""
    import numpy as np
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f"{what} must be a scalar or 3 values")
    return a


def align_tensor_spec(dtype="float16", layout="nchw", channels=3, order="rgb", scale=None, bias=None, mean=None, std=None,
                      gray_shift=14) -> SdmAlignTensor:
    """The ``sdm_align_tensor`` of the named options.  Pure host code.  ``dtype``: "uint8" | "float16" | "float32" (or a numpy / torch
    dtype of that name); ``layout``: "nchw" | "nhwc"; ``order``: "rgb" | "bgr".  Element = float32(v) * scale[c] + bias[c] per OUTPUT
    channel c.  ``scale`` / ``bias``: a scalar or 3 values, given to the library as float32 (defaults 1 and 0).  ``mean`` / ``std``
    (0-255 units, a scalar or 3 values) are sugar for ``scale = float32(1 / std)``, ``bias = float32(-mean / std)``, both quotients
    computed in float64 and rounded once; giving them together with ``scale`` or ``bias`` is an error."""
    import numpy as np
    name = str(dtype).split(".")[-1].lower() if not isinstance(dtype, type) else np.dtype(dtype).name
    if name not in ALIGN_DTYPES:
        raise ValueError(f"unknown dtype {dtype!r}: one of {sorted(ALIGN_DTYPES)}")
    if not isinstance(layout, str) or layout.lower() not in ALIGN_LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: one of {sorted(ALIGN_LAYOUTS)}")
    if not isinstance(order, str) or order.lower() not in ALIGN_ORDERS:
        raise ValueError(f"unknown channel order {order!r}: one of {sorted(ALIGN_ORDERS)}")
    if int(channels) not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    if int(gray_shift) not in (14, 15):
        raise ValueError("gray_shift must be 14 or 15")
    if (mean is not None or std is not None) and (scale is not None or bias is not None):
        raise ValueError("give either scale / bias or mean / std, not both")
    if mean is not None or std is not None:
        m = _three(0.0 if mean is None else mean, "mean")
        sd = _three(1.0 if std is None else std, "std")
        if not (sd != 0).all():
            raise ValueError("std must not be 0")
        sc, bi = (1.0 / sd).astype(np.float32), (-m / sd).astype(np.float32)
    else:
        sc = _three(1.0 if scale is None else scale, "scale").astype(np.float32)
        bi = _three(0.0 if bias is None else bias, "bias").astype(np.float32)
    return SdmAlignTensor(ALIGN_DTYPES[name], ALIGN_LAYOUTS[layout.lower()], int(channels), ALIGN_ORDERS[order.lower()],
                          (ctypes.c_float * 3)(*sc.tolist()), (ctypes.c_float * 3)(*bi.tolist()), int(gray_shift))


def paste_tensor_spec(dtype, layout="nchw", channels=3, order="rgb", scale=None, bias=None, mean=None, std=None,
                      gray_shift=14) -> SdmAlignTensor:
    """The ``sdm_align_tensor`` of a paste (sdm_align_paste_tensor): a tensor element e is decoded as float32(e) * scale[c] + bias[c], the
    INVERSE of the crop call's element -- so ``mean`` / ``std`` (0-255 units, a scalar or 3 values) here mean ``scale = float32(std)``,
    ``bias = float32(mean)``: the same ``mean`` / ``std`` as in the crop call undo it.  Everything else as ``align_tensor_spec``."""
    if (mean is not None or std is not None) and (scale is not None or bias is not None):
        raise ValueError("give either scale / bias or mean / std, not both")
    if mean is not None or std is not None:
        scale, bias = (1.0 if std is None else std), (0.0 if mean is None else mean)
    return align_tensor_spec(dtype, layout, channels, order, scale, bias, None, None, gray_shift)


def align_tensor_shape(n: int, width: int, height: int, layout: int, channels: int):
    return (n, channels, height, width) if layout == SDM_ALIGN_NCHW else (n, height, width, channels)


def check_align_out(out, shape, dtype_name: str):
    """``out`` of aligned_crops_tensor: a contiguous device tensor of the requested dtype and shape (duck-typed: dtype, shape,
    is_contiguous(), is_cuda)."""
    if str(out.dtype).split(".")[-1] != dtype_name:
        raise ValueError(f"out must be a {dtype_name} tensor, not {out.dtype}")
    if tuple(int(v) for v in out.shape) != tuple(shape):
        raise ValueError(f"out must have the shape {tuple(shape)}, not {tuple(out.shape)}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    if not getattr(out, "is_cuda", False):
        raise ValueError("out must be on the device")


# every name of a frame format, in lower case: the formats there always were, and base[:matrix][:range] of the YUV bases with each
# part at most once and in that order (one look-up per frame: a list of thousands names its format once per frame)
_FRAME_NAMES = dict(FRAME_FORMATS)
for _base, _code in _FRAME_YUV_BASES.items():
    for _m, _mbits in [("", 0)] + [(":" + k, v) for k, v in FRAME_MATRICES.items()]:
        for _r, _rbits in [("", 0)] + [(":" + k, v) for k, v in FRAME_RANGES.items()]:
            _FRAME_NAMES[_base + _m + _r] = _code | _mbits | _rbits


def _frame_format(fmt) -> int:
    if isinstance(fmt, str):
        code = _FRAME_NAMES.get(fmt)
        if code is None:
            code = _FRAME_NAMES.get(fmt.lower())
        if code is None:
            raise ValueError(f"unknown frame format {fmt!r}: one of {sorted(FRAME_FORMATS) + ['p010']}, a YUV one as "
                             f"base[:matrix][:range] with {sorted(FRAME_MATRICES)} and {sorted(FRAME_RANGES)}")
        return code
    return int(fmt)


def _is_tensor(obj) -> bool:
    return hasattr(obj, "data_ptr") and hasattr(obj, "stride") and hasattr(obj, "shape")


def _is_planar_name(fmt) -> bool:
    return fmt is not None and _frame_format(fmt) in _FRAME_PLANAR


def _planar_tensor_frame(ptr: int, shape, stride, fmt):
    """One 3 x H x W view named planar -> ((ptr, w, h, stride_bytes, format), the second plane's address or None for the default
    plane distance height * stride_bytes).  Only stride(2) == 1 is asked for: the row and the channel stride are free, of any sign."""
    if len(shape) != 3 or shape[0] != 3:
        raise ValueError(f"a {fmt!r} frame is 3 x H x W")
    _, h, w = shape
    ch, row, px = stride
    if h < 1 or w < 1:
        raise ValueError("empty frame")
    if w > 1 and px != 1:
        raise ValueError("a planar frame must be dense within a row: stride(2) == 1")
    if h > 1 and row < w:
        raise ValueError("the row stride is smaller than a row")
    st = int(row) if h > 1 else int(w)
    return (int(ptr), int(w), int(h), st, _frame_format(fmt)), (None if ch == h * st else int(ptr) + int(ch))


def _tensor_frame(ptr: int, shape, stride, fmt):
    """One H x W or H x W x C view (sizes and strides in elements = bytes) -> (ptr, w, h, stride_bytes, format)."""
    if len(shape) == 2:
        (h, w), c = shape, 1
        row, px, ch = stride[0], stride[1], 1
        code = SDM_FRAME_GRAY if fmt is None else _frame_format(fmt)
        # (NV12 luma with any colour description; a P010 plane is 16-bit words: it comes as a (ptr, w, h, stride, "p010...") tuple)
        if _FRAME_CHANNELS.get(code if frame_base(code) != SDM_FRAME_NV12 else SDM_FRAME_NV12) != 1:
            raise ValueError("an H x W frame is gray (or NV12 luma)")
    elif len(shape) == 3:
        h, w, c = shape
        row, px, ch = stride
        if c not in (3, 4):
            raise ValueError("a colour frame is H x W x 3 (bgr, rgb) or H x W x 4 (bgra, rgba)")
        code = (SDM_FRAME_BGR if c == 3 else SDM_FRAME_BGRA) if fmt is None else _frame_format(fmt)
        if _FRAME_CHANNELS.get(code) != c:
            raise ValueError(f"format {fmt!r} does not have {c} channels")
    else:
        raise ValueError("a frame is H x W or H x W x C")
    if h < 1 or w < 1:
        raise ValueError("empty frame")
    # (the stride of a dimension of size 1 is never used to form an address: whatever the producer left there is accepted)
    if (c > 1 and ch != 1) or (w > 1 and px != c):
        raise ValueError("frames must be interleaved and dense within a row: stride(-1) == 1 and a pixel stride of C bytes")
    if h > 1 and row < w * c:
        raise ValueError("the row stride is smaller than a row")
    return (int(ptr), int(w), int(h), int(row) if h > 1 else int(w * c), code)


def frame_descriptors(frames, formats=None):
    """``frame_planes(frames, formats)[0]``: the ``sdm_frame`` list alone, as (ptr, width, height, stride_bytes, format) tuples.  A
    planar tensor's 5-tuple does not carry its plane distance; the calls that take ``frames=`` use ``frame_planes``."""
    return frame_planes(frames, formats)[0]


def _one_planar_name(formats):
    """The planar name that makes ONE bare 3 x H x W tensor one frame -- given as a name or as a list of that one name -- or None."""
    if isinstance(formats, (list, tuple)) and len(formats) == 1:
        formats = formats[0]
    return formats if isinstance(formats, (str, int)) and _is_planar_name(formats) else None


def frame_planes(frames, formats=None, chroma=None):
    """(descriptors, planes): the ``sdm_frame`` list of ``frames`` as (ptr, width, height, stride_bytes, format) tuples and, per frame,
    the address of its SECOND PLANE or None (the default: directly behind plane 0) -- what the library's ``chroma`` / ``dst_chroma`` /
    ``planes`` arrays take.  Pure host code on duck-typed objects (``data_ptr()``, ``shape``, ``stride()``, ``dtype``): no device, no
    torch needed.
    ``frames``: a list whose members are uint8 tensors -- H x W (gray), H x W x 3 ("bgr", the default, or "rgb"), H x W x 4 ("bgra",
    the default, or "rgba") -- or ready (ptr, w, h, stride, format) tuples (NV12 luma, foreign allocators), which pass through
    unchanged but for a format given by name; or ONE stacked tensor n x H x W [x C].  A tensor only needs stride(-1) == 1 and a pixel
    stride of C: the row stride is free, so views into larger frames work.  ``formats``: None, one name for all tensors, or one per
    frame (None entries = the default).
    A 3 x H x W uint8 tensor is a planar colour frame ONLY when ``formats`` names it "bgr_planar" or "rgb_planar": it needs
    stride(2) == 1, the row stride and the channel stride are free (regions x[:, 100:580, 200:840], frames of an n x 3 x H x W batch,
    channel-reversed views with a negative stride), and its second plane is data_ptr() + stride(0) -- None when that is the default
    height * stride_bytes.  One stacked n x 3 x H x W tensor with a planar name splits along dimension 0; one bare 3 x H x W tensor
    with a planar name (or a list of that one name) is one frame.  ``chroma``: None or one entry per frame -- a device pointer, a
    uint8 tensor or None --, the second plane of a (ptr, w, h, stride, "nv12" | "bgr_planar" | "rgb_planar") tuple; an entry given for
    a planar tensor replaces the one computed from its strides.  Without a planar name everything is as ``frame_descriptors`` always
    was, refusals included."""
    if _is_tensor(frames):
        shape, stride = tuple(int(v) for v in frames.shape), tuple(int(v) for v in frames.stride())
        if len(shape) not in (3, 4):
            raise ValueError("a stacked tensor is n x H x W, n x H x W x C or -- named planar -- n x 3 x H x W")
        _check_u8(frames)
        base = int(frames.data_ptr())
        if len(shape) == 3 and _one_planar_name(formats) is not None:
            items = [("t", base, shape, stride)]                 # (one 3 x H x W frame named planar, not a stack of three)
        else:
            items = [("t", base + i * stride[0], shape[1:], stride[1:]) for i in range(shape[0])]
    else:
        items = []
        for f in frames:
            if _is_tensor(f):
                _check_u8(f)
                items.append(("t", int(f.data_ptr()), tuple(int(v) for v in f.shape), tuple(int(v) for v in f.stride())))
            else:
                if len(f) != 5:
                    raise ValueError("a frame tuple is (ptr, width, height, stride_bytes, format)")
                items.append(("d", f))
    if not items:
        raise ValueError("no frames")
    if formats is None or isinstance(formats, (str, int)):
        formats = [formats] * len(items)
    if len(formats) != len(items):
        raise ValueError("one format per frame expected")
    if chroma is not None and len(chroma) != len(items):
        raise ValueError("one chroma entry (or None) per frame expected")
    # (a second plane is stored only where there is one, at the index of the descriptor being appended)
    out, planes = [], [None] * len(items)
    planar = {fmt for fmt in set(formats) if _is_planar_name(fmt)}
    for it, fmt in zip(items, formats):
        if it[0] == "d":
            ptr, w, h, st, code = it[1]
            out.append((int(ptr), int(w), int(h), int(st), _frame_format(code)))
        elif planar and fmt in planar:
            d, planes[len(out)] = _planar_tensor_frame(it[1], it[2], it[3], fmt)
            out.append(d)
        else:
            out.append(_tensor_frame(it[1], it[2], it[3], fmt))
    if chroma is not None:
        for i, u in enumerate(chroma):
            if u is not None:
                planes[i] = int(u.data_ptr()) if _is_tensor(u) else int(u)
    return out, planes


def planes_array(planes):
    """The c_void_p array of ``frame_planes``' second planes, or None when every entry is the default."""
    if planes.count(None) == len(planes):
        return None
    return (ctypes.c_void_p * len(planes))(*planes)


def _check_u8(t):
    if str(t.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"frames must be uint8, not {t.dtype}")


class SdmHogParam(ctypes.Structure):
    """``sdm_hog_param`` = rcr::HoGParam (include/rcr/adaptive_vlhog.hpp:41-60)."""

    _fields_ = [("variant", ctypes.c_int), ("num_cells", ctypes.c_int), ("cell_size", ctypes.c_int),
                ("num_bins", ctypes.c_int), ("relative_patch_size", ctypes.c_float)]


ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                ctypes.c_void_p)
# sdm_bcast_fn(dev_ptr, count_f32, root, hip_stream, user), sdm_allgather_fn(send_ptr, recv_ptr, count_f32, hip_stream, user)
BCAST_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p)

_LIB = None


class SdmError(RuntimeError):
    """Raised for every non-zero status of the C-ABI (the C++ layer rethrows std::runtime_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"sdm error {code}: {msg}")
        self.code = code


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm ships its own libamdhip64.so.7 next to libtorch; libsdm_hip.so is linked against the ROCm
    installation's copy of the same soname.  Whichever is mapped first serves both.  Mapping the ROCm copy first leaves
    a later ``import torch`` with a runtime it cannot initialise ("No HIP GPUs are available"), so -- when torch is
    installed but not imported yet -- its copy is mapped first; the engine is happy with either."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(LIB_PATH)
        c_int, c_void_p, c_float_p = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
        c_int_p = ctypes.POINTER(ctypes.c_int)
        L.sdm_last_error.restype = ctypes.c_char_p
        L.sdm_create.restype = c_void_p
        L.sdm_create.argtypes = [c_int]
        L.sdm_destroy.argtypes = [c_void_p]
        L.sdm_destroy.restype = None
        sigs = {
            "sdm_set_stream": [c_void_p, c_void_p],
            "sdm_synchronize": [c_void_p],
            "sdm_set_model_geometry": [c_void_p, c_int, c_int_p, c_int, c_int_p, c_int, c_int,
                                       ctypes.POINTER(SdmHogParam)],
            "sdm_feature_dim": [c_void_p, c_int],
            "sdm_set_hog_mode": [c_void_p, c_int],
            "sdm_get_hog_info": [c_void_p, c_int, c_int_p, c_int_p],
            "sdm_upload_images_u8": [c_void_p, ctypes.POINTER(c_void_p), c_int_p, c_int_p, c_int_p, c_int],
            "sdm_set_images_device": [c_void_p, c_void_p, c_int, c_int, c_int, c_int],
            "sdm_upload_images_bgr_u8": [c_void_p, ctypes.POINTER(c_void_p), c_int_p, c_int_p, c_int_p, c_int, c_int],
            "sdm_debug_download_images": [c_void_p, c_void_p, c_int, c_int, c_int],
            "sdm_set_sample_image_index": [c_void_p, c_int_p, c_int],
            "sdm_set_x": [c_void_p, c_float_p, c_int],
            "sdm_get_x": [c_void_p, c_float_p],
            "sdm_set_x_device": [c_void_p, c_void_p, c_int],
            "sdm_get_x_device": [c_void_p, c_void_p],
            "sdm_hog_features": [c_void_p, c_int, c_float_p],
            "sdm_get_patch_indices": [c_void_p, c_int_p],
            "sdm_set_regressor": [c_void_p, c_int, c_float_p],
            "sdm_get_regressor": [c_void_p, c_int, c_float_p],
            "sdm_apply": [c_void_p, c_int],
            "sdm_detect_batch": [c_void_p, c_float_p],
            "sdm_detect_level": [c_void_p, c_int],
            "sdm_set_targets": [c_void_p, c_float_p, c_int],
            "sdm_gram_rhs": [c_void_p, c_int],
            "sdm_set_allreduce": [c_void_p, ALLREDUCE_FN, c_void_p, c_int],
            "sdm_allreduce_gram_rhs": [c_void_p],
            "sdm_set_allreduce_rccl": [c_void_p, c_void_p, c_void_p, c_int],
            "sdm_set_solve_sharding": [c_void_p, c_int, c_int, BCAST_FN, ALLGATHER_FN, c_void_p],
            "sdm_set_solve_sharding_rccl": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
            "sdm_set_reduce_scatter": [c_void_p, ALLGATHER_FN, c_void_p],          # (same shape: send, recv, count per rank, stream, user)
            "sdm_set_reduce_scatter_rccl": [c_void_p, c_int, c_void_p],
            "sdm_solve": [c_void_p, c_int, c_int, ctypes.c_float, c_int, ctypes.c_longlong, c_float_p, c_float_p],
            "sdm_train_level": [c_void_p, c_int, c_int, ctypes.c_float, c_int, ctypes.c_longlong],
            "sdm_set_solver": [c_void_p, c_int],
            "sdm_last_rank": [c_void_p, c_int_p, c_int_p],
            "sdm_solve_normal_equations": [c_void_p, c_float_p, c_int, c_int, c_float_p, c_int, c_int, ctypes.c_float, c_int,
                                           c_float_p, c_float_p],
            "sdm_solve_normal_equations_with": [c_void_p, c_int, c_float_p, c_int, c_int, c_float_p, c_int, c_int, ctypes.c_float, c_int,
                                                c_float_p, c_float_p, c_int_p, c_int_p],
            "sdm_set_templates": [c_void_p, c_void_p, c_int, c_int],
            "sdm_init_from_boxes": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
            "sdm_normalised_errors": [c_void_p, c_void_p, ctypes.POINTER(ctypes.c_double)],
            "sdm_gram_device_ptr": [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_size_t)],
            "sdm_x_device_ptr": [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_size_t)],
            "sdm_features_device_ptr": [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_longlong), c_int_p],
            "sdm_enable_timing": [c_void_p, c_int],
            "sdm_get_timing": [c_void_p, c_float_p, c_int_p, c_int],
            "sdm_debug_patch": [c_void_p, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_uint8),
                                ctypes.POINTER(ctypes.c_uint8), c_float_p, c_float_p],
            "sdm_debug_gradient_table": [c_void_p, c_int, c_float_p, c_int_p],
            "sdm_debug_set_option": [c_void_p, ctypes.c_char_p, c_int],
            "sdm_debug_update_f16": [c_void_p, c_float_p, c_int, c_int, c_int, ctypes.c_float, c_float_p],
            "sdm_debug_hog_profile": [c_void_p, c_int, ctypes.POINTER(ctypes.c_ulonglong)],
            "sdm_debug_set_hog_packing": [c_void_p, c_int],
            "sdm_debug_gram_fallbacks": [c_void_p],
            "sdm_debug_update_fallbacks": [c_void_p],
            "sdm_debug_hog_plan": [c_int, c_int, c_int, c_int, c_int_p, c_void_p, c_void_p, c_void_p, c_int],
            "sdm_debug_hog_plan_cut": [c_int, c_int, c_int, c_int, c_int_p],
            "sdm_debug_hog_plan_columns": [c_int, c_int, c_int, c_int, c_int_p],
            "sdm_debug_hog_band_weights": [c_int, c_int, c_float_p],
            "sdm_debug_hog_taps": [c_void_p, c_int, c_int_p, c_int_p],
            "sdm_debug_hog_pair_taps": [c_void_p, c_int, c_int_p, c_int_p],
            "sdm_debug_set_detect_path": [c_void_p, c_int, c_int],
            "sdm_pose_set_model": [c_void_p, c_void_p, c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_float],
            "sdm_pose_set_x": [c_void_p, c_void_p, c_int],
            "sdm_pose_get_x": [c_void_p, c_void_p],
            "sdm_pose_set_x_device": [c_void_p, c_void_p, c_int],
            "sdm_pose_set_templates": [c_void_p, c_void_p, c_int, c_int],
            "sdm_pose_templates_from_landmarks": [c_void_p, c_void_p, c_int, ctypes.c_float],
            "sdm_pose_set_targets": [c_void_p, c_void_p, c_int],
            "sdm_pose_features": [c_void_p, c_int, c_void_p],
            "sdm_pose_train_level": [c_void_p, c_int, c_int, ctypes.c_float, c_int, c_void_p, c_float_p],
            "sdm_pose_set_regressor": [c_void_p, c_int, c_void_p],
            "sdm_pose_get_regressor": [c_void_p, c_int, c_void_p],
            "sdm_pose_test": [c_void_p, c_int, c_int],
            "sdm_track_configure": [c_void_p, c_int, c_void_p, c_int, ctypes.c_float, ctypes.c_float],
            "sdm_track_start": [c_void_p, c_void_p, c_void_p, c_int],
            "sdm_track_stop": [c_void_p, c_void_p, c_int],
            "sdm_track_step": [c_void_p, c_void_p, c_int, c_void_p, c_void_p],
            "sdm_track_get": [c_void_p, c_void_p, c_int, c_void_p, c_void_p],
            "sdm_align_set_source": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int],
            "sdm_align_crops": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p],
            "sdm_align_set_source_frames": [c_void_p, ctypes.POINTER(SdmFrame), c_void_p, c_int],
            "sdm_align_crops_tensor": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor), c_void_p, c_void_p,
                                       c_void_p],
            "sdm_align_crops_tensor_filtered": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor),
                                                ctypes.POINTER(SdmAlignFilter), c_void_p, c_void_p, c_void_p, c_void_p],
            "sdm_train_level_sweep": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, ctypes.c_longlong, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int_p],
            "sdm_sweep_get_regressor": [c_void_p, c_int, c_float_p],
            "sdm_set_frames_device": [c_void_p, ctypes.POINTER(SdmFrame), c_int, c_int],
            "sdm_set_frames_device_planes": [c_void_p, ctypes.POINTER(SdmFrame), c_void_p, c_int, c_int],
            "sdm_debug_download_image": [c_void_p, c_int, c_void_p],
            "sdm_upright_configure": [c_void_p, c_int, c_int],
            "sdm_detect_batch_upright": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
            "sdm_upright_get": [c_void_p, c_void_p, c_void_p, c_void_p],
            "sdm_track_configure_upright": [c_void_p, c_int],
            "sdm_track_start_rolled": [c_void_p, c_void_p, c_void_p, c_void_p, c_int],
            "sdm_track_configure_filter": [c_void_p, c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float],
            "sdm_track_step_filtered": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
            "sdm_track_get_filtered": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
            "sdm_track_configure_motion": [c_void_p, c_int, c_int, ctypes.c_float, c_int],
            "sdm_track_get_motion": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
            "sdm_warp_delaunay": [c_void_p, c_int, c_void_p, c_int, c_int_p],
            "sdm_warp_set_mesh": [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int],
            "sdm_warp_get_labels": [c_void_p, c_void_p],
            "sdm_warp_crops_tensor": [c_void_p, ctypes.POINTER(SdmAlignTensor), c_void_p, c_void_p, c_void_p],
            "sdm_warp_crops_tensor_filtered": [c_void_p, ctypes.POINTER(SdmAlignTensor), ctypes.POINTER(SdmAlignFilter), c_void_p, c_void_p,
                                               c_void_p, c_void_p],
            "sdm_align_paste_tensor": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor), c_void_p,
                                       ctypes.POINTER(SdmAlignPaste), ctypes.POINTER(SdmFrame), c_int, c_void_p, c_void_p],
            "sdm_align_paste_tensor_at": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor), c_void_p,
                                          ctypes.POINTER(SdmAlignPaste), ctypes.POINTER(SdmFrame), c_int, c_void_p],
            "sdm_warp_paste_tensor": [c_void_p, ctypes.POINTER(SdmAlignTensor), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                      ctypes.POINTER(SdmFrame), c_int, c_void_p, c_void_p],
            "sdm_warp_paste_tensor_at": [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(SdmAlignTensor), c_void_p,
                                         ctypes.POINTER(SdmAlignPaste), ctypes.POINTER(SdmFrame), c_int, c_void_p],
            "sdm_align_paste_tensor_filtered": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor),
                                                ctypes.POINTER(SdmAlignFilter), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                                ctypes.POINTER(SdmFrame), c_int, c_void_p, c_void_p, c_void_p],
            "sdm_align_paste_tensor_at_filtered": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor),
                                                   ctypes.POINTER(SdmAlignFilter), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                                   ctypes.POINTER(SdmFrame), c_int, c_void_p, c_void_p],
            "sdm_align_paste_tensor_nv12": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor),
                                            ctypes.POINTER(SdmAlignFilter), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                            ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p, c_void_p, c_void_p],
            "sdm_align_paste_tensor_at_nv12": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmAlignTensor),
                                               ctypes.POINTER(SdmAlignFilter), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                               ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p, c_void_p],
            "sdm_warp_paste_tensor_nv12": [c_void_p, ctypes.POINTER(SdmAlignTensor), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                           ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p, c_void_p],
            "sdm_warp_paste_tensor_at_nv12": [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(SdmAlignTensor), c_void_p,
                                              ctypes.POINTER(SdmAlignPaste), ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p],
            "sdm_warp_paste_tensor_filtered": [c_void_p, ctypes.POINTER(SdmAlignTensor), ctypes.POINTER(SdmAlignFilter), c_void_p,
                                               ctypes.POINTER(SdmAlignPaste), ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p, c_void_p,
                                               c_void_p],
            "sdm_warp_paste_tensor_at_filtered": [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(SdmAlignTensor),
                                                  ctypes.POINTER(SdmAlignFilter), c_void_p, ctypes.POINTER(SdmAlignPaste),
                                                  ctypes.POINTER(SdmFrame), c_void_p, c_int, c_void_p, c_void_p],
            "sdm_align_region_mask": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, ctypes.POINTER(SdmRegionMask), c_void_p,
                                      c_void_p, c_void_p],
            "sdm_align_region_mask_at": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SdmRegionMask), c_void_p,
                                         c_void_p],
        }
        for name, args in sigs.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = c_int
        L.sdm_device_count.restype = c_int
        _LIB = L
    return _LIB


def check(rc: int) -> int:
    if rc < 0:
        raise SdmError(rc, lib().sdm_last_error().decode("utf-8", "replace"))
    return rc


def delaunay(xy):
    """The Delaunay triangulation of K x 2 points (sdm_warp_delaunay; host code of the library, no device needed): T x 3 int32 positions
    into ``xy``, every triangle counter-clockwise in the header's sense (D > 0), the same output for the same input."""
    import numpy as np
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    k = p.shape[0]
    tri = np.empty((max(2 * k, 1), 3), np.int32)
    n = ctypes.c_int(0)
    check(lib().sdm_warp_delaunay(p.ctypes.data, k, tri.ctypes.data, tri.shape[0], ctypes.byref(n)))
    return tri[:n.value].copy()
