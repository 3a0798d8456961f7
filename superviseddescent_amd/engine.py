"""Python host side of the engine: the reference's operator surface for the RCR hot path, bound to the
C-ABI (``include/sdm.h``) through ctypes.

Class and method names follow the reference so that the parity tests read like its own:

=============================================  =====================================================
``HoGParam``                                   rcr::HoGParam                 include/rcr/adaptive_vlhog.hpp:41-60
``HogTransform``                               rcr::HogTransform             include/rcr/adaptive_vlhog.hpp:70-195
``InterEyeDistanceNormalisation``              include/rcr/model.hpp:84-116
``Regulariser`` / ``LinearRegressor``          include/superviseddescent/regressors.hpp:87-169, 318-400
``SupervisedDescentOptimiser.train/test/predict``  include/superviseddescent/superviseddescent.hpp:165-344
``detection_model.detect``                     include/rcr/model.hpp:122-183
``ModelProjection``                            examples/pose_estimation.cpp:187-240 (head pose, csrc/sdm_pose.hip)
``detection_model.tracker`` / ``Tracker``       apps/rcr/rcr-track.cpp:133-177 (multi-stream tracking, csrc/sdm_track.hip)
``detection_model.aligned_crops``              (extension) aligned face crops of the current rows, csrc/sdm_align.hip
``detection_model.aligned_crops_tensor``       (extension) the crops as a network's input tensor, csrc/sdm_align_tensor.hip,
                                               csrc/sdm_align_area.hip (``filter="area"``: minified faces averaged per footprint)
=============================================  =====================================================

Everything numeric happens on the MI355X: HOG extraction, regressor apply, Gram/RHS build and the
Cholesky solve are HIP kernels behind the C-ABI.  Nothing here falls back to the CPU -- without the
built library or without a gfx950 device the constructors raise.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _lib, ibug
from ._lib import SdmError, SdmHogParam, check


@dataclass
class HoGParam:
    """rcr::HoGParam (include/rcr/adaptive_vlhog.hpp:41-60)."""

    vlhog_variant: int
    num_cells: int
    cell_size: int
    num_bins: int
    relative_patch_size: float

    @property
    def dim(self) -> int:
        return 3 * self.num_bins + 4 if self.vlhog_variant == 1 else 4 * self.num_bins  # hog.c:212-219

    @property
    def patch_dim(self) -> int:
        return self.num_cells * self.num_cells * self.dim


def _device_frames(images) -> bool:
    """``images`` is device input for ``Context.set_frames_device``: a tensor on the device, or a list whose first member is one
    or is a (ptr, w, h, stride, format) tuple."""
    if getattr(images, "is_cuda", False):
        return True
    if isinstance(images, (list, tuple)) and len(images):
        return bool(getattr(images[0], "is_cuda", False)) or isinstance(images[0], tuple)
    return False


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


_DEV_OPTIONS = ("hog_no_pack", "hog_two_load", "hog_split_store", "detect_unfused", "detect_fuse_wide", "apply_f32", "gram_f32", "gram_bf16x3", "update_f32",
                "gram_xblocks", "solve_upd_min_tiles", "solve_fine_head", "solve_bs_cap", "solve_shard_emulate")


# the tracker's motion search takes the best offset only when its SAD is at most (256 - MOTION_MIN_GAIN) / 256 of staying in place's.
# Of {0, 16, 32, 64} none leaves 90 % of the rows of a slowly moving face (up to 3 pixels per frame) at shift (0, 0) -- 58, 63, 68 and
# 78 % were measured --, so the default is the largest of the four
MOTION_MIN_GAIN = 64


class Context:
    """Owner of one ``sdm_ctx`` (one GPU, one stream).  Thin, 1:1 with the C-ABI."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = _lib.lib()
        self._h = self._lib.sdm_create(int(device))
        if not self._h:
            raise SdmError(_lib.SDM_ERR_NO_DEVICE, self._lib.sdm_last_error().decode())
        self.device = device
        self._keep = []  # keeps ctypes callbacks alive
        # development switches: the library reads no environment variable; this mirror -- what tests, bench legs and A/B scripts
        # drive -- forwards SDM_<NAME>=<int> of the process environment to sdm_debug_set_option (names: csrc/sdm_capi_debug.hip)
        for key, val in os.environ.items():
            if key.startswith("SDM_") and key[4:].lower() in _DEV_OPTIONS:
                self.set_option(key[4:].lower(), int(val))
        if stream is not None:
            check(self._lib.sdm_set_stream(self._h, ctypes.c_void_p(stream)))
        self.L = 0
        self.n_levels = 0
        self.align_channels = 1     # C of the crop source installed by align_set_source (the library writes N x H x W x C bytes)
        # level -> token of the regressor the DEVICE holds (None: unknown).  Kept here, next to the device copy, so that
        # two optimisers sharing this context cannot mistake each other's upload for their own.
        self._resident = {}

    def set_option(self, name: str, value: int):
        """A development switch by name (sdm_debug_set_option)."""
        check(self._lib.sdm_debug_set_option(self._h, name.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- geometry / inputs ---------------------------------------------------------------------
    def set_model_geometry(self, num_landmarks: int, right_eye_idx: Sequence[int],
                           left_eye_idx: Sequence[int], hog_params: Sequence[HoGParam]):
        re = np.ascontiguousarray(right_eye_idx, np.int32)
        le = np.ascontiguousarray(left_eye_idx, np.int32)
        arr = (SdmHogParam * len(hog_params))(*[
            SdmHogParam(p.vlhog_variant, p.num_cells, p.cell_size, p.num_bins, p.relative_patch_size)
            for p in hog_params])
        check(self._lib.sdm_set_model_geometry(self._h, num_landmarks, _ip(re), re.size, _ip(le), le.size,
                                               len(hog_params), arr))
        self.L, self.n_levels = num_landmarks, len(hog_params)
        # a changed geometry drops the device-side regressors (the same geometry again is a no-op in the library)
        key = (num_landmarks, tuple(re.tolist()), tuple(le.tolist()),
               tuple((p.vlhog_variant, p.num_cells, p.cell_size, p.num_bins, float(np.float32(p.relative_patch_size))) for p in hog_params))
        if key != getattr(self, "_geometry_key", None):
            self._geometry_key = key
            self.geometry_epoch = getattr(self, "geometry_epoch", 0) + 1
            self._resident = {}

    def set_hog_mode(self, mode: int):
        """``_lib.SDM_HOG_COLUMNS`` (default: per-pixel-column f32 sums folded into cells on the matrix cores),
        ``_lib.SDM_HOG_FAST`` (exact fixed-point sum, rounded once) or ``_lib.SDM_HOG_EXACT_ORDER`` (reference
        accumulation order, features bit-identical to the reference's CPU path)."""
        check(self._lib.sdm_set_hog_mode(self._h, int(mode)))

    def hog_info(self, level: int):
        fk, fb = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.sdm_get_hog_info(self._h, level, ctypes.byref(fk), ctypes.byref(fb)))
        return {"fast_kernel": bool(fk.value), "fast_bins": int(fb.value)}

    def feature_dim(self, level: int) -> int:
        return check(self._lib.sdm_feature_dim(self._h, level))

    def upload_images(self, images, gray_shift: int = 14):
        """``images``: list of uint8 arrays (or one stack): H x W single-channel, or H x W x 3 BGR as ``cv::imread`` yields
        them.  Colour images are converted to gray ONCE per image on the device with OpenCV's fixed-point weights
        (``cvtColor(COLOR_BGR2GRAY)``, adaptive_vlhog.hpp:114-120 -- the reference converts per sample and per level)."""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        n = len(imgs)
        colour = [im.ndim == 3 for im in imgs]
        for im in imgs:
            if not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
                raise ValueError("images must be H x W (gray) or H x W x 3 (BGR) uint8")
        if any(colour) and not all(colour):
            raise ValueError("gray and colour images cannot be mixed in one upload")
        ptrs = (ctypes.c_void_p * n)(*[im.ctypes.data for im in imgs])
        w = np.array([im.shape[1] for im in imgs], np.int32)
        h = np.array([im.shape[0] for im in imgs], np.int32)
        s = np.array([im.strides[0] for im in imgs], np.int32)
        if n and colour[0]:
            check(self._lib.sdm_upload_images_bgr_u8(self._h, ptrs, _ip(w), _ip(h), _ip(s), n, int(gray_shift)))
        else:
            check(self._lib.sdm_upload_images_u8(self._h, ptrs, _ip(w), _ip(h), _ip(s), n))
        self._image_sizes = list(zip(w.tolist(), h.tolist()))
        self._frames_keep = None

    def download_images(self, n: int, width: int, height: int) -> np.ndarray:
        """The first ``n`` equally sized images of the context's single-channel image set (tests of the gray conversion)."""
        out = np.empty((n, height, width), np.uint8)
        check(self._lib.sdm_debug_download_images(self._h, out.ctypes.data, n, width, height))
        return out

    def set_images_device(self, dev_ptr: int, n_images: int, width: int, height: int, stride: int):
        check(self._lib.sdm_set_images_device(self._h, ctypes.c_void_p(dev_ptr), n_images, width, height, stride))
        self._image_sizes = [(int(width), int(height))] * int(n_images)
        self._frames_keep = None

    def set_frames_device(self, frames, formats=None, gray_shift: int = 14, chroma=None):
        """Frames that are already on the device as the image set (sdm_set_frames_device): image i is frame i.  ``frames``: a list
        of uint8 device tensors -- H x W gray, H x W x 3 ("bgr", default, or "rgb"), H x W x 4 ("bgra", default, or "rgba"); any row
        stride, so views into larger frames work -- and / or (ptr, w, h, stride_bytes, format) tuples (format by name or
        SDM_FRAME_*: "nv12" with ptr = the Y plane; foreign allocators); or one stacked tensor n x H x W [x C].  ``formats``: one
        name for all tensors or one per frame.  Gray and NV12 frames are used in place -- the context keeps a reference to the
        tensors until the image set is replaced; memory behind a tuple is the caller's to keep alive -- colour frames are converted
        once, in one launch, with ``upload_images``' arithmetic.  A 3 x H x W tensor named "bgr_planar" / "rgb_planar" (or one stacked
        n x 3 x H x W tensor) is a planar colour frame, read where it lies whatever its row and channel strides
        (``_lib.frame_planes``); ``chroma``: the second planes of planar tuples.  A YUV frame's name is base[:matrix][:range] --
        "nv12:bt709" (1080p and above), "nv12:bt601:full", "p010:bt2020" (16-bit words, the sample in bits 15..6; converted to
        gray here, read in place by the crop and warp calls); "nv12" alone keeps BT.601 limited range with OpenCV's constants
        (include/sdm.h, "YUV colour description and 10-bit surfaces").  torch's current stream is synchronised first: the
        library runs on a stream of its own."""
        desc, planes = _lib.frame_planes(frames, formats, chroma)
        for t in ([frames] if _lib._is_tensor(frames) else frames):
            if getattr(t, "is_cuda", False):
                import torch
                torch.cuda.current_stream(t.device).synchronize()
                break
        arr = (_lib.SdmFrame * len(desc))(*[_lib.SdmFrame(ctypes.c_void_p(p), w, h, st, f) for p, w, h, st, f in desc])
        check(self._lib.sdm_set_frames_device_planes(self._h, arr, _lib.planes_array(planes), len(desc), int(gray_shift)))
        self._image_sizes = [(w, h) for _, w, h, _, _ in desc]
        self._frames_keep = frames

    def download_image(self, i: int, width: Optional[int] = None, height: Optional[int] = None) -> np.ndarray:
        """Image ``i`` of the current image set, whichever call installed it, read back through the image table (H x W uint8).
        Its size is known after ``set_frames_device`` / ``set_images_device``; otherwise give ``width`` and ``height``."""
        if width is None or height is None:
            sizes = getattr(self, "_image_sizes", None)
            if not sizes or not 0 <= i < len(sizes):
                raise ValueError("give width and height: the size of this image is not known to the Python layer")
            width, height = sizes[i]
        out = np.empty((int(height), int(width)), np.uint8)
        check(self._lib.sdm_debug_download_image(self._h, int(i), out.ctypes.data))
        return out

    def set_sample_image_index(self, idx: Optional[np.ndarray]):
        if idx is None:
            check(self._lib.sdm_set_sample_image_index(self._h, None, 0))
        else:
            a = np.ascontiguousarray(idx, np.int32)
            check(self._lib.sdm_set_sample_image_index(self._h, _ip(a), a.size))

    def set_x(self, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != 2 * self.L:
            raise ValueError("x must be N x 2L")
        check(self._lib.sdm_set_x(self._h, _fp(x), x.shape[0]))
        self.N = x.shape[0]

    def init_from_boxes(self, mean: np.ndarray, boxes: np.ndarray, perturbations: Optional[np.ndarray] = None,
                        fetch: bool = False) -> Optional[np.ndarray]:
        """x_n = rcr::align_mean(mean, box_n) (model.hpp:64-76) -- or align_mean(mean, perturb(box_n, t_n))
        (rcr-train.cpp:130-146) -- evaluated on the device into the state x.  boxes: N x (x, y, w, h) ints;
        perturbations: N x (translation_x, translation_y, scaling)."""
        m = np.ascontiguousarray(mean, np.float32).reshape(-1)
        b = np.ascontiguousarray(boxes, np.int32)
        if m.size != 2 * self.L or b.ndim != 2 or b.shape[1] != 4:
            raise ValueError("mean must have 2L entries, boxes must be N x 4")
        p = None
        if perturbations is not None:
            p = np.ascontiguousarray(perturbations, np.float32)
            if p.shape != (b.shape[0], 3):
                raise ValueError("perturbations must be N x 3")
        out = np.empty((b.shape[0], 2 * self.L), np.float32) if fetch else None
        check(self._lib.sdm_init_from_boxes(self._h, m.ctypes.data, b.ctypes.data, p.ctypes.data if p is not None else None,
                                            b.shape[0], out.ctypes.data if fetch else None))
        self.N = b.shape[0]
        return out

    def normalised_errors(self, fetch: bool = True):
        """calculate_normalised_landmark_errors (rcr-train.cpp:200-212) of the current x against the targets:
        returns (N x L matrix of ||x_i - x*_i|| / IED(x) or None, its mean)."""
        out = np.empty((self.N, self.L), np.float32) if fetch else None
        mean = ctypes.c_double(0.0)
        check(self._lib.sdm_normalised_errors(self._h, out.ctypes.data if fetch else None, ctypes.byref(mean)))
        return out, float(mean.value)

    def set_x_device(self, dev_ptr: int, n: int):
        check(self._lib.sdm_set_x_device(self._h, ctypes.c_void_p(dev_ptr), n))
        self.N = n

    def get_x(self) -> np.ndarray:
        out = np.empty((self.N, 2 * self.L), np.float32)
        check(self._lib.sdm_get_x(self._h, _fp(out)))
        return out

    # -- cascade steps ---------------------------------------------------------------------------
    def hog_features(self, level: int, fetch: bool = False) -> Optional[np.ndarray]:
        if fetch:
            out = np.empty((self.N, self.feature_dim(level)), np.float32)
            check(self._lib.sdm_hog_features(self._h, level, _fp(out)))
            return out
        check(self._lib.sdm_hog_features(self._h, level, None))
        return None

    def patch_indices(self) -> np.ndarray:
        out = np.empty((self.N, 1 + 2 * self.L), np.int32)
        check(self._lib.sdm_get_patch_indices(self._h, _ip(out)))
        return out

    def set_regressor(self, level: int, R: np.ndarray, token=None):
        """Uploads R as the regressor of ``level``.  ``token`` (any object) names what the device now holds; whoever writes
        the level's device copy -- this call or ``solve`` -- replaces it (``resident_token``)."""
        R = np.ascontiguousarray(R, np.float32)
        if R.shape != (self.feature_dim(level), 2 * self.L):
            raise ValueError(f"regressor must be {self.feature_dim(level)} x {2 * self.L}")
        self._resident.pop(level, None)
        check(self._lib.sdm_set_regressor(self._h, level, _fp(R)))
        if token is not None:
            self._resident[level] = token

    def resident_token(self, level: int):
        return self._resident.get(level)

    def set_resident_token(self, level: int, token):
        """Names the device copy ``solve`` just left behind (the optimiser that called it knows which regressor it is)."""
        if token is None:
            self._resident.pop(level, None)
        else:
            self._resident[level] = token

    def get_regressor(self, level: int) -> np.ndarray:
        out = np.empty((self.feature_dim(level), 2 * self.L), np.float32)
        check(self._lib.sdm_get_regressor(self._h, level, _fp(out)))
        return out

    def apply(self, level: int):
        check(self._lib.sdm_apply(self._h, level))

    def detect_level(self, level: int):
        """One cascade level of ``detect_batch`` (same launches, same bits): x_{k+1} replaces x_k on the device."""
        check(self._lib.sdm_detect_level(self._h, level))

    def detect_batch(self, fetch: bool = True) -> Optional[np.ndarray]:
        if fetch:
            out = np.empty((self.N, 2 * self.L), np.float32)
            check(self._lib.sdm_detect_batch(self._h, _fp(out)))
            return out
        check(self._lib.sdm_detect_batch(self._h, None))
        return None

    # -- training ----------------------------------------------------------------------------------
    def set_templates(self, templates: Optional[np.ndarray]):
        """Known-template mode: features - templates from now on (None / empty clears it)."""
        if templates is None or np.size(templates) == 0:
            check(self._lib.sdm_set_templates(self._h, None, 0, 0))
            return
        t = np.ascontiguousarray(templates, np.float32)
        check(self._lib.sdm_set_templates(self._h, t.ctypes.data, t.shape[0], t.shape[1]))

    def set_targets(self, xstar: np.ndarray):
        xs = np.ascontiguousarray(xstar, np.float32)
        check(self._lib.sdm_set_targets(self._h, _fp(xs), xs.shape[0]))

    def gram_rhs(self, level: int):
        check(self._lib.sdm_gram_rhs(self._h, level))

    def set_allreduce(self, fn: Optional[Callable[[int, int, int], int]], world_size: int):
        """``fn(dev_ptr, count_f32, hip_stream) -> 0`` sums the buffer over all ranks in place."""
        if fn is None:
            cb = _lib.ALLREDUCE_FN()
        else:
            def tramp(ptr, count, stream, _user):
                try:
                    return int(fn(ptr, count, stream) or 0)
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _lib.ALLREDUCE_FN(tramp)
        check(self._lib.sdm_set_allreduce(self._h, cb, None, world_size))
        self._keep_allreduce = cb       # (replaces the previous thunk, which the library no longer references)

    def set_allreduce_rccl(self, comm, world_size: int = 1, allreduce_fn=None):
        """The exchange through RCCL called by the library itself on its own stream (include/sdm.h: sdm_set_allreduce_rccl);
        ``comm`` = ncclComm_t of this rank (``parallel.RcclCommunicator``), ``None`` uninstalls."""
        check(self._lib.sdm_set_allreduce_rccl(self._h, comm, allreduce_fn, world_size))
        self._keep_allreduce = None

    def allreduce_gram_rhs(self):
        check(self._lib.sdm_allreduce_gram_rhs(self._h))

    def set_solve_sharding(self, rank: int, world_size: int, bcast: Optional[Callable[[int, int, int, int], int]],
                           allgather: Optional[Callable[[int, int, int, int], int]]):
        """Sharded factorisation inside ``solve`` (include/sdm.h: sdm_set_solve_sharding): rank ``rank`` of ``world_size``
        works on the tile columns ``j % world_size == rank``.  ``bcast(dev_ptr, count_f32, root, hip_stream) -> 0`` and
        ``allgather(send_ptr, recv_ptr, count_f32_per_rank, hip_stream) -> 0`` must be stream-ordered.  ``None`` for both
        restores the replicated solve."""
        if bcast is None and allgather is None:
            check(self._lib.sdm_set_solve_sharding(self._h, 0, 0, _lib.BCAST_FN(), _lib.ALLGATHER_FN(), None))
            self._keep_sharding = None
            return

        def guard(fn):
            def tramp(*args):
                try:
                    return int(fn(*args[:-1]) or 0)
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            return tramp
        b, g = _lib.BCAST_FN(guard(bcast)), _lib.ALLGATHER_FN(guard(allgather))
        check(self._lib.sdm_set_solve_sharding(self._h, rank, world_size, b, g, None))
        self._keep_sharding = (b, g)    # (replaces the previous pair: nothing accumulates over train() calls)

    def set_solve_sharding_rccl(self, comm: Optional[int], rank: int = 0, world_size: int = 1, bcast_fn: Optional[int] = None,
                                allgather_fn: Optional[int] = None):
        """The same through RCCL called by the library on its own stream; ``comm`` = ncclComm_t (None uninstalls)."""
        check(self._lib.sdm_set_solve_sharding_rccl(self._h, comm, rank, world_size, bcast_fn, allgather_fn))

    def set_reduce_scatter(self, fn: Optional[Callable[[int, int, int, int], int]]):
        """Reduce-scatter form of the Gram exchange (include/sdm.h: sdm_set_reduce_scatter), taken by ``allreduce_gram_rhs`` when the
        solve is sharded over the same ranks: ``fn(send_ptr, recv_ptr, count_f32_per_rank, hip_stream) -> 0`` leaves the sum over
        the ranks of this rank's chunk at ``recv_ptr``.  ``None`` restores the all-reduce."""
        if fn is None:
            check(self._lib.sdm_set_reduce_scatter(self._h, _lib.ALLGATHER_FN(), None))
            self._keep_reduce_scatter = None
            return

        def tramp(send, recv, count, stream, _user):
            try:
                return int(fn(send, recv, count, stream) or 0)
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = _lib.ALLGATHER_FN(tramp)
        check(self._lib.sdm_set_reduce_scatter(self._h, cb, None))
        self._keep_reduce_scatter = cb

    def set_reduce_scatter_rccl(self, enable: bool, reduce_scatter_fn: Optional[int] = None):
        """The same through ``ncclReduceScatter`` on the communicator of ``set_allreduce_rccl``."""
        check(self._lib.sdm_set_reduce_scatter_rccl(self._h, int(bool(enable)), reduce_scatter_fn))

    def solve(self, level: int, reg_type: int, reg_param: float, regularise_last_row: bool,
              n_train_global: int = 0, fetch: bool = True):
        lam = ctypes.c_float(0.0)
        R = np.empty((self.feature_dim(level), 2 * self.L), np.float32) if fetch else None
        self._resident.pop(level, None)                     # the device copy of this level is overwritten
        check(self._lib.sdm_solve(self._h, level, reg_type, reg_param, int(regularise_last_row),
                                  n_train_global, _fp(R) if fetch else None, ctypes.byref(lam)))
        return R, lam.value

    def set_solver(self, solver):
        """Which of the reference's solvers ``solve`` / ``solve_normal_equations`` / ``train_level`` run: ``"cholesky"`` (default;
        PartialPivLUSolver's role) or ``"colpivqr"`` (ColPivHouseholderQRSolver, regressors.hpp:242-306, on the device)."""
        kind = {"cholesky": 0, "lu": 0, "colpivqr": 1, "qr": 1}.get(solver, solver) if isinstance(solver, str) else int(solver)
        check(self._lib.sdm_set_solver(self._h, int(kind)))

    def last_rank(self):
        """``(rank, full_rank)`` of the last column-pivoted QR: qr_of_AtA.rank() and the matrix order (regressors.hpp:288-292)."""
        r, f = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.sdm_last_rank(self._h, ctypes.byref(r), ctypes.byref(f)))
        return r.value, f.value

    def solve_normal_equations(self, data: np.ndarray, labels: np.ndarray, reg_type: int = 0, reg_param: float = 0.0,
                               regularise_last_row: bool = True, solver=None, return_rank: bool = False):
        """Solver::solve(data, labels, regulariser) of regressors.hpp:199-234 on the GPU, for host matrices.  ``solver``: None = the
        handle's (``set_solver``), or "cholesky" / "colpivqr" for this call only (the handle's choice is left alone);
        ``return_rank``: also return (rank, full rank) as regressors.hpp:288-292 sees them."""
        A = np.ascontiguousarray(data, np.float32)
        b = np.ascontiguousarray(labels, np.float32)
        R = np.empty((A.shape[1], b.shape[1]), np.float32)
        lam = ctypes.c_float(0.0)
        if solver is None and not return_rank:
            check(self._lib.sdm_solve_normal_equations(self._h, _fp(A), A.shape[0], A.shape[1], _fp(b), b.shape[1], reg_type,
                                                       reg_param, int(regularise_last_row), _fp(R), ctypes.byref(lam)))
            return R, lam.value
        kind = {"cholesky": 0, "lu": 0, "colpivqr": 1, "qr": 1}.get(solver, solver) if isinstance(solver, str) else solver
        if kind is None:
            raise ValueError("return_rank needs the solver named for the call")
        rank, full = ctypes.c_int(-1), ctypes.c_int(0)
        check(self._lib.sdm_solve_normal_equations_with(self._h, int(kind), _fp(A), A.shape[0], A.shape[1], _fp(b), b.shape[1], reg_type,
                                                        reg_param, int(regularise_last_row), _fp(R), ctypes.byref(lam),
                                                        ctypes.byref(rank), ctypes.byref(full)))
        return (R, lam.value, (rank.value, full.value)) if return_rank else (R, lam.value)

    def train_level(self, level: int, reg_type: int, reg_param: float, regularise_last_row: bool,
                    n_train_global: int = 0):
        self._resident.pop(level, None)
        check(self._lib.sdm_train_level(self._h, level, reg_type, reg_param, int(regularise_last_row),
                                        n_train_global))

    def train_level_sweep(self, level: int, reg_type: int, reg_params, regularise_last_row: bool, n_fit_rows: int,
                          n_train_global: int = 0):
        """One training level with K regulariser candidates on ONE feature extraction and Gram product (include/sdm.h:
        sdm_train_level_sweep): rows [0, n_fit_rows) are fitted, the rows behind them held out; the candidate with the lowest
        held-out mean normalised error becomes the level's regressor and is applied to all rows.  Returns a dict: ``params``,
        ``lambdas``, ``holdout_errors``, ``fit_errors`` (float64, +inf for a failed candidate), ``status`` (0 or SDM_ERR_NOT_SPD per
        candidate), ``best``.  If every candidate failed the call raises SdmError(SDM_ERR_NOT_SPD) and the state is untouched."""
        params = np.ascontiguousarray(np.atleast_1d(np.asarray(reg_params, np.float32)).reshape(-1))
        K = int(params.size)
        hold, fit = np.full(max(K, 1), np.inf, np.float64), np.full(max(K, 1), np.inf, np.float64)
        lam, status = np.zeros(max(K, 1), np.float32), np.zeros(max(K, 1), np.int32)
        best = ctypes.c_int(-1)
        self._resident.pop(level, None)                     # the device copy of this level is overwritten
        check(self._lib.sdm_train_level_sweep(self._h, level, int(reg_type), params.ctypes.data, K, int(bool(regularise_last_row)),
                                              int(n_train_global), int(n_fit_rows), hold.ctypes.data, fit.ctypes.data,
                                              lam.ctypes.data, status.ctypes.data, ctypes.byref(best)))
        self._sweep_level = level
        return {"params": params, "lambdas": lam[:K], "holdout_errors": hold[:K], "fit_errors": fit[:K], "status": status[:K],
                "best": int(best.value)}

    def sweep_regressor(self, k: int) -> np.ndarray:
        """Candidate ``k`` of the last ``train_level_sweep`` (F x 2L, as ``get_regressor``)."""
        out = np.empty((self.feature_dim(getattr(self, "_sweep_level", 0)), 2 * self.L), np.float32)
        check(self._lib.sdm_sweep_get_regressor(self._h, int(k), _fp(out)))
        return out

    # -- head pose (sdm_pose_*: the ModelProjection cascade, state beside the landmark state) -------------------------------
    def pose_set_model(self, points: np.ndarray, focal: float = 1800.0, width: float = 1000.0, height: float = 1000.0,
                       near: float = 1.0, far: float = 5000.0):
        """``points``: K x 3 model coordinates.  Camera defaults: examples/pose_estimation.cpp:205-211."""
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("pose model points must be K x 3")
        check(self._lib.sdm_pose_set_model(self._h, p.ctypes.data, p.shape[0], focal, width, height, near, far))
        self.pose_K = p.shape[0]

    def pose_set_x(self, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != 6:
            raise ValueError("pose parameters must be N x 6")
        check(self._lib.sdm_pose_set_x(self._h, x.ctypes.data, x.shape[0]))
        self.pose_N = x.shape[0]

    def pose_set_x_device(self, dev_ptr: int, n: int):
        check(self._lib.sdm_pose_set_x_device(self._h, ctypes.c_void_p(dev_ptr), n))
        self.pose_N = n

    def pose_get_x(self) -> np.ndarray:
        out = np.empty((self.pose_N, 6), np.float32)
        check(self._lib.sdm_pose_get_x(self._h, out.ctypes.data))
        return out

    def pose_set_templates(self, templates: np.ndarray):
        t = np.ascontiguousarray(templates, np.float32)
        if t.ndim != 2:
            raise ValueError("pose templates must be N x 2K")
        check(self._lib.sdm_pose_set_templates(self._h, t.ctypes.data, t.shape[0], t.shape[1]))

    def pose_templates_from_landmarks(self, landmark_index: Sequence[int], focal: float):
        """Templates of every row of the LANDMARK state (e.g. after ``detect_batch``), gathered and normalised by each row's
        image centre on the device."""
        idx = np.ascontiguousarray(landmark_index, np.int32)
        check(self._lib.sdm_pose_templates_from_landmarks(self._h, idx.ctypes.data, idx.size, float(focal)))

    def pose_set_targets(self, xstar: np.ndarray):
        xs = np.ascontiguousarray(xstar, np.float32)
        check(self._lib.sdm_pose_set_targets(self._h, xs.ctypes.data, xs.shape[0]))

    def pose_features(self, level: int = 0) -> np.ndarray:
        out = np.empty((self.pose_N, 2 * self.pose_K), np.float32)
        check(self._lib.sdm_pose_features(self._h, level, out.ctypes.data))
        return out

    def pose_train_level(self, level: int, reg_type: int, reg_param: float, regularise_last_row: bool):
        """One training level on the device; returns (R (2K x 6), lambda).  x becomes x_{k+1}."""
        R = np.empty((2 * self.pose_K, 6), np.float32)
        lam = ctypes.c_float(0.0)
        check(self._lib.sdm_pose_train_level(self._h, level, int(reg_type), float(reg_param), int(bool(regularise_last_row)),
                                             R.ctypes.data, ctypes.byref(lam)))
        return R, lam.value

    def pose_set_regressor(self, level: int, R: np.ndarray):
        R = np.ascontiguousarray(R, np.float32)
        if R.shape != (2 * self.pose_K, 6):
            raise ValueError(f"pose regressor must be {2 * self.pose_K} x 6")
        check(self._lib.sdm_pose_set_regressor(self._h, level, R.ctypes.data))

    def pose_get_regressor(self, level: int) -> np.ndarray:
        out = np.empty((2 * self.pose_K, 6), np.float32)
        check(self._lib.sdm_pose_get_regressor(self._h, level, out.ctypes.data))
        return out

    def pose_test(self, first_level: int, n_levels: int):
        """Levels first_level .. first_level + n_levels - 1 in one launch."""
        check(self._lib.sdm_pose_test(self._h, first_level, n_levels))

    # -- multi-stream tracking (csrc/sdm_track.hip) ---------------------------------------------------
    @staticmethod
    def _ids(ids) -> np.ndarray:
        return np.ascontiguousarray(np.atleast_1d(np.asarray(ids)), np.int32).reshape(-1)

    def track_configure(self, capacity: int, mean: np.ndarray, init_mode: int, min_size: float, max_scale_change: float):
        m = np.ascontiguousarray(mean, np.float32).reshape(-1)
        if m.size != 2 * self.L:
            raise ValueError("the mean must hold 2L coordinates")
        check(self._lib.sdm_track_configure(self._h, int(capacity), m.ctypes.data, int(init_mode), float(min_size),
                                            float(max_scale_change)))

    def track_start(self, ids, boxes: np.ndarray):
        i = self._ids(ids)
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        if b.shape[0] != i.size:
            raise ValueError("one face box (x, y, w, h) per stream id expected")
        check(self._lib.sdm_track_start(self._h, i.ctypes.data, b.ctypes.data, i.size))

    def track_stop(self, ids):
        i = self._ids(ids)
        check(self._lib.sdm_track_stop(self._h, i.ctypes.data, i.size))

    def track_step(self, ids, fetch: bool = True):
        """One frame for the streams ``ids`` (row i of the current images belongs to ids[i]): returns (landmarks n x 2L or None,
        lost masks n).  The rows are the current x afterwards."""
        i = self._ids(ids)
        out = np.empty((i.size, 2 * self.L), np.float32) if fetch else None
        lost = np.empty(i.size, np.int32)
        rc = self._lib.sdm_track_step(self._h, i.ctypes.data, i.size, out.ctypes.data if fetch else None, lost.ctypes.data)
        if rc in (_lib.SDM_OK, _lib.SDM_ERR_EMPTY_PATCH):      # (the step was committed)
            self.N = i.size
            if getattr(self, "track_upright", False):
                self.upright_N = i.size
        check(rc)
        return out, lost

    def track_get(self, ids):
        i = self._ids(ids)
        out = np.empty((i.size, 2 * self.L), np.float32)
        st = np.empty(i.size, np.int32)
        check(self._lib.sdm_track_get(self._h, i.ctypes.data, i.size, out.ctypes.data, st.ctypes.data))
        return out, st

    # -- the tracker's temporal landmark filter (csrc/sdm_track_filter.hip) --------------------------
    def track_configure_filter(self, min_cutoff: Optional[float] = None, beta: float = 0.0, d_cutoff: float = 1.0):
        """The One-Euro filter on the tracker's output (include/sdm.h, "Tracking, filtered"): ``min_cutoff`` > 0 Hz, ``beta`` >= 0 Hz
        per face size per second, ``d_cutoff`` > 0 Hz; every slot un-primed.  ``min_cutoff`` None: the filter off."""
        if min_cutoff is None:
            check(self._lib.sdm_track_configure_filter(self._h, _lib.SDM_TRACK_FILTER_OFF, 0.0, 0.0, 0.0))
        else:
            check(self._lib.sdm_track_configure_filter(self._h, _lib.SDM_TRACK_FILTER_ONE_EURO, float(min_cutoff), float(beta),
                                                       float(d_cutoff)))

    def track_step_filtered(self, ids, dt, fetch: bool = True):
        """``track_step`` with the filter behind it; ``dt``: seconds since the streams' last filtered step, one value or one per
        row.  Returns (filtered rows n x 2L or None, lost masks n, raw rows n x 2L or None); the FILTERED rows are the current x
        afterwards."""
        i = self._ids(ids)
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, np.float32).reshape(-1), (i.size,)), np.float32)
        raw = np.empty((i.size, 2 * self.L), np.float32) if fetch else None
        out = np.empty((i.size, 2 * self.L), np.float32) if fetch else None
        lost = np.empty(i.size, np.int32)
        rc = self._lib.sdm_track_step_filtered(self._h, i.ctypes.data, i.size, d.ctypes.data, raw.ctypes.data if fetch else None,
                                               lost.ctypes.data, out.ctypes.data if fetch else None)
        if rc in (_lib.SDM_OK, _lib.SDM_ERR_EMPTY_PATCH):      # (the step was committed)
            self.N = i.size
            if getattr(self, "track_upright", False):
                self.upright_N = i.size
        check(rc)
        return out, lost, raw

    def track_get_filtered(self, ids):
        """(filtered rows n x 2L, derivative rows n x 2L, primed flags n) of the streams ``ids``; zeros where a stream's filter holds
        nothing yet."""
        i = self._ids(ids)
        f = np.empty((i.size, 2 * self.L), np.float32)
        d = np.empty((i.size, 2 * self.L), np.float32)
        p = np.empty(i.size, np.int32)
        check(self._lib.sdm_track_get_filtered(self._h, i.ctypes.data, i.size, f.ctypes.data, d.ctypes.data, p.ctypes.data))
        return f, d, p

    # -- the tracker's motion-compensated initialisation (csrc/sdm_track_motion.hip) ----------------
    def track_configure_motion(self, search: Optional[int] = 8, scale: float = 1.25, min_gain: int = MOTION_MIN_GAIN):
        """Block matching ahead of every step (include/sdm.h, "Tracking, motion-compensated"): ``search`` 1 ... 16 chip pixels,
        ``scale`` in [0.5, 4] (the chip's side in face sizes), ``min_gain`` 0 ... 255 (how much, in 256ths, the best offset must beat
        staying in place); every slot invalid.  ``search`` None: the mode off."""
        if search is None:
            check(self._lib.sdm_track_configure_motion(self._h, _lib.SDM_TRACK_MOTION_OFF, 0, 0.0, 0))
        else:
            check(self._lib.sdm_track_configure_motion(self._h, _lib.SDM_TRACK_MOTION_SAD, int(search), float(scale), int(min_gain)))

    def track_get_motion(self, ids):
        """Of the streams ``ids``: (motion n x 6 int32 -- the last step's shift dx, dy in pixels, best SAD, SAD(0, 0), k, searched --,
        grid n x 3 int32 (k, ox, oy), chips n x 32 x 32 uint8); zeros where a stream holds nothing."""
        i = self._ids(ids)
        m = np.empty((i.size, 6), np.int32)
        g = np.empty((i.size, 3), np.int32)
        ch = np.empty((i.size, 32, 32), np.uint8)
        check(self._lib.sdm_track_get_motion(self._h, i.ctypes.data, i.size, m.ctypes.data, g.ctypes.data, ch.ctypes.data))
        return m, g, ch

    # -- upright-normalised detect and tracking (csrc/sdm_upright.hip) ------------------------------
    def upright_configure(self, chip: int, guard: int):
        """The size of the upright chips (32 ... 1024 pixels) and the NEAR_EDGE guard band (0 ... chip / 2 - 1 pixels)."""
        check(self._lib.sdm_upright_configure(self._h, int(chip), int(guard)))
        self.upright_chip = int(chip)

    def detect_batch_upright(self, mean: np.ndarray, boxes: np.ndarray, roll_deg, fetch: bool = True) -> Optional[np.ndarray]:
        """``detect_batch`` for rolled faces (include/sdm.h, sdm_detect_batch_upright): row i's face, in box i with a roll of
        ``roll_deg[i]`` degrees (clockwise positive), is cut upright from its frame, the cascade runs on the chips, the result comes
        back in frame coordinates and is the current x."""
        m = np.ascontiguousarray(mean, np.float32).reshape(-1)
        if m.size != 2 * self.L:
            raise ValueError("the mean must hold 2L coordinates")
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(roll_deg, np.float32).reshape(-1), (b.shape[0],)), np.float32)
        out = np.empty((b.shape[0], 2 * self.L), np.float32) if fetch else None
        rc = self._lib.sdm_detect_batch_upright(self._h, m.ctypes.data, b.ctypes.data, r.ctypes.data, b.shape[0],
                                                out.ctypes.data if fetch else None)
        if rc in (_lib.SDM_OK, _lib.SDM_ERR_EMPTY_PATCH):
            self.N = b.shape[0]
            self.upright_N = b.shape[0]
        check(rc)
        return out

    def upright_get(self, chips: bool = False):
        """Of the last upright call (detect or tracker step): (M n x 2 x 3 float32, chip -> frame; flags n int32, SDM_UPRIGHT_* bits)
        and, with ``chips``, the n x chip x chip uint8 chips the cascade ran on."""
        n = int(getattr(self, "upright_N", 0))
        mats = np.empty((n, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        chip = int(getattr(self, "upright_chip", 0))
        ch = np.empty((n, chip, chip), np.uint8) if chips and n else None
        check(self._lib.sdm_upright_get(self._h, mats.ctypes.data, flags.ctypes.data, ch.ctypes.data if ch is not None else None))
        return (mats, flags, ch) if chips else (mats, flags)

    def track_configure_upright(self, enable: bool = True):
        check(self._lib.sdm_track_configure_upright(self._h, 1 if enable else 0))
        self.track_upright = bool(enable)

    def track_start_rolled(self, ids, boxes: np.ndarray, roll_deg):
        i = self._ids(ids)
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        if b.shape[0] != i.size:
            raise ValueError("one face box (x, y, w, h) per stream id expected")
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(roll_deg, np.float32).reshape(-1), (i.size,)), np.float32)
        check(self._lib.sdm_track_start_rolled(self._h, i.ctypes.data, b.ctypes.data, r.ctypes.data, i.size))

    # -- aligned face crops (csrc/sdm_align.hip) -------------------------------------------------------
    def align_set_source(self, source=None):
        """The images the crops are cut from: None (the context's own images), a host uint8 array n x H x W [x C] (copied once),
        or a contiguous uint8 n x H x W [x C] tensor on the device (used in place; it must stay alive while crops are made).
        Returns C, which the next ``align_crops`` writes per pixel."""
        if source is None:
            check(self._lib.sdm_align_set_source(self._h, None, 0, 0, 0, 0, 0, 0))
            self.align_channels = 1
            return 1
        if hasattr(source, "data_ptr") and getattr(source, "is_cuda", False):
            import torch
            if source.dtype != torch.uint8 or source.dim() not in (3, 4) or not source.is_contiguous():
                raise ValueError("a device source must be a contiguous uint8 n x H x W [x C] tensor")
            torch.cuda.current_stream(source.device).synchronize()          # (the library runs on its own stream)
            shape, ptr, on_device = tuple(int(v) for v in source.shape), source.data_ptr(), 1
        else:
            if np.asarray(source).dtype != np.uint8:
                raise ValueError("a host source must be a uint8 array")
            source = np.ascontiguousarray(source)
            if source.ndim not in (3, 4):
                raise ValueError("a host source must be an n x H x W [x C] uint8 array")
            shape, ptr, on_device = source.shape, source.ctypes.data, 0
        n, h, w = shape[:3]
        C = shape[3] if len(shape) == 4 else 1
        check(self._lib.sdm_align_set_source(self._h, ctypes.c_void_p(ptr), n, w, h, w * C, C, on_device))
        self.align_channels = C
        return C

    def align_crops(self, landmark_index, template: np.ndarray, width: int, height: int, channels: Optional[int] = None, out=None):
        """Crops of the N current rows (include/sdm.h, sdm_align_crops) from the source set by ``align_set_source``: returns (crops
        N x height x width x C uint8 -- ``out`` itself when a device tensor is given, written in place and not fetched --,
        matrices N x 2 x 3 float32 (crop -> source), flags N int32: SDM_ALIGN_* bits).  C is the source's; ``channels``, when
        given, must equal it."""
        C = self.align_channels
        if channels is not None and int(channels) != C:
            raise ValueError(f"the crop source has {C} channel(s), not {channels}")
        idx = np.ascontiguousarray(landmark_index, np.int32).reshape(-1)
        t = np.ascontiguousarray(template, np.float32).reshape(-1, 2)
        if t.shape[0] != idx.size:
            raise ValueError("one template point (x, y) per landmark index expected")
        n = int(getattr(self, "N", 0))          # (0: no rows yet -- the library refuses the call)
        mats = np.empty((n, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        if out is not None:
            import torch
            if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor on the device")
            if tuple(out.shape) != (n, int(height), int(width), C):
                raise ValueError(f"out must be a {n} x {height} x {width} x {C} tensor")
            torch.cuda.current_stream(out.device).synchronize()
            check(self._lib.sdm_align_crops(self._h, idx.ctypes.data, t.ctypes.data, idx.size, int(width), int(height),
                                            ctypes.c_void_p(out.data_ptr()), 1, mats.ctypes.data, flags.ctypes.data))
            return out, mats, flags
        crops = np.empty((n, int(height), int(width), C), np.uint8)
        check(self._lib.sdm_align_crops(self._h, idx.ctypes.data, t.ctypes.data, idx.size, int(width), int(height),
                                        crops.ctypes.data, 0, mats.ctypes.data, flags.ctypes.data))
        return crops, mats, flags

    def align_set_source_frames(self, frames=None, formats=None, chroma=None):
        """A frame list as the crop source, used in place (sdm_align_set_source_frames): ``frames`` and ``formats`` as for
        ``set_frames_device`` -- every format --, ``chroma``: None or one entry per frame, the device pointer (or a uint8 tensor) of
        an NV12 frame's interleaved UV plane or of a planar colour tuple's second plane; None entries mean "directly behind the first
        plane".  ``frames`` None: back to the
        context's images.  The memory must stay valid while crops are made from it.  Returns C of ``align_crops`` on this source
        (the bytes per pixel all frames share), or None when only ``align_crops_tensor`` can read it (NV12, planar colour, mixed pixel sizes)."""
        if frames is None:
            check(self._lib.sdm_align_set_source_frames(self._h, None, None, 0))
            self.align_channels = 1
            return 1
        desc, planes = _lib.frame_planes(frames, formats, chroma)          # (a planar tensor's second plane comes from its strides)
        tensors = [frames] if _lib._is_tensor(frames) else list(frames)
        if chroma is not None:
            tensors += [u for u in chroma if _lib._is_tensor(u)]
        uv = _lib.planes_array(planes)
        for t in tensors:
            if getattr(t, "is_cuda", False):
                import torch
                torch.cuda.current_stream(t.device).synchronize()          # (the library runs on its own stream)
                break
        arr = (_lib.SdmFrame * len(desc))(*[_lib.SdmFrame(ctypes.c_void_p(p), w, h, st, f) for p, w, h, st, f in desc])
        check(self._lib.sdm_align_set_source_frames(self._h, arr, uv, len(desc)))
        kinds = {0 if _lib.frame_base(f) in (_lib.SDM_FRAME_NV12, _lib.SDM_FRAME_P010) or f in _lib._FRAME_PLANAR else _lib._FRAME_CHANNELS[f]
                 for _, _, _, _, f in desc}
        C = kinds.pop() if len(kinds) == 1 else 0
        self.align_channels = C if C else 1
        return C if C else None

    def _crop_tensor_out(self, spec, options, width, height, out):
        """What ``align_crops_tensor`` and ``warp_crops_tensor`` do alike before their call: the specification (``spec`` or the
        ``options`` of ``_lib.align_tensor_spec``), the output tensor (``out`` checked, or a new one) with torch's stream on its device
        synchronised -- the library runs on its own.  Returns (spec, out, rows)."""
        if spec is None:
            spec = _lib.align_tensor_spec(**options)
        elif options:
            raise ValueError("give either spec or the named options")
        n = int(getattr(self, "N", 0))          # (0: no rows yet -- the library refuses the call)
        shape = _lib.align_tensor_shape(n, width, height, spec.layout, spec.channels)
        name = {v: k for k, v in _lib.ALIGN_DTYPES.items()}[spec.dtype]
        import torch
        if out is None:
            out = torch.empty(shape, dtype=getattr(torch, name), device=f"cuda:{self.device}")
        else:
            _lib.check_align_out(out, shape, name)
        torch.cuda.current_stream(out.device).synchronize()
        return spec, out, n

    def align_crops_tensor(self, landmark_index, template: np.ndarray, width: int, height: int, spec=None, out=None, filter=None,
                           **options):
        """Crops of the N current rows as a network's input tensor (include/sdm.h, sdm_align_crops_tensor) from the source set by
        ``align_set_source_frames`` / ``align_set_source`` (default: the context's images).  ``spec``: an ``_lib.SdmAlignTensor``, or
        the ``options`` of ``_lib.align_tensor_spec`` (dtype, layout, channels, order, scale, bias, mean, std, gray_shift).  ``out``:
        a contiguous device tensor of the requested dtype and shape, written in place; default: a new one.  Returns (tensor
        N x C x H x W or N x H x W x C, matrices N x 2 x 3 float32, flags N int32).  ``filter``: None (plain bilinear), or "area" / an
        ``_lib.SdmAlignFilter`` (``_lib.align_filter``) for sdm_align_crops_tensor_filtered -- rows whose similarity minifies average
        S x S sub-samples per pixel -- which returns (tensor, matrices, flags, samples N int32: S of every row)."""
        if isinstance(filter, str):
            filter = _lib.align_filter(filter)
        elif filter is not None and not isinstance(filter, _lib.SdmAlignFilter):
            raise ValueError('filter must be None, "area", "bilinear" or an SdmAlignFilter')
        idx = np.ascontiguousarray(landmark_index, np.int32).reshape(-1)
        t = np.ascontiguousarray(template, np.float32).reshape(-1, 2)
        if t.shape[0] != idx.size:
            raise ValueError("one template point (x, y) per landmark index expected")
        spec, out, n = self._crop_tensor_out(spec, options, int(width), int(height), out)
        mats = np.empty((n, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        if filter is None:
            check(self._lib.sdm_align_crops_tensor(self._h, idx.ctypes.data, t.ctypes.data, idx.size, int(width), int(height), ctypes.byref(spec),
                                                   ctypes.c_void_p(out.data_ptr()), mats.ctypes.data, flags.ctypes.data))
            return out, mats, flags
        samples = np.empty(n, np.int32)
        check(self._lib.sdm_align_crops_tensor_filtered(self._h, idx.ctypes.data, t.ctypes.data, idx.size, int(width), int(height),
                                                        ctypes.byref(spec), ctypes.byref(filter), ctypes.c_void_p(out.data_ptr()),
                                                        mats.ctypes.data, flags.ctypes.data, samples.ctypes.data))
        return out, mats, flags, samples

    # -- piecewise-affine warped faces (csrc/sdm_warp.hip) ---------------------------------------------
    def warp_set_mesh(self, landmark_index, template: np.ndarray, triangles: np.ndarray, width: int, height: int):
        """The mesh of ``warp_crops_tensor`` (include/sdm.h, sdm_warp_set_mesh): K landmark indices, their K x 2 template points in crop
        pixels, T x 3 triangles over the positions 0 .. K - 1 (e.g. ``_lib.delaunay(template)``) and the crop size.  The label map is
        computed once, here."""
        idx = np.ascontiguousarray(landmark_index, np.int32).reshape(-1)
        t = np.ascontiguousarray(template, np.float32).reshape(-1, 2)
        if t.shape[0] != idx.size:
            raise ValueError("one template point (x, y) per landmark index expected")
        tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        check(self._lib.sdm_warp_set_mesh(self._h, idx.ctypes.data, t.ctypes.data, idx.size, tri.ctypes.data, tri.shape[0], int(width),
                                          int(height)))
        self.warp_mesh = (tri.shape[0], int(width), int(height))

    def warp_labels(self) -> np.ndarray:
        """The mesh's label map, height x width uint8: the triangle every crop pixel belongs to, 255 = none."""
        _, w, h = getattr(self, "warp_mesh", (0, 0, 0))
        out = np.empty((h, w), np.uint8)
        check(self._lib.sdm_warp_get_labels(self._h, out.ctypes.data))
        return out

    def warp_crops_tensor(self, spec=None, out=None, filter=None, **options):
        """The N current rows warped piecewise-affinely onto the mesh's template, as a network's input tensor (include/sdm.h,
        sdm_warp_crops_tensor), from the source ``align_crops_tensor`` reads.  ``spec`` / ``options`` / ``out``: as for
        ``align_crops_tensor``.  Returns (tensor N x C x H x W or N x H x W x C, matrices N x T x 2 x 3 float32 crop -> source, one per
        triangle, flags N int32: SDM_WARP_* bits).  ``filter``: None (plain bilinear), or "area" / "bilinear" / an
        ``_lib.SdmAlignFilter`` (``_lib.align_filter``) for sdm_warp_crops_tensor_filtered -- every pixel of a triangle whose map
        minifies averages Sx x Sy sub-samples -- which returns (tensor, matrices, flags, samples N x T x 2 int32: (Sx, Sy) of every
        triangle)."""
        if isinstance(filter, str):
            filter = _lib.align_filter(filter)
        elif filter is not None and not isinstance(filter, _lib.SdmAlignFilter):
            raise ValueError('filter must be None, "area", "bilinear" or an SdmAlignFilter')
        T, width, height = getattr(self, "warp_mesh", (0, 0, 0))
        spec, out, n = self._crop_tensor_out(spec, options, width, height, out)
        mats = np.empty((n, T, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        if filter is None:
            check(self._lib.sdm_warp_crops_tensor(self._h, ctypes.byref(spec), ctypes.c_void_p(out.data_ptr()), mats.ctypes.data,
                                                  flags.ctypes.data))
            return out, mats, flags
        samples = np.empty((n, T, 2), np.int32)
        check(self._lib.sdm_warp_crops_tensor_filtered(self._h, ctypes.byref(spec), ctypes.byref(filter), ctypes.c_void_p(out.data_ptr()),
                                                       mats.ctypes.data, flags.ctypes.data, samples.ctypes.data))
        return out, mats, flags, samples

    # -- crop tensors pasted back into frames (csrc/sdm_align_paste.hip) ------------------------------
    def _paste_call(self, y, layout, frames, formats, mask, spec, options):
        """What the two paste calls do alike before their call: the tensor (a contiguous uint8 / float16 / float32 device tensor,
        N x C x H x W or N x H x W x C by ``layout``, C in {1, 3}) gives dtype, channels and the crop size of the specification (``spec``,
        or the ``options`` of ``_lib.paste_tensor_spec``); the frames' descriptors; the opacity (``mask``: None, or an H x W or
        N x H x W uint8 device tensor or numpy array).  torch's stream is synchronised: the library runs on its own.  Returns
        (spec, paste, frame array, rows, width, height, what must stay alive over the call)."""
        import torch
        if not (isinstance(y, torch.Tensor) and y.is_cuda and y.is_contiguous() and y.dim() == 4):
            raise ValueError("the tensor must be a contiguous 4-dimensional tensor on the device")
        name = str(y.dtype).split(".")[-1]
        if name not in _lib.ALIGN_DTYPES:
            raise ValueError(f"the tensor must be uint8, float16 or float32, not {y.dtype}")
        if not isinstance(layout, str) or layout.lower() not in _lib.ALIGN_LAYOUTS:
            raise ValueError(f"unknown layout {layout!r}: one of {sorted(_lib.ALIGN_LAYOUTS)}")
        n, (channels, height, width) = int(y.shape[0]), ([int(v) for v in y.shape[1:]] if layout.lower() == "nchw"
                                                         else [int(y.shape[3]), int(y.shape[1]), int(y.shape[2])])
        if spec is None:
            spec = _lib.paste_tensor_spec(name, layout, channels, **options)
        elif options:
            raise ValueError("give either spec or the named options")
        elif (spec.dtype, spec.layout, spec.channels) != (_lib.ALIGN_DTYPES[name], _lib.ALIGN_LAYOUTS[layout.lower()], channels):
            raise ValueError("spec does not describe this tensor")
        alpha = None
        if mask is not None:
            alpha = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(y.device)
            if not alpha.is_cuda or alpha.dtype != torch.uint8 or not alpha.is_contiguous() or \
                    tuple(alpha.shape) not in ((height, width), (n, height, width)):
                raise ValueError(f"mask must be a contiguous uint8 {height} x {width} or {n} x {height} x {width} array or device tensor")
        paste = _lib.SdmAlignPaste(None if alpha is None else alpha.data_ptr(), int(alpha is not None and alpha.dim() == 3))
        desc, planes = _lib.frame_planes(frames, formats)                  # (planes: planar tensors' second planes, for _paste_chroma)
        arr = (_lib.SdmFrame * len(desc))(*[_lib.SdmFrame(ctypes.c_void_p(p), w, h, st, f) for p, w, h, st, f in desc])
        torch.cuda.current_stream(y.device).synchronize()
        return spec, paste, arr, n, width, height, (alpha, frames), planes

    def _paste_rows(self, n):                                   # the fit forms: the tensor's rows are the context's current rows
        if int(getattr(self, "N", 0)) and n != self.N:          # (no rows yet: the library refuses the call)
            raise ValueError(f"the tensor has {n} rows, the context {int(getattr(self, 'N', 0))}")

    def _paste_image_index(self, image_index, n):               # the ``_at`` forms: None, or one int32 per row
        idx = None if image_index is None else np.ascontiguousarray(image_index, np.int32).reshape(-1)
        if idx is not None and idx.size != n:
            raise ValueError("one image index per row expected")
        return idx

    @staticmethod
    def _paste_filter(filter, max_samples, min_scale):
        """None, or the ``SdmAlignFilter`` of a paste call's ``filter`` ("area" | "bilinear" with ``max_samples`` / ``min_scale``, or
        an ``SdmAlignFilter`` as it is)"""
        if filter is None or isinstance(filter, _lib.SdmAlignFilter):
            return filter
        if isinstance(filter, str):
            return _lib.align_filter(filter, max_samples, min_scale)
        raise ValueError('filter must be None, "area", "bilinear" or an SdmAlignFilter')

    @staticmethod
    def _paste_chroma(chroma, arr, keep, planes=None):
        """The NV12 calls' second planes: None unless a destination is NV12, ``chroma`` is given or a planar tensor's plane distance
        is not the default (``planes``: what ``_lib.frame_planes`` found in the tensors' strides) -- then (the c_void_p array or None,
        what must stay alive).  ``chroma``: one entry per frame as ``align_set_source_frames`` takes it -- a device pointer, a uint8
        tensor or None (directly behind the first plane)."""
        planes = list(planes or [None] * len(arr))
        if chroma is None and all(p is None for p in planes):
            return (None, keep) if any(_lib.frame_base(f.format) == _lib.SDM_FRAME_NV12 for f in arr) else None
        if chroma is not None:
            if len(chroma) != len(arr):
                raise ValueError("one chroma entry (or None) per frame expected")
            planes = [p if u is None else int(u.data_ptr()) if _lib._is_tensor(u) else int(u) for p, u in zip(planes, chroma)]
        return (ctypes.c_void_p * len(arr))(*planes), (keep, chroma)

    def align_paste_tensor(self, landmark_index, template: np.ndarray, y, frames, formats=None, layout="nchw", mask=None, spec=None,
                           filter=None, max_samples=16, min_scale=1.0, chroma=None, **options):
        """The inverse of ``align_crops_tensor`` for the N current rows (include/sdm.h, sdm_align_paste_tensor): ``y`` -- a network's
        output on the crops, a device tensor whose dtype, channels and crop size are read from it -- is warped back through every row's
        fitted similarity and blended into ``frames`` IN PLACE.  ``frames`` / ``formats``: as for ``set_frames_device``;
        row n goes to the frame ``set_sample_image_index`` names.  ``mask``: the crop-space opacity, None (255 inside the crop) or an
        H x W (all rows) or N x H x W uint8 device tensor or numpy array.  ``options``: order, scale, bias, mean, std, gray_shift of
        ``_lib.paste_tensor_spec`` (an element is decoded as e * scale + bias: ``mean`` / ``std`` as in the crop call undo it).  Returns
        (matrices N x 2 x 3 float32 crop -> frame, flags N int32: SDM_ALIGN_* bits).  ``filter``: None (plain bilinear), or "area" /
        "bilinear" with ``max_samples`` and ``min_scale`` (``_lib.align_filter``) or an ``SdmAlignFilter`` for
        sdm_align_paste_tensor_filtered -- a row whose crop outsizes its face averages S x S sub-samples per frame pixel -- which
        returns (matrices, flags, samples N int32: S of every row).  With an "nv12" destination among ``frames``, or ``chroma`` given
        (per frame the UV plane's device pointer, a uint8 tensor or None, as for ``align_set_source_frames``), the call is
        sdm_align_paste_tensor_nv12: luma and 4:2:0 chroma blended in place; the return values are the same."""
        filter = self._paste_filter(filter, max_samples, min_scale)
        idx = np.ascontiguousarray(landmark_index, np.int32).reshape(-1)
        t = np.ascontiguousarray(template, np.float32).reshape(-1, 2)
        if t.shape[0] != idx.size:
            raise ValueError("one template point (x, y) per landmark index expected")
        spec, paste, arr, n, width, height, keep, planes = self._paste_call(y, layout, frames, formats, mask, spec, options)
        self._paste_rows(n)
        mats = np.empty((n, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        nv12 = self._paste_chroma(chroma, arr, keep, planes)
        if nv12 is not None:
            samples = np.empty(n, np.int32)
            check(self._lib.sdm_align_paste_tensor_nv12(self._h, idx.ctypes.data, t.ctypes.data, idx.size, width, height, ctypes.byref(spec),
                                                        None if filter is None else ctypes.byref(filter), ctypes.c_void_p(y.data_ptr()),
                                                        ctypes.byref(paste), arr, nv12[0], len(arr), mats.ctypes.data, flags.ctypes.data,
                                                        samples.ctypes.data))
            return (mats, flags) if filter is None else (mats, flags, samples)
        if filter is None:
            check(self._lib.sdm_align_paste_tensor(self._h, idx.ctypes.data, t.ctypes.data, idx.size, width, height, ctypes.byref(spec),
                                                   ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, len(arr), mats.ctypes.data,
                                                   flags.ctypes.data))
            return mats, flags
        samples = np.empty(n, np.int32)
        check(self._lib.sdm_align_paste_tensor_filtered(self._h, idx.ctypes.data, t.ctypes.data, idx.size, width, height, ctypes.byref(spec),
                                                        ctypes.byref(filter), ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr,
                                                        len(arr), mats.ctypes.data, flags.ctypes.data, samples.ctypes.data))
        return mats, flags, samples

    def align_paste_tensor_at(self, matrices, y, frames, formats=None, image_index=None, layout="nchw", mask=None, spec=None, filter=None,
                              max_samples=16, min_scale=1.0, chroma=None, **options):
        """``align_paste_tensor`` with explicit crop -> frame matrices (sdm_align_paste_tensor_at): ``matrices`` N x 2 x 3 as an earlier
        crop call returned them -- the tracker may have stepped on since; no landmark state, geometry or context image is needed.
        ``image_index``: the frame of every row (None: row i -> frame i).  Returns flags N int32: SDM_ALIGN_* bits; with a ``filter``
        (as for ``align_paste_tensor``: sdm_align_paste_tensor_at_filtered) it returns (flags, samples N int32: S of every row).  "nv12"
        destinations and ``chroma``: as for ``align_paste_tensor`` (sdm_align_paste_tensor_at_nv12)."""
        filter = self._paste_filter(filter, max_samples, min_scale)
        spec, paste, arr, n, width, height, keep, planes = self._paste_call(y, layout, frames, formats, mask, spec, options)
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 6)
        if m.shape[0] != n:
            raise ValueError(f"one matrix per row of the tensor expected: {m.shape[0]} for {n}")
        idx = self._paste_image_index(image_index, n)
        flags = np.empty(n, np.int32)
        nv12 = self._paste_chroma(chroma, arr, keep, planes)
        if nv12 is not None:
            samples = np.empty(n, np.int32)
            check(self._lib.sdm_align_paste_tensor_at_nv12(self._h, m.ctypes.data, None if idx is None else idx.ctypes.data, n, width, height,
                                                           ctypes.byref(spec), None if filter is None else ctypes.byref(filter),
                                                           ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, nv12[0], len(arr),
                                                           flags.ctypes.data, samples.ctypes.data))
            return flags if filter is None else (flags, samples)
        if filter is None:
            check(self._lib.sdm_align_paste_tensor_at(self._h, m.ctypes.data, None if idx is None else idx.ctypes.data, n, width, height,
                                                      ctypes.byref(spec), ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, len(arr),
                                                      flags.ctypes.data))
            return flags
        samples = np.empty(n, np.int32)
        check(self._lib.sdm_align_paste_tensor_at_filtered(self._h, m.ctypes.data, None if idx is None else idx.ctypes.data, n, width, height,
                                                           ctypes.byref(spec), ctypes.byref(filter), ctypes.c_void_p(y.data_ptr()),
                                                           ctypes.byref(paste), arr, len(arr), flags.ctypes.data, samples.ctypes.data))
        return flags, samples

    # -- landmark region masks (csrc/sdm_region_mask.hip) ----------------------------------------------
    def _region_out(self, n, width, height, out):
        """The N x height x width uint8 device tensor of a region mask call: ``out`` checked, or a new one.  torch's stream is
        synchronised: the library runs on its own."""
        import torch
        shape = (int(n), int(height), int(width))
        if out is None:
            if n < 1 or not (1 <= width <= 1024 and 1 <= height <= 1024):            # (the library refuses the call; nothing to allocate)
                out = torch.empty(16, dtype=torch.uint8, device=f"cuda:{self.device}")
            else:
                out = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous uint8 device tensor of shape {shape}")
        torch.cuda.current_stream(out.device).synchronize()
        return out

    @staticmethod
    def _region_polygons(polygons, holes, hull, grow, feather):
        """(the ``sdm_region_mask``, what keeps it alive, the P vertex entries in order) of ``polygons`` followed by ``holes`` -- each a
        sequence of vertex entries --; ``hull``: positions in that joined list"""
        polys = [list(p) for p in polygons] + [list(p) for p in holes]
        region, keep = _lib.region_mask([len(p) for p in polys], len(list(holes)), hull, grow, feather)
        return region, keep, [v for p in polys for v in p]

    def align_region_mask(self, landmark_index, template: np.ndarray, width: int, height: int, polygons, holes=(), hull=(), grow=0.0,
                          feather=0.0, out=None):
        """One crop-space opacity map per current row from its landmarks (include/sdm.h, sdm_align_region_mask): the fit of
        ``align_crops_tensor`` on ``landmark_index`` / ``template``, then the union of ``polygons`` minus ``holes`` -- each a sequence of
        landmark indices in order, 3 to 128 of them, at most 8 polygons and 256 indices in all; ``hull``: the positions (in
        ``polygons`` followed by ``holes``) of the polygons that are the convex hull of their landmarks -- moved outwards by ``grow``
        pixels with a linear ramp ``feather`` pixels wide (0: a one-pixel antialiased edge).  ``out``: a contiguous uint8 device
        tensor N x height x width, written in place; default: a new one.  Returns (maps, matrices N x 2 x 3 float32 crop -> source,
        flags N int32: SDM_ALIGN_* bits and SDM_REGION_NONFINITE) -- the maps are what ``mask=`` of ``align_paste_tensor`` takes."""
        idx = np.ascontiguousarray(landmark_index, np.int32).reshape(-1)
        t = np.ascontiguousarray(template, np.float32).reshape(-1, 2)
        if t.shape[0] != idx.size:
            raise ValueError("one template point (x, y) per landmark index expected")
        region, keep, verts = self._region_polygons(polygons, holes, hull, grow, feather)
        vidx = np.ascontiguousarray(verts, np.int32).reshape(-1)
        n = int(getattr(self, "N", 0))
        out = self._region_out(n, width, height, out)
        mats = np.empty((n, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        check(self._lib.sdm_align_region_mask(self._h, idx.ctypes.data, t.ctypes.data, idx.size, int(width), int(height), vidx.ctypes.data,
                                              ctypes.byref(region), ctypes.c_void_p(out.data_ptr()), mats.ctypes.data, flags.ctypes.data))
        return out, mats, flags

    def align_region_mask_at(self, matrices, points, width: int, height: int, sizes, n_holes=0, hull=(), grow=0.0, feather=0.0, out=None):
        """``align_region_mask`` for rows that are no longer current (sdm_align_region_mask_at): ``matrices`` N x 2 x 3 as an earlier crop
        call returned them, ``points`` N x P x 2 float32 frame positions of the polygons' vertices, one polygon after the other;
        ``sizes``: the vertex count of every polygon, the ``n_holes`` holes last; ``hull``: positions in ``sizes``.  No landmark state,
        geometry or image is needed.  Returns (maps N x height x width uint8 on the device, flags N int32)."""
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 6)
        region, keep = _lib.region_mask(sizes, n_holes, hull, grow, feather)
        p = np.ascontiguousarray(points, np.float32)
        P = sum(int(v) for v in sizes)
        if p.ndim != 3 or p.shape != (m.shape[0], P, 2):
            raise ValueError(f"points must be {m.shape[0]} x {P} x 2, one (x, y) per vertex of every row")
        n = m.shape[0]
        out = self._region_out(n, width, height, out)
        flags = np.empty(n, np.int32)
        check(self._lib.sdm_align_region_mask_at(self._h, m.ctypes.data, p.ctypes.data, n, int(width), int(height), ctypes.byref(region),
                                                 ctypes.c_void_p(out.data_ptr()), flags.ctypes.data))
        return out, flags

    # -- warped face tensors pasted back into frames (csrc/sdm_warp_paste.hip) -------------------------
    def _warp_paste_size(self, width, height):
        T, w, h = getattr(self, "warp_mesh", (0, 0, 0))
        if T and (w, h) != (width, height):
            raise ValueError(f"the tensor's crop is {width} x {height}, the mesh's {w} x {h}")
        return T

    def _warp_paste_chroma(self, chroma, arr, keep, planes=None):
        """the filtered calls take a mixed list: their UV planes, all None (behind the Y plane, read for NV12 frames only) by default"""
        return self._paste_chroma(chroma, arr, keep, planes) or (None, keep)

    def warp_paste_tensor(self, y, frames, formats=None, layout="nchw", mask=None, spec=None, chroma=None, filter=None, max_samples=16,
                          min_scale=1.0, **options):
        """The inverse of ``warp_crops_tensor`` for the N current rows (include/sdm.h, sdm_warp_paste_tensor): ``y`` -- a network's output
        in template space, a device tensor of the mesh's crop size -- is warped back under every row's own shape, triangle by triangle,
        and blended into ``frames`` IN PLACE.  ``frames``, ``formats``, ``layout``, ``mask``, ``spec`` / ``options``: as for
        ``align_paste_tensor``.  Returns (matrices N x T x 2 x 3 float32 crop -> frame, as ``warp_crops_tensor`` returns them, flags N
        int32: SDM_WARP_* bits).  With an "nv12" destination among ``frames``, or ``chroma`` given (as for ``align_paste_tensor``), the
        call is sdm_warp_paste_tensor_nv12: luma and 4:2:0 chroma blended in place; the return values are the same.  ``filter``: None
        (plain bilinear), or "area" / "bilinear" with ``max_samples`` and ``min_scale`` (``_lib.align_filter``) or an ``SdmAlignFilter``
        for sdm_warp_paste_tensor_filtered -- a frame pixel whose triangle's inverse map minifies averages Sx x Sy sub-samples, the
        destinations may mix NV12 and the other formats -- which returns (matrices, flags, samples N x T x 2 int32: (Sx, Sy) of every
        triangle)."""
        filter = self._paste_filter(filter, max_samples, min_scale)
        spec, paste, arr, n, width, height, keep, planes = self._paste_call(y, layout, frames, formats, mask, spec, options)
        T = self._warp_paste_size(width, height)
        self._paste_rows(n)
        mats = np.empty((n, T, 2, 3), np.float32)
        flags = np.empty(n, np.int32)
        if filter is not None:
            uv, keep = self._warp_paste_chroma(chroma, arr, keep, planes)
            samples = np.empty((n, T, 2), np.int32)
            check(self._lib.sdm_warp_paste_tensor_filtered(self._h, ctypes.byref(spec), ctypes.byref(filter), ctypes.c_void_p(y.data_ptr()),
                                                           ctypes.byref(paste), arr, uv, len(arr), mats.ctypes.data, flags.ctypes.data,
                                                           samples.ctypes.data))
            return mats, flags, samples
        nv12 = self._paste_chroma(chroma, arr, keep, planes)
        if nv12 is not None:
            check(self._lib.sdm_warp_paste_tensor_nv12(self._h, ctypes.byref(spec), ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr,
                                                       nv12[0], len(arr), mats.ctypes.data, flags.ctypes.data))
            return mats, flags
        check(self._lib.sdm_warp_paste_tensor(self._h, ctypes.byref(spec), ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, len(arr),
                                              mats.ctypes.data, flags.ctypes.data))
        return mats, flags

    def warp_paste_tensor_at(self, points, y, frames, formats=None, image_index=None, layout="nchw", mask=None, spec=None, chroma=None,
                             filter=None, max_samples=16, min_scale=1.0, **options):
        """``warp_paste_tensor`` with explicit landmarks (sdm_warp_paste_tensor_at): ``points`` N x K x 2 float32, (x, y) of the mesh's
        k-th landmark in its row's frame -- the tracker may have stepped on since; the mesh is needed, but no landmark state and no
        context image.  ``image_index``: the frame of every row (None: row i -> frame i).  Returns flags N int32: SDM_WARP_* bits.
        "nv12" destinations and ``chroma``: as for ``warp_paste_tensor`` (sdm_warp_paste_tensor_at_nv12).  With a ``filter`` (as for
        ``warp_paste_tensor``: sdm_warp_paste_tensor_at_filtered) it returns (flags, samples N x T x 2 int32)."""
        filter = self._paste_filter(filter, max_samples, min_scale)
        spec, paste, arr, n, width, height, keep, planes = self._paste_call(y, layout, frames, formats, mask, spec, options)
        T = self._warp_paste_size(width, height)
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 3 or p.shape[0] != n or p.shape[2] != 2:
            raise ValueError(f"points must be N x K x 2 with one row per row of the tensor ({n}), not {p.shape}")
        idx = self._paste_image_index(image_index, n)
        flags = np.empty(n, np.int32)
        if filter is not None:
            uv, keep = self._warp_paste_chroma(chroma, arr, keep, planes)
            samples = np.empty((n, T, 2), np.int32)
            check(self._lib.sdm_warp_paste_tensor_at_filtered(self._h, p.ctypes.data, None if idx is None else idx.ctypes.data, n,
                                                              ctypes.byref(spec), ctypes.byref(filter), ctypes.c_void_p(y.data_ptr()),
                                                              ctypes.byref(paste), arr, uv, len(arr), flags.ctypes.data, samples.ctypes.data))
            return flags, samples
        nv12 = self._paste_chroma(chroma, arr, keep, planes)
        if nv12 is not None:
            check(self._lib.sdm_warp_paste_tensor_at_nv12(self._h, p.ctypes.data, None if idx is None else idx.ctypes.data, n, ctypes.byref(spec),
                                                          ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, nv12[0], len(arr),
                                                          flags.ctypes.data))
            return flags
        check(self._lib.sdm_warp_paste_tensor_at(self._h, p.ctypes.data, None if idx is None else idx.ctypes.data, n, ctypes.byref(spec),
                                                 ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, len(arr), flags.ctypes.data))
        return flags

    # -- misc ------------------------------------------------------------------------------------------
    def synchronize(self):
        check(self._lib.sdm_synchronize(self._h))

    def enable_timing(self, on: bool = True):
        check(self._lib.sdm_enable_timing(self._h, int(on)))

    def get_timing(self, reset: bool = False):
        ms = (ctypes.c_float * _lib.SDM_T_COUNT)()
        n = (ctypes.c_int * _lib.SDM_T_COUNT)()
        check(self._lib.sdm_get_timing(self._h, ms, n, int(reset)))
        return {_lib.TIMING_NAMES[i]: (float(ms[i]), int(n[i])) for i in range(_lib.SDM_T_COUNT - 1)}

    def gram_device_ptr(self):
        p, c = ctypes.c_void_p(), ctypes.c_size_t()
        check(self._lib.sdm_gram_device_ptr(self._h, ctypes.byref(p), ctypes.byref(c)))
        return p.value, c.value

    def features_device_ptr(self):
        """(device pointer, row stride in floats, rows) of the feature matrix of the last sdm_hog_features call."""
        p, ld, n = ctypes.c_void_p(), ctypes.c_longlong(), ctypes.c_int()
        check(self._lib.sdm_features_device_ptr(self._h, ctypes.byref(p), ctypes.byref(ld), ctypes.byref(n)))
        return p.value, ld.value, n.value

    def x_device_ptr(self):
        p, c = ctypes.c_void_p(), ctypes.c_size_t()
        check(self._lib.sdm_x_device_ptr(self._h, ctypes.byref(p), ctypes.byref(c)))
        return p.value, c.value

    def debug_patch(self, level: int, sample: int, landmark: int, hp: HoGParam):
        S, C, O = hp.num_cells * hp.cell_size, hp.num_cells, hp.num_bins
        rsz = np.empty((S, S), np.uint8)
        bins = np.empty((S, S), np.uint8)
        hist = np.empty((2 * O, C, C), np.float32)
        desc = np.empty(hp.patch_dim, np.float32)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        check(self._lib.sdm_debug_patch(self._h, level, sample, landmark, rsz.ctypes.data_as(u8),
                                        bins.ctypes.data_as(u8), _fp(hist), _fp(desc)))
        return rsz, bins, hist, desc

    def debug_update_f16(self, P: np.ndarray, C: np.ndarray, wcols_factor: int, factor_bound: float) -> np.ndarray:
        """C - P^T P on the float16 matrix cores (the Cholesky's trailing update by itself; sdm_debug_update_f16)."""
        P = np.ascontiguousarray(P, np.float32)
        out = np.ascontiguousarray(C, np.float32).copy()
        check(self._lib.sdm_debug_update_f16(self._h, _fp(P), P.shape[0], P.shape[1], int(wcols_factor), float(factor_bound), _fp(out)))
        return out

    def debug_hog_profile(self, level: int):
        out = (ctypes.c_ulonglong * 8)()
        check(self._lib.sdm_debug_hog_profile(self._h, level, out))
        n = max(int(out[7]), 1)
        names = ["setup", "clear", "rows", "barrier", "normalise", "store"]
        return {names[i]: out[i] / n for i in range(6)}, n

    def debug_hog_taps(self, level: int):
        """The level's cv::resize taps table as the device built it, [128 half-widths][64 coordinates][8], and
        {cells_launch, one_load_instance, two_load_option} (include/sdm.h: sdm_debug_hog_taps)."""
        table = np.empty((128, 64, 8), np.int32)
        info = np.zeros(3, np.int32)
        check(self._lib.sdm_debug_hog_taps(self._h, level, _ip(table), _ip(info)))
        return table, dict(cells_launch=bool(info[0]), one_load_instance=bool(info[1]), two_load_option=bool(info[2]))

    def debug_hog_pair_taps(self, level: int):
        """The level's pair-loop table as the device built it, [128 half-widths][64][4] = {take-the-spare mask of row d, spare source
        row of pixel rows (2d + 1, 2d + 2) or -1, pair eligible, orphan rows}, and {pair_instance, two_load_option}
        (include/sdm.h: sdm_debug_hog_pair_taps)."""
        table = np.empty((128, 64, 4), np.int32)
        info = np.zeros(2, np.int32)
        check(self._lib.sdm_debug_hog_pair_taps(self._h, level, _ip(table), _ip(info)))
        return table, dict(pair_instance=bool(info[0]), two_load_option=bool(info[1]))

    def set_hog_packing(self, on: bool):
        """Lane packing of the HOG launch (include/sdm.h: sdm_debug_set_hog_packing); on by default."""
        check(self._lib.sdm_debug_set_hog_packing(self._h, int(on)))

    def set_detect_path(self, fused: bool = True, split_store: bool = False):
        """Round-4 A/B switch (``sdm_debug_set_detect_path``): ``fused`` -- ``detect_batch`` multiplies the descriptors by the
        regressor on the chip and never writes the feature matrix (default for 2L <= 64; ``fused="wide"`` also for wider outputs); ``split_store`` -- feature rows through the raw cell
        histograms + the store form of csrc/sdm_desc.hip instead of the pixel kernel's own normalisation (default off)."""
        check(self._lib.sdm_debug_set_detect_path(self._h, 2 if fused == "wide" else int(bool(fused)), int(bool(split_store))))

    def gram_fallbacks(self) -> int:
        """Gram launches of this context repeated with three bf16 pieces (an operand beyond float16's range); tests."""
        return check(self._lib.sdm_debug_gram_fallbacks(self._h))

    def update_fallbacks(self) -> int:
        """Factorisations that ran their trailing updates in f32 because the Gram diagonal spanned more than 2^20."""
        return check(self._lib.sdm_debug_update_fallbacks(self._h))

    def debug_gradient_table(self, level: int):
        g = np.empty((511, 511), np.float32)
        b = np.empty((511, 511), np.int32)
        check(self._lib.sdm_debug_gradient_table(self._h, level, _fp(g), _ip(b)))
        return g, b


def hog_plan(num_cells: int, cell_size: int, num_bins: int, num_landmarks: int, max_passes: int = 64):
    """The lane-packing plan of a level geometry (host only; csrc/sdm_kernels.h: HogPlanDev).  Returns None when the
    geometry has no packed kernel instance, else a dict with G, P, n_main, Gt, Pt and the three tables."""
    L = _lib.lib()
    info = np.zeros(5, np.int32)
    lane_tab = np.zeros((max_passes, 64), np.uint32)
    wb = np.zeros((max_passes, 64, 16), np.float32)
    pass_info = np.zeros((max_passes, 4), np.int32)
    check(L.sdm_debug_hog_plan(num_cells, cell_size, num_bins, num_landmarks, _ip(info), lane_tab.ctypes.data,
                               wb.ctypes.data, pass_info.ctypes.data, max_passes))
    if info[0] == 0:
        return None
    n = int(info[1] + info[4])
    cut = np.zeros(num_landmarks, np.int32)
    check(L.sdm_debug_hog_plan_cut(num_cells, cell_size, num_bins, num_landmarks, _ip(cut)))
    cols = np.zeros((num_landmarks, 3), np.int32)      # {cut, jA, jB}: the cell columns part 0 (0 .. jA) and part 1 (jB ..) hold
    check(L.sdm_debug_hog_plan_columns(num_cells, cell_size, num_bins, num_landmarks, _ip(cols)))
    return {"G": int(info[0]), "P": int(info[1]), "n_main": int(info[2]), "Gt": int(info[3]), "Pt": int(info[4]),
            "lane_tab": lane_tab[:n], "wb": wb[:n], "pass_info": pass_info[:n], "cut": cut, "columns": cols}


def hog_band_weights(cell_size: int, num_cells: int):
    """The band-slot weights {slot 0, slot 1} of the resized-ROI rows of a level geometry, [num_cells * cell_size][2] float32, as the
    pixel kernel's detect instances hold them (host only; include/sdm.h: sdm_debug_hog_band_weights)."""
    out = np.zeros((64, 2), np.float32)
    check(_lib.lib().sdm_debug_hog_band_weights(cell_size, num_cells, _fp(out)))
    return out[:num_cells * cell_size]


# --------------------------------------------------------------------------------------------------
# Reference-shaped operator surface
# --------------------------------------------------------------------------------------------------

class Regulariser:
    """regressors.hpp:87-169."""

    class RegularisationType:
        Manual = 0
        MatrixNorm = 1

    def __init__(self, regularisation_type: int = 0, param: float = 0.0, regularise_last_row: bool = True):
        self.regularisation_type = regularisation_type
        self.param = float(param)
        self.regularise_last_row = bool(regularise_last_row)


class RegulariserSweep(Regulariser):
    """K candidates of ``Regulariser``'s one parameter, chosen per level by the error on held-out rows
    (``SupervisedDescentOptimiser.train(..., holdout=h)``; include/sdm.h: sdm_train_level_sweep).  Usable wherever a
    ``Regulariser`` is: after training ``param`` is the winner's, so the object then reads as the plain regulariser that was
    picked."""

    def __init__(self, regularisation_type: int = 0, params: Sequence[float] = (0.0,), regularise_last_row: bool = True):
        params = [float(p) for p in np.atleast_1d(np.asarray(params, np.float64)).reshape(-1)]
        if not 1 <= len(params) <= 32:
            raise ValueError("a RegulariserSweep holds 1 ... 32 candidate parameters")
        super().__init__(regularisation_type, params[0], regularise_last_row)
        self.params = params


class _ResidentToken:
    """What a Context's device copy of one level holds: THE array object (a strong reference, so its id cannot be reused by
    another array) and the regressor's version when it was uploaded."""

    __slots__ = ("array", "version")

    def __init__(self, array, version):
        self.array, self.version = array, version


class PartialPivLUSolver:
    """regressors.hpp:181-234: the default solver of LinearRegressor.  On the device the regularised normal matrix -- symmetric
    positive definite -- is factored by a blocked Cholesky (csrc/sdm_solve.hip)."""
    kind = 0


class ColPivHouseholderQRSolver:
    """regressors.hpp:242-306: Householder QR with column pivoting of AtA + reg, on the device (csrc/sdm_qr.hip).  Like the
    reference it reports a system that is not invertible (``rank``, ``is_invertible`` after a solve; the warning text is the
    reference's) and is much slower than the default."""
    kind = 1

    def __init__(self):
        self.rank: Optional[int] = None
        self.full_rank: Optional[int] = None

    @property
    def is_invertible(self) -> Optional[bool]:
        return None if self.rank is None else self.rank == self.full_rank

    def _report(self, ctx):
        self.rank, self.full_rank = ctx.last_rank()
        if self.rank != self.full_rank:      # regressors.hpp:289-292
            print("The regularised AtA is not invertible. We continued learning, but Eigen may return garbage (their docu is not "
                  "very specific). (The rank is %d, full rank would be %d). Increase lambda." % (self.rank, self.full_rank))


class LinearRegressor:
    """regressors.hpp:318-400.  ``x`` is the learned F x M matrix (public, as in the reference); ``solver`` the reference's
    template parameter (PartialPivLUSolver by default, or ColPivHouseholderQRSolver).

    The optimiser keeps an unchanged regressor resident on the device between calls.  "Unchanged" is enforced, not assumed:
    while a device copy of ``x`` exists the array is read-only, so ``reg.x[...] = v`` or ``reg.x *= s`` raise instead of
    silently leaving the device with stale coefficients.  Assign a new array (``reg.x = ...``), or call ``touch()`` and then
    edit in place: both make the next ``test``/``predict``/``detect`` upload the level again."""

    def __init__(self, regulariser: Optional[Regulariser] = None, solver=None):
        self.solver = solver or PartialPivLUSolver()
        self._x: Optional[np.ndarray] = None
        self._version = 0
        self._frozen = None          # (array, its original writeable flag) while a device copy exists
        self.regulariser = regulariser or Regulariser()
        self.last_lambda: Optional[float] = None
        self.sweep: Optional[dict] = None       # the record of train(..., holdout=h): Context.train_level_sweep's dict

    @property
    def x(self) -> Optional[np.ndarray]:
        return self._x

    @x.setter
    def x(self, value):
        self._thaw()
        self._x = value
        self._version += 1

    def touch(self):
        """Declares ``x`` about to be modified in place: writable again, and uploaded again at the next use."""
        self._thaw()
        self._version += 1

    def _freeze(self):
        a = self._x
        if isinstance(a, np.ndarray) and self._frozen is None:
            self._frozen = (a, bool(a.flags.writeable))
            a.flags.writeable = False

    def _thaw(self):
        if self._frozen is not None:
            a, was = self._frozen
            self._frozen = None
            if was:
                try:
                    a.flags.writeable = True
                except ValueError:      # (a view of a read-only base)
                    pass


class InterEyeDistanceNormalisation:
    """model.hpp:84-116 (string ids resolved to positions once instead of per call)."""

    def __init__(self, model_landmarks: Sequence[str], right_eye_ids: Sequence[str], left_eye_ids: Sequence[str]):
        ids = list(model_landmarks)
        try:
            self.right_eye = [ids.index(i) for i in right_eye_ids]
            self.left_eye = [ids.index(i) for i in left_eye_ids]
        except ValueError as e:  # helpers.hpp:143-145, 152-154
            raise RuntimeError("one of given eye identifiers not present in lms") from e
        self.model_landmarks = ids


class HogTransform:
    """rcr::HogTransform (adaptive_vlhog.hpp:70-195): holds the images and per-level HoG parameters.

    ``images`` is a list / stack of single-channel uint8 images (or device-resident frames, see
    ``Context.set_frames_device``); ``img_index`` maps a sample row to its
    image (the reference's ``training_index``; perturbed copies share an image)."""

    def __init__(self, images, hog_params: Sequence[HoGParam], model_landmarks: Sequence[str],
                 right_eye_ids: Sequence[str], left_eye_ids: Sequence[str],
                 img_index: Optional[np.ndarray] = None, images_resident: bool = False, formats=None, chroma=None):
        self.images = images
        self.formats, self.chroma = formats, chroma    # device frames: as Context.set_frames_device takes them (planar names)
        self.images_resident = bool(images_resident)   # opt-in: the pixels do not change between calls with THIS object
        self.hog_params = list(hog_params)
        self.model_landmarks = list(model_landmarks)
        self.norm = InterEyeDistanceNormalisation(model_landmarks, right_eye_ids, left_eye_ids)
        self.img_index = img_index


def _mat4_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Batched 4 x 4 product (..., 4, 4) in float32, every entry summed k = 0..3 in order (the device kernel's order)."""
    c = np.empty(np.broadcast_shapes(a.shape, b.shape), np.float32)
    for i in range(4):
        for j in range(4):
            c[..., i, j] = a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j] + a[..., i, 2] * b[..., 2, j] + a[..., i, 3] * b[..., 3, j]
    return c


class ModelProjection:
    """The ModelProjection function object of the reference's examples/pose_estimation.cpp:187-240: projects a 3D model with the
    6-DOF parameters x = [r_x, r_y, r_z, t_x, t_y, t_z] (degrees) through a pinhole camera and returns the normalised 2D points
    [u_0..u_{K-1}, v_0..v_{K-1}].

    ``model``: 4 x K homogeneous points as in the example (:257-267), or 3 x K.  The camera defaults are the example's (focal
    1800, a 1000 x 1000 screen, near 1, far 5000); u and v do not depend on them (the field of view is derived from the focal
    length, :46), which is why landmarks in any image can be normalised by their own image centre (``estimate_pose``).
    Passed to :class:`SupervisedDescentOptimiser` the cascade runs on the device (csrc/sdm_pose.hip); ``__call__`` is the host
    evaluation (float32) users synthesise training data with (:305-309)."""

    def __init__(self, model, focal: float = 1800.0, width: float = 1000.0, height: float = 1000.0, near: float = 1.0,
                 far: float = 5000.0):
        m = np.asarray(model, np.float32)
        if m.ndim != 2 or m.shape[0] not in (3, 4) or not 1 <= m.shape[1] <= 64:
            raise ValueError("the model must be 4 x K (homogeneous) or 3 x K, 1 <= K <= 64")
        self.points = np.ascontiguousarray(m[:3].T)                      # K x 3
        self.focal, self.width, self.height, self.near, self.far = (float(v) for v in (focal, width, height, near, far))

    @property
    def K(self) -> int:
        return self.points.shape[0]

    def projection_matrix(self) -> np.ndarray:
        """createPerspectiveProjectionMatrix (:142-154) with fovy = focalLengthToFovy (:46), in float32."""
        f32 = np.float32
        fovy = (f32(2.0) * np.arctan2(f32(self.height), f32(2.0) * f32(self.focal))) * f32(180 / np.pi)
        rad = (fovy / f32(2.0)) * f32(np.pi) / f32(180.0)
        cotan = np.cos(rad) / np.sin(rad)
        aspect = f32(self.width) / f32(self.height)
        n, fa = f32(self.near), f32(self.far)
        P = np.zeros((4, 4), np.float32)
        P[0, 0], P[1, 1] = cotan / aspect, cotan
        P[2, 2], P[2, 3] = -(n + fa) / (fa - n), (f32(-2.0) * n * fa) / (fa - n)
        P[3, 2] = -1.0
        return P

    def __call__(self, parameters, regressor_level: int = 0, training_index: int = 0) -> np.ndarray:
        """1 x 6 (or N x 6) parameters -> 1 x 2K (N x 2K) normalised projections.  regressor_level / training_index are not
        used, as in the example."""
        x = np.atleast_2d(np.asarray(parameters, np.float32))
        if x.shape[1] != 6:
            raise ValueError("parameters must be rows [r_x, r_y, r_z, t_x, t_y, t_z]")
        f32, n = np.float32, x.shape[0]
        d2r = f32(np.pi / 180)
        c, s = np.cos(x[:, :3] * d2r), np.sin(x[:, :3] * d2r)
        one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
        mk = lambda *rows: np.stack([np.stack(r, -1) for r in rows], -2)   # noqa: E731
        T = mk((one, zero, zero, x[:, 3]), (zero, one, zero, x[:, 4]), (zero, zero, one, x[:, 5]), (zero, zero, zero, one))
        Ry = mk((c[:, 1], zero, s[:, 1], zero), (zero, one, zero, zero), (-s[:, 1], zero, c[:, 1], zero), (zero, zero, zero, one))
        Rx = mk((one, zero, zero, zero), (zero, c[:, 0], -s[:, 0], zero), (zero, s[:, 0], c[:, 0], zero), (zero, zero, zero, one))
        Rz = mk((c[:, 2], -s[:, 2], zero, zero), (s[:, 2], c[:, 2], zero, zero), (zero, zero, one, zero), (zero, zero, zero, one))
        mvp = _mat4_mul(self.projection_matrix()[None], _mat4_mul(_mat4_mul(_mat4_mul(T, Ry), Rx), Rz))
        X, Y, Z = (self.points[:, k][None, :] for k in range(3))
        clip = [mvp[:, r, 0:1] * X + mvp[:, r, 1:2] * Y + mvp[:, r, 2:3] * Z + mvp[:, r, 3:4] for r in (0, 1, 3)]
        nx, ny = clip[0] / clip[2], clip[1] / clip[2]
        hw, hh = f32(self.width) / f32(2.0), f32(self.height) / f32(2.0)
        x_ss = (nx + f32(1.0)) * hw
        y_ss = f32(self.height) - (ny + f32(1.0)) * hh
        u, v = (x_ss - hw) / f32(self.focal), (y_ss - hh) / f32(self.focal)
        return np.concatenate([u, v], axis=1).astype(np.float32)


class SupervisedDescentOptimiser:
    """superviseddescent.hpp:85-361 for RegressorType = LinearRegressor and ProjectionFunction =
    HogTransform: the per-level work runs as batched HIP kernels.

    ``allreduce`` (optional) is ``fn(dev_ptr, count_f32, hip_stream)``; with it ``train`` is the
    data-parallel variant: every rank holds a shard of the rows, {A^T A, A^T b} are summed over ranks
    once per level and every rank solves the identical system (see parallel.py)."""

    def __init__(self, regressors: List[LinearRegressor], normalisation: Optional[InterEyeDistanceNormalisation] = None,
                 device: int = 0, stream: Optional[int] = None, ctx=None):
        self.regressors = regressors
        self.normalisation = normalisation
        # ``ctx``: an object with Context's methods; the CPU tests of the data-parallel logic inject one built on
        # the oracle, the product path always builds the HIP context here
        self.ctx = ctx if ctx is not None else Context(device, stream)
        self._bound = None

    def _bind(self, projection: HogTransform, n_rows: int):
        if not isinstance(projection, HogTransform):
            raise TypeError("the HIP engine accelerates HogTransform projections; generic projection "
                            "functors are served by the C++ header layer (superviseddescent.hpp)")
        if len(projection.hog_params) != len(self.regressors):
            raise ValueError("one HoGParam per regressor level expected")  # rcr-train.cpp:448
        if projection.img_index is not None and len(projection.img_index) != n_rows:
            raise ValueError("HogTransform.img_index must hold one image number per sample row")
        norm = self.normalisation or projection.norm
        # (a no-op on the device when the geometry has not changed: regressors and buffers stay resident)
        self.ctx.set_model_geometry(len(projection.model_landmarks), norm.right_eye, norm.left_eye,
                                    projection.hog_params)
        # The reference's HogTransform reads the CURRENT pixels of its images at every call, so the images are uploaded at
        # every bind -- unless the caller declares them resident (HogTransform(..., images_resident=True)) and passes the
        # very same projection object again, which this optimiser then holds a strong reference to.
        if not (projection.images_resident and self._bound is projection):
            if _device_frames(projection.images):
                named = {k: v for k in ("formats", "chroma") for v in [getattr(projection, k, None)] if v is not None}
                self.ctx.set_frames_device(projection.images, **named)
            else:
                self.ctx.upload_images(projection.images)
        self._bound = projection
        self.ctx.set_sample_image_index(projection.img_index)

    def train(self, parameters, initialisations, templates, projection: HogTransform,
              on_training_epoch_callback: Optional[Callable[[np.ndarray], None]] = None,
              allreduce=None, world_size: int = 1, n_train_global: int = 0, rank: Optional[int] = None,
              solve_collectives=None, reduce_scatter=None, rccl=None, rccl_shard_solve: bool = False, holdout: int = 0):
        """``holdout = h`` holds the LAST ``h`` rows out of every level's fit: a level whose regressor carries a ``RegulariserSweep``
        tries all its candidates on one Gram product and keeps the one with the lowest mean normalised error on those rows
        (``reg.sweep`` records params, lambdas, holdout_errors, fit_errors, status, best); a level with a plain ``Regulariser`` is
        a sweep of one candidate, so the cascade sees one split.  Single device only (no collective arguments).

        ``rank`` + ``solve_collectives = (bcast, allgather)`` (parallel.make_torch_solve_collectives) additionally shard the
        factorisation of the summed system over the ranks (Context.set_solve_sharding); without them every rank solves it.
        ``reduce_scatter`` (parallel.make_torch_reduce_scatter) then replaces the all-reduce of the whole Gram matrix by a
        reduce-scatter of the owned tile columns + a small all-reduce (Context.set_reduce_scatter).
        ``rccl`` (a ``parallel.RcclCommunicator``) takes the place of all three callbacks: the library then issues the collectives
        itself through RCCL on its own streams (``rccl_shard_solve``: sharded factorisation + reduce-scatter exchange); the
        callbacks remain for backends without RCCL (the gloo tests)."""
        sweeping = any(isinstance(reg.regulariser, RegulariserSweep) for reg in self.regressors)
        collective = allreduce is not None or rccl is not None or solve_collectives is not None or reduce_scatter is not None
        holdout = int(holdout or 0)
        if holdout < 0:
            raise ValueError("holdout must be a row count >= 0")
        if sweeping and not holdout:
            raise ValueError("a RegulariserSweep needs held-out rows to choose by: train(..., holdout=h)")
        if (sweeping or holdout) and collective:
            raise ValueError("a regulariser sweep / holdout runs on one device: no collective arguments")
        if (sweeping or holdout) and isinstance(projection, ModelProjection):
            raise ValueError("the pose cascade has no regulariser sweep / holdout")
        if isinstance(projection, ModelProjection):
            if collective:
                raise ValueError("pose training runs on one device")
            return self._pose_train(parameters, initialisations, templates, projection, on_training_epoch_callback)
        x0 = np.asarray(initialisations, np.float32)
        if holdout and not 1 <= holdout < x0.shape[0]:
            raise ValueError("holdout must leave at least one row to fit and hold at least one out")
        self._bind(projection, x0.shape[0])
        c = self.ctx
        c.set_templates(templates)                                           # superviseddescent.hpp:195-197
        c.set_x(x0)
        c.set_targets(np.asarray(parameters, np.float32))
        if rccl is not None and (allreduce is not None or solve_collectives is not None or reduce_scatter is not None):
            raise ValueError("train: pass either the RCCL communicator or the collective callbacks, not both")
        n_glob = n_train_global or c.N
        try:
            # (inside the try: an install that fails half-way must not leave the communicator registered on a shared context)
            if rccl is not None:
                rccl.install(c, shard_solve=rccl_shard_solve, reduce_scatter=rccl_shard_solve)
            else:
                c.set_allreduce(allreduce, world_size)
                if hasattr(c, "set_solve_sharding"):
                    if solve_collectives is not None and rank is not None:
                        c.set_solve_sharding(rank, world_size, *solve_collectives)
                    else:
                        c.set_solve_sharding(0, 0, None, None)
                if hasattr(c, "set_reduce_scatter"):
                    c.set_reduce_scatter(reduce_scatter if (solve_collectives is not None and rank is not None) else None)
            if holdout:
                return self._train_levels_holdout(c, x0.shape[0] - holdout, n_train_global, on_training_epoch_callback)
            return self._train_levels(c, n_glob, on_training_epoch_callback)
        finally:
            if hasattr(c, "set_solver"):
                c.set_solver(0)                                              # (the context may be shared: leave the default solver behind)
            if rccl is not None:
                rccl.uninstall(c)                                            # (the communicator belongs to the caller)

    def _train_levels(self, c, n_glob, on_training_epoch_callback):
        for level, reg in enumerate(self.regressors):
            kind = getattr(reg.solver, "kind", 0)
            if hasattr(c, "set_solver"):
                c.set_solver(kind)                                           # LinearRegressor<Solver>, regressors.hpp:318 (before the Gram launch: it picks the exchange form by the solver)
            c.hog_features(level)                                            # superviseddescent.hpp:173-189
            c.gram_rhs(level)                                                # :199-205 + regressors.hpp:208,225
            c.allreduce_gram_rhs()
            r = reg.regulariser
            reg.x, reg.last_lambda = c.solve(level, r.regularisation_type, r.param, r.regularise_last_row,
                                             n_glob)                         # :207
            if kind == 1 and hasattr(c, "last_rank"):
                reg.solver._report(c)
            self._mark_resident(level, reg)                                  # (sdm_solve left it on the device)
            c.apply(level)                                                   # :209-216
            if on_training_epoch_callback is not None:
                on_training_epoch_callback(c.get_x())                        # :217
        return c.get_x()

    def _train_levels_holdout(self, c, n_fit, n_train_global, on_training_epoch_callback):
        """Every level fits rows [0, n_fit) and is scored on the rows behind them (Context.train_level_sweep); the winner is
        installed and applied on the device, its coefficients fetched once."""
        for level, reg in enumerate(self.regressors):
            kind = getattr(reg.solver, "kind", 0)
            c.set_solver(kind)
            r = reg.regulariser
            params = r.params if isinstance(r, RegulariserSweep) else [r.param]
            rec = c.train_level_sweep(level, r.regularisation_type, params, r.regularise_last_row, n_fit, n_train_global)
            best = rec["best"]
            reg.x, reg.last_lambda = c.get_regressor(level), float(rec["lambdas"][best])
            if isinstance(r, RegulariserSweep):
                r.param = float(r.params[best])
            reg.sweep = rec
            if kind == 1 and hasattr(c, "last_rank"):
                reg.solver._report(c)
            self._mark_resident(level, reg)                                  # (the sweep installed the winner on the device)
            if on_training_epoch_callback is not None:
                on_training_epoch_callback(c.get_x())
        return c.get_x()

    def _mark_resident(self, level: int, reg: LinearRegressor):
        if hasattr(self.ctx, "set_resident_token") and isinstance(reg.x, np.ndarray):
            self.ctx.set_resident_token(level, _ResidentToken(reg.x, reg._version))
            reg._freeze()

    def _load_regressors(self):
        """Regressors the device already holds are not uploaded again: a per-frame ``detect()`` then costs the image upload
        and the kernels, not 4 x 1.5 MB of regressor traffic.  The record of what the device holds lives in the Context (any
        ``set_regressor`` / ``solve`` by anyone, or a changed geometry, replaces it), it names the array OBJECT (no id()
        reuse) and its version, and a resident array is read-only (in-place edits raise; see LinearRegressor)."""
        c = self.ctx
        for level, reg in enumerate(self.regressors):
            if reg.x is None:
                raise RuntimeError("regressor level %d has not been learned" % level)
            tok = c.resident_token(level) if hasattr(c, "resident_token") else None
            if isinstance(tok, _ResidentToken) and tok.array is reg.x and tok.version == reg._version:
                continue
            if hasattr(c, "resident_token"):
                x = reg.x if isinstance(reg.x, np.ndarray) else np.asarray(reg.x, np.float32)
                c.set_regressor(level, x, token=_ResidentToken(reg.x, reg._version) if isinstance(reg.x, np.ndarray) else None)
                reg._freeze()
            else:
                c.set_regressor(level, reg.x)

    def test(self, initialisations, templates, projection: HogTransform,
             on_regressor_iteration_callback: Optional[Callable[[np.ndarray], None]] = None) -> np.ndarray:
        if isinstance(projection, ModelProjection):
            return self._pose_test(initialisations, templates, projection, on_regressor_iteration_callback)
        x0 = np.atleast_2d(np.asarray(initialisations, np.float32))
        self._bind(projection, x0.shape[0])
        self._load_regressors()
        c = self.ctx
        c.set_templates(templates)                                           # superviseddescent.hpp:287-289
        c.set_x(x0)
        if on_regressor_iteration_callback is None:
            return c.detect_batch()                                           # :262-306
        for level in range(len(self.regressors)):
            c.detect_level(level)                                             # (the launches detect_batch runs: same bits)
            on_regressor_iteration_callback(c.get_x())                        # :303
        return c.get_x()

    def predict(self, initialisation, templates, projection: HogTransform) -> np.ndarray:
        if isinstance(projection, ModelProjection):
            return self.test(np.atleast_2d(initialisation), np.atleast_2d(templates), projection)
        return self.test(np.atleast_2d(initialisation), templates, projection)  # :323-344

    # -- ModelProjection (examples/pose_estimation.cpp): known-template SDM, NoNormalisation, on csrc/sdm_pose.hip ------------------
    def _pose_bind(self, projection: "ModelProjection", ctx=None):
        if self.normalisation is not None:
            raise TypeError("the pose cascade takes no normalisation (NoNormalisation, pose_estimation.cpp:285)")
        if not 1 <= len(self.regressors) <= 16:
            raise ValueError("the pose cascade runs 1 ... 16 regressor levels")
        c = ctx or self.ctx
        c.pose_set_model(projection.points, projection.focal, projection.width, projection.height, projection.near, projection.far)
        return c

    def _pose_train(self, parameters, initialisations, templates, projection, on_training_epoch_callback):
        if templates is None or np.size(templates) == 0:
            raise ValueError("the pose cascade is a known-template SDM: pass the observed landmarks as templates")
        c = self._pose_bind(projection)
        for reg in self.regressors:
            if getattr(reg.solver, "kind", 0) != 0:
                raise TypeError("the device pose path solves with PartialPivLUSolver (the LU family)")
        c.pose_set_x(np.asarray(initialisations, np.float32))
        c.pose_set_templates(np.asarray(templates, np.float32))
        c.pose_set_targets(np.asarray(parameters, np.float32))
        for level, reg in enumerate(self.regressors):
            r = reg.regulariser
            reg.x, reg.last_lambda = c.pose_train_level(level, r.regularisation_type, r.param, r.regularise_last_row)   # :170-216
            if on_training_epoch_callback is not None:
                on_training_epoch_callback(c.pose_get_x())                   # :217
        return c.pose_get_x()

    def _pose_upload(self, c):
        for level, reg in enumerate(self.regressors):
            if reg.x is None:
                raise RuntimeError("regressor level %d has not been learned" % level)
            c.pose_set_regressor(level, reg.x)

    def _pose_test(self, initialisations, templates, projection, on_regressor_iteration_callback=None):
        if templates is None or np.size(templates) == 0:
            raise ValueError("the pose cascade is a known-template SDM: pass the observed landmarks as templates")
        c = self._pose_bind(projection)
        self._pose_upload(c)
        c.pose_set_x(np.atleast_2d(np.asarray(initialisations, np.float32)))
        c.pose_set_templates(np.atleast_2d(np.asarray(templates, np.float32)))
        n = len(self.regressors)
        if on_regressor_iteration_callback is None:
            c.pose_test(0, n)                                                # all levels in one launch
        else:
            for level in range(n):
                c.pose_test(level, 1)                                        # (the same kernel per level: same bits)
                on_regressor_iteration_callback(c.pose_get_x())              # superviseddescent.hpp:303
        return c.pose_get_x()


class detection_model:
    """rcr::detection_model (model.hpp:122-183)."""

    def __init__(self, optimised_model: SupervisedDescentOptimiser, mean: np.ndarray, landmark_ids: Sequence[str],
                 hog_params: Sequence[HoGParam], right_eye_ids: Sequence[str], left_eye_ids: Sequence[str]):
        self.optimised_model = optimised_model
        self.mean = np.asarray(mean, np.float32).reshape(-1)
        self.landmark_ids = list(landmark_ids)
        self.hog_params = list(hog_params)
        self.right_eye_ids, self.left_eye_ids = list(right_eye_ids), list(left_eye_ids)

    def detect(self, image: np.ndarray, facebox=None, initialisation=None) -> np.ndarray:
        """model.hpp:132-157, both overloads: ``detect(image, facebox)`` with a face box (x, y, w, h) -- four numbers, 1-D --
        or ``detect(image, initialisation=row)`` with an initial landmark row (1 x 2L).  A 2-D second positional argument is
        taken as an initialisation, so a 2-landmark model (2L = 4) is not mistaken for a box."""
        from .synth import align_mean
        if (facebox is None) == (initialisation is None):
            raise ValueError("give either a face box or an initialisation")
        if facebox is not None:
            a = np.asarray(facebox)
            if a.ndim == 2:
                initialisation, facebox = a, None
            elif a.shape != (4,):
                raise ValueError("a face box is (x, y, width, height)")
        if facebox is not None:
            init = align_mean(self.mean, tuple(int(v) for v in np.asarray(facebox)))
        else:
            init = np.asarray(initialisation, np.float32).reshape(1, -1)
            if init.shape[1] != self.mean.size:
                raise ValueError("the initialisation must hold 2L coordinates")
        hog = HogTransform([image], self.hog_params, self.landmark_ids, self.right_eye_ids, self.left_eye_ids)
        return self.optimised_model.predict(np.atleast_2d(init), None, hog)[0]

    def detect_batch(self, images, faceboxes: np.ndarray, img_index: Optional[np.ndarray] = None, roll=None, chip: Optional[int] = None,
                     guard: Optional[int] = None, formats=None, chroma=None) -> np.ndarray:
        """Batched ``detect``: row i starts from align_mean(mean, faceboxes[i]) on image img_index[i].  ``images``: host images, or
        frames on the device as ``Context.set_frames_device`` takes them (gray, "bgr" / "bgra" tensors of any size and row stride;
        (ptr, w, h, stride, format) tuples for the other formats; with ``formats`` "bgr_planar" / "rgb_planar", 3 x H x W tensors or
        one n x 3 x H x W tensor, and ``chroma`` the second planes of planar tuples) -- those are not downloaded.
        ``roll`` (degrees, clockwise positive; one value or one per row) selects the upright path for rolled faces: every face is cut
        upright from its frame as a ``chip`` x ``chip`` image on the device, the cascade runs on the chips and the landmarks come
        back in frame coordinates (include/sdm.h, "Rolled faces").  ``chip`` defaults to the smallest multiple of 32 that is
        >= 1.75 x the largest box side, ``guard`` to ``chip // 8``; ``upright_info()`` returns the matrices and flags."""
        if roll is not None:
            return self._detect_batch_upright(images, faceboxes, img_index, roll, chip, guard, formats, chroma)
        if chip is not None or guard is not None:
            raise ValueError("chip and guard go with roll")
        from .synth import align_mean
        init = np.stack([align_mean(self.mean, tuple(int(v) for v in b)) for b in np.asarray(faceboxes)])
        hog = HogTransform(images, self.hog_params, self.landmark_ids, self.right_eye_ids, self.left_eye_ids,
                           img_index, formats=formats, chroma=chroma)
        return self.optimised_model.test(init, None, hog)

    @staticmethod
    def default_chip(faceboxes) -> int:
        """The smallest multiple of 32 that is >= 1.75 x the largest box side (at least 32)."""
        side = int(np.asarray(faceboxes).reshape(-1, 4)[:, 2:].max())
        return max(32, -(-(7 * side) // (4 * 32)) * 32)

    def _detect_batch_upright(self, images, faceboxes, img_index, roll, chip, guard, formats=None, chroma=None):
        opt = self.optimised_model
        boxes = np.asarray(faceboxes).reshape(-1, 4)
        chip = self.default_chip(boxes) if chip is None else int(chip)
        guard = chip // 8 if guard is None else int(guard)
        hog = HogTransform(images, self.hog_params, self.landmark_ids, self.right_eye_ids, self.left_eye_ids, img_index,
                           formats=formats, chroma=chroma)
        opt._bind(hog, boxes.shape[0])
        opt._load_regressors()
        c = opt.ctx
        c.set_templates(None)
        c.upright_configure(chip, guard)
        return c.detect_batch_upright(self.mean, boxes, roll)

    def upright_info(self):
        """(M n x 2 x 3, chip -> frame; flags n: SDM_UPRIGHT_PARTIAL / SDM_UPRIGHT_NEAR_EDGE bits) of the last upright detect or
        tracker step."""
        return self.optimised_model.ctx.upright_get()

    def estimate_pose(self, pose_model: SupervisedDescentOptimiser, projection: ModelProjection, landmark_ids: Sequence[str],
                      focal: Optional[float] = None, initialisation=None) -> np.ndarray:
        """Head pose of every face of the last ``detect_batch`` (N x 6, [r_x, r_y, r_z, t_x, t_y, t_z]) without taking the
        landmarks off the device: the K landmarks named by ``landmark_ids`` (ids of this model, one per model point of
        ``projection``, in its order) are gathered from the detect state and normalised by each row's image centre and ``focal``
        (default: the projection's), then ``pose_model``'s trained cascade runs on them.  ``initialisation``: one parameter row
        for every face (default [0, 0, 0, 0, 0, -2000], examples/pose_estimation.cpp:329-330)."""
        c = self.optimised_model.ctx
        missing = [i for i in landmark_ids if str(i) not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(str(i)) for i in landmark_ids]
        if len(idx) != projection.K:
            raise ValueError("one landmark id per model point of the projection expected")
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch first")
        pose_model._pose_bind(projection, c)
        c.pose_templates_from_landmarks(idx, projection.focal if focal is None else focal)
        x0 = np.array([0, 0, 0, 0, 0, -2000], np.float32) if initialisation is None else np.asarray(initialisation, np.float32).reshape(6)
        c.pose_set_x(np.tile(x0, (c.N, 1)))
        pose_model._pose_upload(c)
        c.pose_test(0, len(pose_model.regressors))
        return c.pose_get_x()

    def tracker(self, capacity: int, init: str = "realign", min_size: float = 8.0, max_scale_change: float = 1.5,
                chip: Optional[int] = None, guard: Optional[int] = None, smooth=None, motion=None) -> "Tracker":
        """Multi-stream tracking on the optimiser's context: ``capacity`` stream slots whose landmarks stay on the device from
        frame to frame (see :class:`Tracker`).  ``init``: how a tracked stream's next frame starts -- "previous" (its landmarks,
        the reference's ``detect(image, initialisation)``) or "realign" (the mean shape in their enclosing box).  A stream is
        lost when its result is not finite, its enclosing box is smaller than ``min_size`` pixels, the box centre leaves the
        image, or its inter-eye distance changes by more than the factor ``max_scale_change`` in one step (0: no such rule).
        ``init="upright"`` follows rolled faces: every step cuts each stream's face upright as a ``chip`` x ``chip`` image (the roll
        from the stream's own previous eye line), realigns in the chip, runs the cascade there and maps the result back; ``chip``
        (required) and ``guard`` (default ``chip // 8``) as for ``detect_batch(roll=...)``.
        ``smooth=(min_cutoff, beta)`` or ``(min_cutoff, beta, d_cutoff)``: a One-Euro filter on what ``step(..., dt=...)`` returns
        and leaves as the current rows -- ``min_cutoff`` (Hz) sets how steady a still face is, ``beta`` how fast the filter lets go
        when the face moves (in face sizes per second), ``d_cutoff`` defaults to 1 Hz.  Tracking itself is not changed by it.
        ``motion=True`` or ``(search, scale, min_gain)``: before the cascade every tracked stream's translation since its last frame
        is estimated by block matching on a 32 x 32 chip of block means and its start is shifted by it (include/sdm.h, "Tracking,
        motion-compensated") -- for faces that move by more than a few percent of their size per frame.  Defaults (8, 1.25, 64)."""
        return Tracker(self, capacity, init, min_size, max_scale_change, chip, guard, smooth, motion)

    def aligned_crops(self, size, landmark_ids: Optional[Sequence[str]] = None, template: Optional[np.ndarray] = None,
                      margin: float = 0.2, source=None, out=None):
        """Aligned face crops of the current rows -- the last ``detect_batch`` or ``Tracker.step`` -- without taking the landmarks or
        the frames off the device (include/sdm.h, sdm_align_*).  ``size``: an int (square) or (width, height).  ``landmark_ids``:
        the landmarks the similarity is fitted to (default: all of this model's).  ``template``: their K x 2 positions in crop
        pixels (default: :func:`alignment_template` of the mean with ``margin``).  ``source``: None (the context's gray images), a
        host array n x H x W [x C] or a contiguous uint8 device tensor of the same shape, e.g. the colour frames of the gray ones
        the cascade ran on (C in {1, 3, 4}, channel order kept).  ``out``: a uint8 device tensor of N x H x W x C bytes, written in
        place.  Returns (crops N x H x W x C uint8 -- or ``out`` --, matrices N x 2 x 3 crop -> source, flags N: SDM_ALIGN_*)."""
        c = self.optimised_model.ctx
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        c.align_set_source(source)
        try:
            return c.align_crops(idx, template, width, height, out=out)
        finally:
            if source is not None:
                c.align_set_source(None)                                  # (no pointer to the caller's frames stays behind)

    def aligned_crops_tensor(self, size, landmark_ids: Optional[Sequence[str]] = None, template: Optional[np.ndarray] = None,
                             margin: float = 0.2, frames=None, formats=None, chroma=None, dtype="float16", layout="nchw", channels=3,
                             order="rgb", scale=None, bias=None, mean=None, std=None, gray_shift=14, out=None, filter=None):
        """Aligned face crops of the current rows as a network's input tensor, in one launch from the frames where they lie on the
        device (include/sdm.h, sdm_align_crops_tensor).  ``size``, ``landmark_ids``, ``template``, ``margin``: as for
        :meth:`aligned_crops`.  ``frames``: what ``detect_batch`` and ``Tracker.step`` accept as device frames -- uint8 tensors of any
        size and row stride (gray, "bgr" / "rgb", "bgra" / "rgba" by ``formats``), (ptr, w, h, stride, format) tuples ("nv12": ptr = the
        Y plane; ``chroma``: per frame the UV plane's pointer or tensor, None = directly behind Y), one stacked tensor -- used in place,
        each with the size of the context image its row maps to; None: the context's own gray images.  ``dtype``: "float16" |
        "float32" | "uint8"; ``layout``: "nchw" | "nhwc"; ``channels``: 3 (a gray source is replicated) or 1 (colour is weighed with
        the gray weights of ``gray_shift``; NV12 gives Y); ``order``: "rgb" | "bgr".  Element = float32(v) * scale[c] + bias[c] per
        output channel c, the product and the sum each rounded to float32, then once to float16.  ``scale`` / ``bias``: a scalar or 3
        values, passed as float32.  ``mean`` / ``std`` (0-255 units) are sugar for ``scale = float32(1 / std)``,
        ``bias = float32(-mean / std)``; giving both pairs is an error.  ``out``: a contiguous device tensor of that dtype and shape.
        Returns (tensor, matrices N x 2 x 3 crop -> source, flags N: SDM_ALIGN_*).  No pointer to the frames stays behind.
        ``filter``: None (plain bilinear) | "area" | an ``SdmAlignFilter`` (``align_filter``): with a filter, a face that is larger in
        the frame than in the crop is averaged over every pixel's footprint (sdm_align_crops_tensor_filtered) and the return value is
        (tensor, matrices, flags, samples N: the sub-samples per axis of every row)."""
        c = self.optimised_model.ctx
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        spec = _lib.align_tensor_spec(dtype, layout, channels, order, scale, bias, mean, std, gray_shift)
        width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        c.align_set_source_frames(frames, formats, chroma)
        try:
            return c.align_crops_tensor(idx, template, width, height, spec=spec, out=out, filter=filter)
        finally:
            if frames is not None:
                c.align_set_source_frames(None)                           # (no pointer to the caller's frames stays behind)

    def warped_crops_tensor(self, size, landmark_ids: Optional[Sequence[str]] = None, template: Optional[np.ndarray] = None,
                            triangles: Optional[np.ndarray] = None, margin: float = 0.1, frames=None, formats=None, chroma=None,
                            dtype="float16", layout="nchw", channels=3, order="rgb", scale=None, bias=None, mean=None, std=None,
                            gray_shift=14, out=None, filter=None, max_samples=16, min_scale=1.0):
        """The faces of the current rows warped piecewise-affinely onto a template shape -- every landmark lands on its template point:
        the shape-normalised texture -- as a network's input tensor, in two launches from the frames where they lie on the device
        (include/sdm.h, "Warped faces").  ``size``, ``landmark_ids``, ``frames``, ``formats``, ``chroma``, the tensor options and ``out``: as
        for :meth:`aligned_crops_tensor`.  ``template``: the K x 2 positions of the landmarks in crop pixels (default:
        :func:`alignment_template` of the mean with ``margin``).  ``triangles``: T x 3 positions 0 .. K - 1, T <= 254 (default: the
        Delaunay triangulation of the template; a list of one's own may e.g. leave the mouth's interior out).  Pixels that no triangle
        covers are 0 before scale and bias; :meth:`warp_mask` tells them apart.  Returns (tensor, matrices N x T x 2 x 3 crop -> source,
        flags N: SDM_WARP_* bits).  No pointer to the frames stays behind.
        ``filter``: None (plain bilinear) | "area" | "bilinear" | an ``SdmAlignFilter``, with ``max_samples`` and ``min_scale`` as in
        :func:`align_filter`: with a filter, every pixel of a triangle that is larger in the frame than in the crop is averaged over its
        footprint, the sub-sample counts chosen per triangle and per axis (include/sdm.h, "Warped faces, filtered"), and the return
        value is (tensor, matrices, flags, samples N x T x 2: (Sx, Sy) of every triangle)."""
        c = self.optimised_model.ctx
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        filter = c._paste_filter(filter, max_samples, min_scale)
        spec = _lib.align_tensor_spec(dtype, layout, channels, order, scale, bias, mean, std, gray_shift)
        width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        if triangles is None:
            triangles = _lib.delaunay(template)
        c.warp_set_mesh(idx, template, triangles, width, height)
        self._warp_index = idx
        c.align_set_source_frames(frames, formats, chroma)
        try:
            return c.warp_crops_tensor(spec=spec, out=out, filter=filter)
        finally:
            if frames is not None:
                c.align_set_source_frames(None)                           # (no pointer to the caller's frames stays behind)

    def paste_crops_tensor(self, y, landmark_ids: Optional[Sequence[str]] = None, template: Optional[np.ndarray] = None, margin: float = 0.2,
                           frames=None, formats=None, layout="nchw", order="rgb", scale=None, bias=None, mean=None, std=None, gray_shift=14,
                           mask=None, matrices=None, image_index=None, filter=None, max_samples=16, min_scale=1.0, chroma=None):
        """The way back of :meth:`aligned_crops_tensor`: ``y = net(x)`` on the crops -- a device tensor, N x C x H x W or N x H x W x C by
        ``layout``; dtype, channels and crop size are read from it -- is warped back and blended into ``frames`` in place, in one launch
        (include/sdm.h, "Pasting crops back").  ``landmark_ids``, ``template``, ``margin``, ``order``, ``gray_shift``: as in the crop call,
        with the same defaults, so that ``paste(net(crop(...)))`` lands where it was cut.  ``frames`` / ``formats``: the destination, as
        for ``detect_batch`` on device frames; an "nv12" frame -- ``(y_ptr, width, height, stride, "nv12")``, with ``chroma`` per frame the
        UV plane's pointer, a uint8 tensor or None (directly behind the Y plane) as in the crop call -- has its luma and 4:2:0 chroma
        blended in place (include/sdm.h, "Pasting crops back into NV12 frames").  ``mean`` / ``std`` (0-255 units) as in the crop call: here they mean
        ``scale = std``, ``bias = mean``, the decoded value is ``e * scale + bias``.  ``mask``: the crop-space opacity -- None, or an H x W
        or N x H x W uint8 device tensor or numpy array, e.g. :func:`feather_mask`.  ``matrices`` (N x 2 x 3, as a crop call returned
        them) with ``image_index`` (None: row i -> frame i) pastes rows that are no longer current; otherwise the current rows are
        fitted again.  Returns (matrices N x 2 x 3 crop -> frame, flags N: SDM_ALIGN_*).  No pointer to the frames stays behind.
        ``filter``: None (plain bilinear) | "area" | "bilinear" | an ``SdmAlignFilter``, with ``max_samples`` and ``min_scale`` as in
        :func:`align_filter`: where the crop is larger than the face in the frame -- a 256- or 512-pixel network on a face 100 pixels
        wide -- every frame pixel averages S x S sub-samples of the crop (include/sdm.h, "Pasting crops back, filtered"), and the
        call returns (matrices, flags, S), as :meth:`aligned_crops_tensor` appends S."""
        c = self.optimised_model.ctx
        if frames is None:
            raise ValueError("give the frames to paste into")
        options = dict(order=order, scale=scale, bias=bias, mean=mean, std=std, gray_shift=gray_shift, filter=filter, max_samples=max_samples,
                       min_scale=min_scale)
        if chroma is not None:
            options["chroma"] = chroma
        if matrices is not None:
            m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 2, 3)
            got = c.align_paste_tensor_at(m, y, frames, formats, image_index, layout, mask, **options)
            return (m, got) if filter is None else (m,) + tuple(got)
        if image_index is not None:
            raise ValueError("image_index goes with matrices; the current rows map through the context's sample -> image index")
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        height, width = (int(y.shape[2]), int(y.shape[3])) if str(layout).lower() == "nchw" else (int(y.shape[1]), int(y.shape[2]))
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        return c.align_paste_tensor(idx, template, y, frames, formats, layout, mask, **options)

    def _region_index(self, regions, holes):
        """(polygons, holes, hull positions) as landmark positions of this model.  A region is a list of id names in order,
        ("hull", ids), or the name of a preset of ``ibug.REGIONS`` / ``ibug.REGIONS_RCR22`` (``ibug.region_preset``)."""
        if isinstance(regions, str) or (isinstance(regions, tuple) and len(regions) == 2 and regions[0] == "hull"):
            regions = [regions]
        if isinstance(holes, str) or (isinstance(holes, tuple) and len(holes) == 2 and holes[0] == "hull"):
            holes = [holes]
        polys, hull = [], []
        for g, region in enumerate(list(regions) + list(holes)):
            if isinstance(region, str):
                region = ibug.region_preset(region, self.landmark_ids)
            if isinstance(region, tuple) and len(region) == 2 and region[0] == "hull":
                hull.append(g)
                region = region[1]
            ids = [str(i) for i in region]
            missing = [i for i in ids if i not in self.landmark_ids]
            if missing:
                raise ValueError(f"landmark ids not in this model: {missing}")
            polys.append([self.landmark_ids.index(i) for i in ids])
        n = len(list(regions))
        return polys[:n], polys[n:], hull

    def region_masks(self, size, regions, holes=(), grow: float = 0.0, feather: float = 0.0, landmark_ids: Optional[Sequence[str]] = None,
                     template: Optional[np.ndarray] = None, margin: float = 0.2, matrices=None, points=None, out=None):
        """One crop-space opacity map per current row, drawn from its landmarks on the device (include/sdm.h, "Landmark region masks"):
        the union of ``regions`` minus ``holes``, moved outwards by ``grow`` crop pixels, with a linear ramp ``feather`` pixels wide.  A
        region is a list of landmark id names in order (a polygon), ``("hull", ids)`` (the convex hull of those landmarks) or a preset
        name of :data:`ibug.REGIONS` / :data:`ibug.REGIONS_RCR22` ("face", "right_eye", "mouth_outer", ...).  ``size``,
        ``landmark_ids``, ``template``, ``margin``: as in :meth:`aligned_crops_tensor`, with the same defaults, so that
        ``paste_crops_tensor(net(x), mask=region_masks(112, ["face"], feather=6)[0], ...)`` lines up with the crop.  ``matrices``
        (N x 2 x 3, as a crop call returned them) with ``points`` (:meth:`region_points` of that moment) draws rows that are no longer
        current.  ``out``: a contiguous uint8 device tensor N x height x width.  Returns (maps N x height x width uint8 on the device,
        matrices, flags N: SDM_ALIGN_* bits and SDM_REGION_NONFINITE); a flagged row's map is all zeros."""
        c = self.optimised_model.ctx
        width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        polys, hole_polys, hull = self._region_index(regions, holes)
        if (matrices is None) != (points is None):
            raise ValueError("matrices and points go together")
        if matrices is not None:
            m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 2, 3)
            maps, flags = c.align_region_mask_at(m, points, width, height, [len(p) for p in polys + hole_polys], len(hole_polys), hull, grow,
                                                 feather, out)
            return maps, m, flags
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        return c.align_region_mask(idx, template, width, height, polys, hole_polys, hull, grow, feather, out)

    def region_points(self, regions, holes=()) -> np.ndarray:
        """N x P x 2 float32: (x, y) of the vertices of ``regions`` followed by ``holes`` (as :meth:`region_masks` takes them) of the
        current rows, one polygon after the other -- what ``points=`` of :meth:`region_masks` takes later, the counterpart of
        :meth:`warp_points`."""
        c = self.optimised_model.ctx
        polys, hole_polys, _ = self._region_index(regions, holes)
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        x = np.asarray(c.get_x(), np.float32)
        L = x.shape[1] // 2
        idx = np.asarray([v for p in polys + hole_polys for v in p], np.int64)
        return np.ascontiguousarray(np.stack([x[:, idx], x[:, L + idx]], -1))

    def _warp_mesh_of(self, width, height, landmark_ids, template, triangles, margin):
        ids = self.landmark_ids if landmark_ids is None else [str(i) for i in landmark_ids]
        missing = [i for i in ids if i not in self.landmark_ids]
        if missing:
            raise ValueError(f"landmark ids not in this model: {missing}")
        idx = [self.landmark_ids.index(i) for i in ids]
        if template is None:
            template = alignment_template(self.mean, idx, width, height, margin)
        if triangles is None:
            triangles = _lib.delaunay(template)
        return idx, template, triangles

    def paste_warped_tensor(self, y, landmark_ids: Optional[Sequence[str]] = None, template: Optional[np.ndarray] = None,
                            triangles: Optional[np.ndarray] = None, margin: float = 0.1, frames=None, formats=None, layout="nchw",
                            order="rgb", scale=None, bias=None, mean=None, std=None, gray_shift=14, mask=None, points=None,
                            image_index=None, chroma=None, filter=None, max_samples=16, min_scale=1.0):
        """The way back of :meth:`warped_crops_tensor`: ``y = net(x)`` on the warped faces -- a texture in template space, a device tensor
        whose dtype, channels and crop size are read from it -- is warped back under every face's own shape and blended into ``frames``
        in place (include/sdm.h, "Pasting warped faces back").  ``landmark_ids``, ``template``, ``triangles``, ``margin``, ``order``,
        ``gray_shift``: as in the warp call, with the same defaults, so that ``paste_warped(net(warped_crops(...)))`` lands where it was
        cut.  ``frames``, ``formats``, ``mean`` / ``std``, ``mask``: as for :meth:`paste_crops_tensor`; a tap outside the mesh's hull has
        opacity 0 whatever the mask says (:func:`feather_warp_mask` fades inside it).  ``points`` (N x K x 2, :meth:`warp_points` of
        an earlier moment) with ``image_index`` (None: row i -> frame i) pastes rows that are no longer current; otherwise the current
        rows are fitted again.  Returns (matrices N x T x 2 x 3 crop -> frame or None with ``points``, flags N: SDM_WARP_* bits).  No
        pointer to the frames stays behind.  An "nv12" frame, with ``chroma`` as for :meth:`paste_crops_tensor`, has its luma and 4:2:0
        chroma blended in place (include/sdm.h, "Pasting warped faces back into NV12 frames").  ``filter``: None (plain bilinear) |
        "area" | "bilinear" | an ``SdmAlignFilter``, with ``max_samples`` and ``min_scale`` as in :func:`align_filter`: where a
        triangle of the face is smaller in the frame than in the crop, every frame pixel averages Sx x Sy sub-samples of the crop,
        chosen per triangle and per axis (include/sdm.h, "Pasting warped faces back, filtered"), and the call returns (matrices or
        None, flags, samples N x T x 2)."""
        c = self.optimised_model.ctx
        if frames is None:
            raise ValueError("give the frames to paste into")
        if not hasattr(y, "shape") or len(y.shape) != 4:
            raise ValueError("the tensor must be a contiguous 4-dimensional tensor on the device")
        height, width = (int(y.shape[2]), int(y.shape[3])) if str(layout).lower() == "nchw" else (int(y.shape[1]), int(y.shape[2]))
        if points is None:
            if image_index is not None:
                raise ValueError("image_index goes with points; the current rows map through the context's sample -> image index")
            if not getattr(c, "N", 0):
                raise RuntimeError("run detect_batch or Tracker.step first")
        idx, template, triangles = self._warp_mesh_of(width, height, landmark_ids, template, triangles, margin)
        c.warp_set_mesh(idx, template, triangles, width, height)
        self._warp_index = idx
        options = dict(order=order, scale=scale, bias=bias, mean=mean, std=std, gray_shift=gray_shift)
        if chroma is not None:
            options["chroma"] = chroma
        if filter is not None:
            options.update(filter=filter, max_samples=max_samples, min_scale=min_scale)
        if points is not None:
            got = c.warp_paste_tensor_at(points, y, frames, formats, image_index, layout, mask, **options)
            return (None, got) if filter is None else (None,) + tuple(got)
        return c.warp_paste_tensor(y, frames, formats, layout, mask, **options)

    def warp_points(self) -> np.ndarray:
        """N x K x 2 float32: (x, y) of the mesh's K landmarks of the current rows, in the order of the last
        :meth:`warped_crops_tensor` / :meth:`paste_warped_tensor` mesh -- what ``points=`` of :meth:`paste_warped_tensor` takes later."""
        c = self.optimised_model.ctx
        idx = getattr(self, "_warp_index", None)
        if idx is None:
            raise RuntimeError("run warped_crops_tensor or paste_warped_tensor first")
        if not getattr(c, "N", 0):
            raise RuntimeError("run detect_batch or Tracker.step first")
        x = np.asarray(c.get_x(), np.float32)
        L = x.shape[1] // 2
        idx = np.asarray(idx, np.int64)
        return np.ascontiguousarray(np.stack([x[:, idx], x[:, L + idx]], -1))

    def warp_mask(self) -> np.ndarray:
        """height x width bool of the last :meth:`warped_crops_tensor`'s mesh: True where a triangle covers the crop pixel."""
        return self.optimised_model.ctx.warp_labels() != _lib.SDM_WARP_NO_TRIANGLE

    def get_mean(self) -> np.ndarray:
        return self.mean


def alignment_template(mean: np.ndarray, landmark_index: Sequence[int], width: int, height: int, margin: float = 0.2) -> np.ndarray:
    """The default crop template (K x 2 float32, crop pixels), computed in float64: the mean's selected points with their enclosing
    box centred in the crop ((width - 1) / 2, (height - 1) / 2) and scaled so that its larger side is (1 - 2 margin) of the crop's
    smaller side."""
    m = np.asarray(mean, np.float64).reshape(-1)
    L = m.size // 2
    idx = np.asarray(landmark_index, np.int64)
    px, py = m[idx], m[L + idx]
    extent = max(px.max() - px.min(), py.max() - py.min())
    if not extent > 0:
        raise ValueError("the selected mean points have no extent")
    s = (1.0 - 2.0 * margin) * min(width, height) / extent
    tx = (px - (px.min() + px.max()) / 2) * s + (width - 1) / 2
    ty = (py - (py.min() + py.max()) / 2) * s + (height - 1) / 2
    return np.stack([tx, ty], 1).astype(np.float32)


def feather_mask(size, border: int) -> np.ndarray:
    """A crop-space opacity map for :meth:`detection_model.paste_crops_tensor` (height x width uint8, computed on the host): 255 in the
    interior, a linear ramp to 0 over ``border`` pixels towards every edge -- pixel k from an edge has round(255 (k + 1) / (border + 1)).
    ``size``: an int (square) or (width, height)."""
    width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    if border < 0 or width < 1 or height < 1:
        raise ValueError("size must be >= 1 and border >= 0")
    dx = np.minimum(np.arange(width), np.arange(width)[::-1])[None, :]
    dy = np.minimum(np.arange(height), np.arange(height)[::-1])[:, None]
    k = np.minimum(np.minimum(dx, dy) + 1, border + 1)
    return np.rint(255.0 * k / (border + 1)).astype(np.uint8)


def feather_warp_mask(mask, radius: int) -> np.ndarray:
    """A crop-space opacity map for :meth:`detection_model.paste_warped_tensor` (height x width uint8, computed on the host) from a bool
    height x width map such as :meth:`detection_model.warp_mask`: 0 on unlabelled pixels, rising linearly to 255 over ``radius`` pixels of
    city-block distance -- a pixel at distance d from the nearest unlabelled or out-of-crop pixel has
    round(255 min(d, radius + 1) / (radius + 1)); ``radius`` = 0 gives 255 where the mask is set."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype != np.bool_:
        raise ValueError("mask must be a bool height x width map")
    if radius < 0:
        raise ValueError("radius must be >= 0")
    h, w = m.shape
    # city-block distance to the nearest False pixel, the crop's outside counting as False: two sweeps
    big = h + w + 2
    d = np.where(np.pad(m, 1), big, 0).astype(np.int64)
    for i in range(1, h + 2):
        d[i] = np.minimum(d[i], d[i - 1] + 1)
    for i in range(h, -1, -1):
        d[i] = np.minimum(d[i], d[i + 1] + 1)
    for j in range(1, w + 2):
        d[:, j] = np.minimum(d[:, j], d[:, j - 1] + 1)
    for j in range(w, -1, -1):
        d[:, j] = np.minimum(d[:, j], d[:, j + 1] + 1)
    k = np.minimum(d[1:-1, 1:-1], radius + 1)
    return np.rint(255.0 * k / (radius + 1)).astype(np.uint8)


class Tracker:
    """Faces followed through video, many streams at once (the loop the reference's apps/rcr/rcr-track.cpp:133-177 sketches):
    ``start`` a stream from a face box, ``step`` the streams on their next frames, restart the ones reported lost from a new box.
    The landmark state of every stream lives in a slot table on the device (include/sdm.h, sdm_track_*); a step runs
    ``detect_batch``'s cascade on the stepped streams and leaves its rows as the context's current x, so ``estimate_pose``
    works on tracked faces as on detected ones."""

    _MODES = {"previous": _lib.SDM_TRACK_INIT_PREVIOUS, "realign": _lib.SDM_TRACK_INIT_REALIGN}

    def __init__(self, model: detection_model, capacity: int, init: str = "realign", min_size: float = 8.0,
                 max_scale_change: float = 1.5, chip: Optional[int] = None, guard: Optional[int] = None, smooth=None, motion=None):
        self.smooth = self._smooth(smooth)
        self.motion_params = self._motion(motion)
        if init not in self._MODES and init != "upright":
            raise ValueError('init must be "previous", "realign" or "upright"')
        if init == "upright" and chip is None:
            raise ValueError('init="upright" needs the chip size')
        if init != "upright" and (chip is not None or guard is not None):
            raise ValueError('chip and guard go with init="upright"')
        self.model, self.capacity, self.init = model, int(capacity), init
        self._bind()
        self.ctx.track_configure(self.capacity, model.mean, self._MODES.get(init, _lib.SDM_TRACK_INIT_REALIGN), min_size, max_scale_change)
        if init == "upright":
            self.ctx.upright_configure(int(chip), int(chip) // 8 if guard is None else int(guard))
        if init == "upright" or getattr(self.ctx, "track_upright", False):      # (off again for a plain tracker on the same context)
            self.ctx.track_configure_upright(init == "upright")
        if self.smooth is not None:
            self.ctx.track_configure_filter(*self.smooth)
        if self.motion_params is not None:
            self.ctx.track_configure_motion(*self.motion_params)

    @staticmethod
    def _motion(motion):
        """(search, scale, min_gain) as (int, float, int), or None; True: the defaults"""
        if motion is None or motion is False:
            return None
        if motion is True:
            return (8, 1.25, MOTION_MIN_GAIN)
        try:
            v = tuple(motion)
        except TypeError:
            raise ValueError("motion is True or (search, scale, min_gain)") from None
        if len(v) != 3:
            raise ValueError("motion is True or (search, scale, min_gain)")
        try:
            ok = float(v[0]) == int(v[0]) and float(v[2]) == int(v[2]) and 1 <= int(v[0]) <= 16 and 0.5 <= float(v[1]) <= 4.0 and \
                0 <= int(v[2]) <= 255
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("motion needs search in 1 ... 16, scale in [0.5, 4] and min_gain in 0 ... 255")
        return (int(v[0]), float(v[1]), int(v[2]))

    @staticmethod
    def _smooth(smooth):
        """(min_cutoff, beta[, d_cutoff = 1.0]) as three floats, or None"""
        if smooth is None:
            return None
        try:
            v = tuple(float(a) for a in smooth)
        except TypeError:
            raise ValueError("smooth is (min_cutoff, beta) or (min_cutoff, beta, d_cutoff)") from None
        if len(v) not in (2, 3):
            raise ValueError("smooth is (min_cutoff, beta) or (min_cutoff, beta, d_cutoff)")
        v = v if len(v) == 3 else v + (1.0,)
        if not (np.isfinite(v).all() and v[0] > 0 and v[1] >= 0 and v[2] > 0):
            raise ValueError("smooth needs min_cutoff > 0, beta >= 0 and d_cutoff > 0")
        return v

    @property
    def ctx(self) -> Context:
        return self.model.optimised_model.ctx

    def _bind(self):
        """The model's geometry on the context (a no-op when it is already there) and its regressors (not uploaded again when the
        device holds them: SupervisedDescentOptimiser._load_regressors)."""
        m, opt = self.model, self.model.optimised_model
        norm = opt.normalisation or InterEyeDistanceNormalisation(m.landmark_ids, m.right_eye_ids, m.left_eye_ids)
        self.ctx.set_model_geometry(len(m.landmark_ids), norm.right_eye, norm.left_eye, m.hog_params)
        opt._load_regressors()

    def start(self, ids, boxes, roll=None):
        """(Re)start streams from face boxes (n x (x, y, w, h)), live or lost.  ``roll`` (degrees, one value or one per stream;
        ``init="upright"`` only): the roll of the faces in their boxes."""
        if roll is None:
            self.ctx.track_start(ids, boxes)
        else:
            self.ctx.track_start_rolled(ids, boxes, roll)

    def stop(self, ids):
        self.ctx.track_stop(ids)

    def step(self, ids, frames=None, image_index=None, fetch: bool = True, formats=None, gray_shift: int = 14, dt=None, chroma=None):
        """One frame for the streams ``ids``: row i belongs to stream ids[i] and reads frame ``image_index[i]`` (default i).
        ``frames``: host images (a list or an n x H x W stack, uploaded), a uint8 n x H x W tensor on the device (used in place),
        any other device input of ``Context.set_frames_device`` -- a list of gray or colour tensors of different sizes, pitched
        views, a stacked n x H x W x C tensor, planar 3 x H x W tensors named "bgr_planar" / "rgb_planar" by ``formats``,
        (ptr, w, h, stride, format) tuples; ``formats``, ``gray_shift`` and ``chroma`` (planar tuples' second planes) go with it --
        or None (the images already set on the context).  Returns (landmarks n x 2L -- None unless ``fetch`` --, lost masks n:
        0 = tracked, else the SDM_TRACK_LOST_* bits).
        ``dt`` (a tracker with ``smooth`` only; seconds since the streams' last step with ``dt``, one value or one per row): the
        step's rows go through the filter, and the return is (filtered n x 2L, lost masks n, raw n x 2L) -- the two row entries None
        unless ``fetch``.  The filtered rows are the context's current rows: crops, warps, pastes and poses follow them."""
        if dt is not None:
            if self.smooth is None:
                raise ValueError("dt needs a tracker with smooth=(min_cutoff, beta)")
            dt = np.asarray(dt, np.float32).reshape(-1)
            if dt.size not in (1, np.atleast_1d(np.asarray(ids)).size):
                raise ValueError("dt is one value or one per stream id")
        c = self.ctx
        self._bind()
        if frames is not None:
            if hasattr(frames, "data_ptr") and getattr(frames, "is_cuda", False) and frames.dim() == 3 and frames.is_contiguous() and \
                    _lib._one_planar_name(formats) is None:                     # (one 3 x H x W frame named planar is no stack of gray images)
                if frames.dtype.itemsize != 1:
                    raise ValueError("device frames must be uint8")
                import torch
                torch.cuda.current_stream(frames.device).synchronize()      # (the library runs on its own stream)
                n, h, w = (int(v) for v in frames.shape)
                c.set_images_device(frames.data_ptr(), n, w, h, w)
            elif _device_frames(frames):
                c.set_frames_device(frames, formats, gray_shift, chroma)    # (colour, ragged, pitched, planar: sdm_set_frames_device)
            else:
                c.upload_images(frames)
            self.model.optimised_model._bound = None                        # (the context's images are no longer a bound projection's)
        c.set_templates(None)
        c.set_sample_image_index(image_index)
        return c.track_step(ids, fetch) if dt is None else c.track_step_filtered(ids, dt, fetch)

    def get(self, ids):
        """(landmarks n x 2L, status n: SDM_TRACK_FREE / STARTED / TRACKED / LOST) of the streams ``ids``."""
        return self.ctx.track_get(ids)

    def motion(self, ids):
        """(motion n x 6 int32: the last step's shift dx, dy in pixels, best SAD, SAD(0, 0), k, searched; grid n x 3 int32: k, ox, oy;
        chips n x 32 x 32 uint8) of the streams ``ids`` -- a tracker with ``motion`` only."""
        if self.motion_params is None:
            raise ValueError("motion needs a tracker with motion=True or (search, scale, min_gain)")
        return self.ctx.track_get_motion(ids)

    def get_filtered(self, ids):
        """(filtered rows n x 2L, their derivative in pixels per second n x 2L, primed flags n) of the streams ``ids``; a stream
        whose filter holds nothing yet -- not stepped with ``dt`` since its start -- gives zeros."""
        if self.smooth is None:
            raise ValueError("get_filtered needs a tracker with smooth=(min_cutoff, beta)")
        return self.ctx.track_get_filtered(ids)
