"""superviseddescent_amd -- MI355X-native engine for the data-parallel hot path of
patrikhuber/superviseddescent (batched HOG extraction + LinearRegressor normal equations / apply).

Product code.  The HIP kernels live in ``csrc/`` and are reached only through the C-ABI declared in
``include/sdm.h``; this package is the Python mirror of the reference's operator surface on top of it.
"""
from .engine import (ColPivHouseholderQRSolver, Context, HoGParam, HogTransform, InterEyeDistanceNormalisation, LinearRegressor,
                     ModelProjection, PartialPivLUSolver, Regulariser, RegulariserSweep, SupervisedDescentOptimiser, Tracker, alignment_template, feather_mask, feather_warp_mask,
                     detection_model)
from ._lib import SdmError, align_filter, align_tensor_spec, paste_tensor_spec, delaunay, frame_descriptors, frame_planes

__all__ = ["ColPivHouseholderQRSolver", "PartialPivLUSolver", "Context", "HoGParam", "HogTransform", "InterEyeDistanceNormalisation", "LinearRegressor",
           "ModelProjection", "Regulariser", "RegulariserSweep", "SupervisedDescentOptimiser", "Tracker", "alignment_template", "detection_model", "SdmError", "frame_descriptors", "frame_planes", "align_tensor_spec", "align_filter", "delaunay", "paste_tensor_spec", "feather_mask", "feather_warp_mask"]
