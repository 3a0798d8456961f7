// sdm_warp.h -- what csrc/sdm_warp.hip (kernels) and csrc/sdm_capi_warp.hip (C-ABI) of the piecewise-affine face warp share
// (include/sdm.h, "Warped faces"): the per-row record and the launches.
#pragma once
#include "sdm_kernels.h"
#include "sdm_warp_device.h"

#define SDM_WARP_MAX_TRIANGLES 254

// per row: the SDM_WARP_* flags and the row's image (its first byte from the source base, unless the source is a frame list)
struct WarpFace {
    int flags;
    int w, h, stride;
    long long off;
};

// x: N x 2L; lm: the mesh's K landmark indices; tri: T triangles; src, img_idx: as for sdm_launch_align_fit.  faces: N records;
// matrices: N x T x 6 floats
void sdm_launch_warp_fit(const float* x, int N, int L, const int* lm, int K, const WarpTri* tri, int T, const AlignSourceDev& src,
                         const int* img_idx, WarpFace* faces, float* matrices, hipStream_t s);
// labels: out_h x out_w bytes, 4-byte aligned.  base, frames, img_idx, src_format, spec, out: as for sdm_launch_align_tensor.
void sdm_launch_warp_tensor(const uint8_t* base, const WarpFace* faces, const float* matrices, int T, const uint8_t* labels,
                            const AlignFrameDev* frames, const int* img_idx, int src_format, int N, int out_w, int out_h, int dtype,
                            int layout, int channels, const AlignTensorDev& spec, void* out, hipStream_t s);
// the same with area-averaged sampling (csrc/sdm_warp_area.hip).  samples: N x T x 2 ints (Sx, Sy), 8-byte aligned, written by the launch
void sdm_launch_warp_area(const uint8_t* base, const WarpFace* faces, const float* matrices, int T, const uint8_t* labels,
                          const AlignFrameDev* frames, const int* img_idx, int src_format, int N, int out_w, int out_h, int dtype,
                          int layout, int channels, const AlignTensorDev& spec, const AlignAreaDev& area, int* samples, void* out,
                          hipStream_t s);
