// sdm_warp_paste.h -- what csrc/sdm_warp_paste.hip (kernels) and csrc/sdm_capi_paste.hip (C-ABI) of the piecewise-affine paste share
// (include/sdm.h, "Pasting warped faces back"): the records of csrc/sdm_warp_paste_device.h and the two launches.
#pragma once
#include "sdm_kernels.h"
#include "sdm_warp_paste_device.h"

// x: N x 2L; lm: the mesh's K landmark indices; tri: T triangles; faces, matrices: the N records (their FOLDED bit is read) and the
// N x T x 6 floats of sdm_launch_warp_fit; frame_of_row: N checked indices into frames.  rows: N records; tris: N x T records
void sdm_launch_warp_paste_prepare(const float* x, int N, int L, const int* lm, int K, const WarpTri* tri, int T, const WarpFace* faces,
                                   const float* matrices, const int* frame_of_row, const PasteFrameDev* frames, WarpPasteRow* rows,
                                   WarpPasteTri* tris, hipStream_t s);
// list, entry_of_row: as for sdm_launch_paste.  labels: the mesh's label map, crop.ch x crop.cw bytes
void sdm_launch_warp_paste(const PasteFrameDev* frames, const WarpPasteRow* rows, const WarpPasteTri* tris, int T, const int* list,
                           const int* entry_of_row, int N, const uint8_t* labels, const PasteCropDev& crop, hipStream_t s);
