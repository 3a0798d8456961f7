// sdm_paste.h -- what the two paste kernels (csrc/sdm_align_paste.hip, csrc/sdm_warp_paste.hip) and their C-ABI (csrc/sdm_capi_paste.hip)
// share: the device headers' records, the launches, and a paste kernel's tile walk -- grid (row, paste_groups workgroups); the
// workgroups of a row stride over the 64 x 4 pixel tiles of its box, a wave covers 64 pixels of one frame row: the box never reaches the host.
#pragma once
#include <type_traits>
#include "sdm_warp.h"
#include "sdm_align_paste_device.h"
#include "sdm_align_paste_area_device.h"
#include "sdm_warp_paste_device.h"

#define PASTE_BLOCK 256
#define PASTE_TILE_W 64
#define PASTE_TILE_H (PASTE_BLOCK / PASTE_TILE_W)

// the tiles of a box of bw x bh pixels, across and down; tile t's first pixel from the box's, with tx tiles across
ALIGN_HD int paste_tiles_x(int bw) { return (bw + PASTE_TILE_W - 1) / PASTE_TILE_W; }
ALIGN_HD int paste_tiles_y(int bh) { return (bh + PASTE_TILE_H - 1) / PASTE_TILE_H; }
ALIGN_HD int paste_tile_x(long long t, int tx) { return (int)(t % tx) * PASTE_TILE_W; }
ALIGN_HD int paste_tile_y(long long t, int tx) { return (int)(t / tx) * PASTE_TILE_H; }

// workgroups per row: one per 1 024 crop pixels, 1 ... 32 (a 112 x 112 crop: 13)
inline int paste_groups(const PasteCropDev& crop)
{
    const int groups = (crop.cw * crop.ch + 1023) / 1024;
    return groups < 1 ? 1 : (groups > 32 ? 32 : groups);
}

// A paste kernel is one __global__ template over <NV12, AREA>; a parameter that an instantiation does not take -- the UV planes
// without NV12, the filter's records without AREA -- has this type there: no size, no kernarg bytes, PasteNone{} at the launch
struct PasteNone { int none[0]; };
template <bool ON, class P> using PasteOpt = std::conditional_t<ON, P, PasteNone>;

// faces: N records holding M (fitted: and the fit's flags; otherwise PARTIAL is evaluated here); the final flags go back into them.
// frame_of_row: N frame indices; rows: N records out
void sdm_launch_paste_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                              PasteRow* rows, hipStream_t s);
// the filtered calls' prepare stage.  area: the filter; area_rows: N records out; samples: N ints out, S of every row
void sdm_launch_paste_area_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                                   const AlignAreaDev& area, PasteRow* rows, PasteAreaRow* area_rows, int* samples, hipStream_t s);
// the paste behind either prepare stage: paste_kernel_t<chroma != null, area_rows != null, planar>; planar: the frame list holds a planar
// colour frame (only those instances carry the planar case of the pixel's load and store).  list: the rows of every frame, ascending
// (PasteFrameDev::row_begin / row_end); entry_of_row: where row n stands in it.  chroma: null -- no frame is NV12 --, or one UV plane
// per frame (read for NV12 frames only); area_rows: null -- plain bilinear --, or the filtered prepare stage's records.  yuv: an NV12
// frame of the list carries a colour description (a matrix or range bit): the instances whose block path reads its table row
void sdm_launch_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const PasteRow* rows, const PasteAreaRow* area_rows, const int* list,
                      const int* entry_of_row, int N, const PasteCropDev& crop, bool planar, bool yuv, hipStream_t s);
// x: N x 2L; lm: the mesh's K landmark indices; tri: T triangles; faces, matrices: the N records (their FOLDED bit is read) and the
// N x T x 6 floats of sdm_launch_warp_fit; frame_of_row: N checked indices into frames.  rows: N records; tris: N x T records
void sdm_launch_warp_paste_prepare(const float* x, int N, int L, const int* lm, int K, const WarpTri* tri, int T, const WarpFace* faces,
                                   const float* matrices, const int* frame_of_row, const PasteFrameDev* frames, WarpPasteRow* rows,
                                   WarpPasteTri* tris, hipStream_t s);
// the filtered piecewise-affine calls' stage behind sdm_launch_warp_paste_prepare.  counts: N x T packed (Sx, Sy) out
// (csrc/sdm_warp_paste_area_device.h); samples: N x T x 2 ints out, for the host
void sdm_launch_warp_paste_area_counts(const WarpPasteRow* rows, const WarpPasteTri* tris, int N, int T, const AlignAreaDev& area,
                                       uint16_t* counts, int* samples, hipStream_t s);
// the piecewise-affine paste: warp_paste_kernel_t<chroma != null, counts != null>.  list, entry_of_row, chroma: as for sdm_launch_paste;
// labels: the mesh's label map, crop.ch x crop.cw bytes; counts: null -- unfiltered --, or the counts stage's (then chroma is not
// null: the filtered calls take a list that may mix NV12 and the per-pixel formats)
void sdm_launch_warp_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const WarpPasteRow* rows, const WarpPasteTri* tris,
                           const uint16_t* counts, int T, const int* list, const int* entry_of_row, int N, const uint8_t* labels,
                           const PasteCropDev& crop, bool planar, bool yuv, hipStream_t s);
