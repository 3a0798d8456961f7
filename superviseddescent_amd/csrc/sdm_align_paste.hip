// sdm_align_paste.hip -- crop tensors pasted back into frames on gfx950 (include/sdm.h, "Pasting crops back", "..., filtered", "... into
// NV12 frames"), behind the fit of sdm_align_crops or a caller's matrices.
//
//   paste_prepare_kernel   one lane per row: the inverse map W (double, rounded once to float32), the flags and the footprint's box in
//                          the row's frame, written as one PasteRow record; the final flags go back into the fit's record
//   paste_area_prepare_kernel   the filtered calls' prepare stage: it also leaves S and the working footprint of every row (PasteAreaRow)
//   paste_kernel_t<NV12, AREA>   the paste, one text for its four instantiations: NV12 for the calls that take NV12 destinations, AREA
//                          behind paste_area_prepare_kernel.  The tile walk of csrc/sdm_paste.h over the row's box.  A lane's pixel is
//                          pasted by the lowest-numbered row of the frame whose footprint holds it (paste_pixel, paste_owned): every
//                          frame byte has at most one reader and writer in the launch, whatever the order the workgroups run in.
//                          Stores are per pixel, byte by byte: nothing a neighbour owns is touched.
//                          AREA is the same tile walk and the same ownership rule on the shape PasteRigidArea (paste_area_pixel).  S is
//                          uniform for a workgroup (one row) and, in the owner loop, per list entry: every sub-sample loop has a
//                          wave-uniform trip count.  Rows with S = 1 take the unfiltered per-pixel code.
//                          NV12: the frame's format is uniform for a workgroup, and a frame that is not NV12 takes the pixel walk
//                          above.  On an NV12 frame the tile walk runs over the 2 x 2 blocks of the row's box widened to even
//                          coordinates -- a wave covers 64 blocks of one block row -- and a block is pasted by the lowest-numbered row
//                          of the frame whose footprint holds one of its pixels (paste_owned_block): every byte of both planes has at
//                          most one reader and writer in the launch.  The UV planes come as an array of their own beside the frame
//                          table, which the other instantiations read as they did.
//
// The per-pixel arithmetic is csrc/sdm_align_paste_device.h and csrc/sdm_align_paste_area_device.h on top of csrc/sdm_paste_device.h.
#include "sdm_paste.h"

#pragma clang fp contract(off)

namespace {

#define PASTE_PREPARE_BLOCK 64

__global__ __launch_bounds__(PASTE_PREPARE_BLOCK) void paste_prepare_kernel(AlignFace* __restrict__ faces, const int* __restrict__ frame_of_row,
                                                                            const PasteFrameDev* __restrict__ frames, int N, int cw, int ch,
                                                                            int fitted, PasteRow* __restrict__ rows)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int fi = frame_of_row[n];
    const PasteFrameDev f = frames[fi];
    float m[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) m[e] = faces[n].m[e];
    PasteRow r;
    paste_prepare_row(m, fitted ? faces[n].flags : -1, fi, f.w, f.h, cw, ch, r);
    rows[n] = r;
    faces[n].flags = r.flags;
}

__global__ __launch_bounds__(PASTE_PREPARE_BLOCK) void paste_area_prepare_kernel(AlignFace* __restrict__ faces, const int* __restrict__ frame_of_row,
                                                                                 const PasteFrameDev* __restrict__ frames, int N, int cw, int ch,
                                                                                 int fitted, AlignAreaDev area, PasteRow* __restrict__ rows,
                                                                                 PasteAreaRow* __restrict__ area_rows, int* __restrict__ samples)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int fi = frame_of_row[n];
    const PasteFrameDev f = frames[fi];
    float m[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) m[e] = faces[n].m[e];
    PasteRow r;
    PasteAreaRow ar;
    paste_area_prepare_row(m, fitted ? faces[n].flags : -1, fi, f.w, f.h, cw, ch, area.mode, area.max_samples, area.min2, r, ar);
    rows[n] = r;
    area_rows[n] = ar;
    samples[n] = ar.S;
    faces[n].flags = r.flags;
}

// (area_rows is a parameter of <true, false> too, null there).  PLANAR: the frame list holds a planar colour frame -- only then is the
// planar case of paste_load / paste_store in the kernel's code, so the lists of the other formats run the text they always ran
// YUV: an NV12 frame of the list carries a colour description -- the block path takes its constants from the frame's table row
// (csrc/sdm_yuv_device.h); lists of value 5 alone run the text they always ran
template <bool NV12, bool AREA, bool PLANAR, bool YUV>
__global__ __launch_bounds__(PASTE_BLOCK) void paste_kernel_t(const PasteFrameDev* __restrict__ frames, PasteOpt<NV12, uint8_t* const* __restrict__> chroma,
                                                              const PasteRow* __restrict__ rows,
                                                              PasteOpt<NV12 || AREA, const PasteAreaRow* __restrict__> area_rows,
                                                              const int* __restrict__ list, const int* __restrict__ entry_of_row, PasteCropDev c)
{
    // the row, its list entry and its frame: uniform for the workgroup
    const int n = blockIdx.x;
    const int k = entry_of_row[n];
    const PasteRow r = rows[n];
    // an empty box.  One test in two spellings: whether the height is taken ahead of the width's test or behind it decides how the
    // compiler splits the loads of r, in every instantiation alike, and the kernels this template replaces stood on either side
    // (profiles/paste_template_isa_identity.txt): each pair keeps the spelling that gives it the instructions it had
    if constexpr (NV12) {
        if (r.x1 - r.x0 <= 0 || r.y1 - r.y0 <= 0) return;
    } else {
        const int bw = r.x1 - r.x0, bh = r.y1 - r.y0;
        if (bw <= 0 || bh <= 0) return;
    }
    const PasteFrameDev f = frames[r.frame];
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    if (!NV12 || (YUV ? SDM_FRAME_BASE(f.format) : f.format) != SDM_FRAME_NV12) {
        const int tx = paste_tiles_x(r.x1 - r.x0), ty = paste_tiles_y(r.y1 - r.y0);
        for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
            const int X = r.x0 + paste_tile_x(t, tx) + lx, Y = r.y0 + paste_tile_y(t, tx) + ly;
            if (X < r.x1 && Y < r.y1) {
                if constexpr (AREA) paste_area_pixel<PLANAR>(f, rows, area_rows, list, k, c, X, Y);
                else paste_pixel<PLANAR>(f, rows, list, k, c, X, Y);
            }
        }
        return;
    }
    if constexpr (NV12) {
        // the blocks of the box widened to even coordinates: [bx0, bx1) x [by0, by1)
        uint8_t* const uv = chroma[r.frame];
        const int bx0 = r.x0 >> 1, by0 = r.y0 >> 1, bx1 = (r.x1 + 1) >> 1, by1 = (r.y1 + 1) >> 1;
        const int tx = paste_tiles_x(bx1 - bx0), ty = paste_tiles_y(by1 - by0);
        for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
            const int BX = bx0 + paste_tile_x(t, tx) + lx, BY = by0 + paste_tile_y(t, tx) + ly;
            if (BX < bx1 && BY < by1) {
                if constexpr (AREA) paste_owned_block<YUV>(f, uv, PasteRigidArea{rows, area_rows}, list, k, c, BX, BY);
                else paste_owned_block<YUV>(f, uv, PasteRigid{rows}, list, k, c, BX, BY);
            }
        }
    }
}

}  // namespace

void sdm_launch_paste_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                              PasteRow* rows, hipStream_t s)
{
    hipLaunchKernelGGL(paste_prepare_kernel, dim3((unsigned)((N + PASTE_PREPARE_BLOCK - 1) / PASTE_PREPARE_BLOCK)), dim3(PASTE_PREPARE_BLOCK), 0, s,
                       faces, frame_of_row, frames, N, cw, ch, fitted ? 1 : 0, rows);
}

void sdm_launch_paste_area_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                                   const AlignAreaDev& area, PasteRow* rows, PasteAreaRow* area_rows, int* samples, hipStream_t s)
{
    hipLaunchKernelGGL(paste_area_prepare_kernel, dim3((unsigned)((N + PASTE_PREPARE_BLOCK - 1) / PASTE_PREPARE_BLOCK)), dim3(PASTE_PREPARE_BLOCK),
                       0, s, faces, frame_of_row, frames, N, cw, ch, fitted ? 1 : 0, area, rows, area_rows, samples);
}

// (YUV is a choice of the NV12 launches alone: without NV12 frames there is no block path)
template <bool PLANAR, bool YUV>
static void launch_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const PasteRow* rows, const PasteAreaRow* area_rows, const int* list,
                         const int* entry_of_row, int N, const PasteCropDev& crop, hipStream_t s)
{
    const dim3 grid((unsigned)N, (unsigned)paste_groups(crop)), block(PASTE_BLOCK);
    if (chroma && area_rows)
        hipLaunchKernelGGL((paste_kernel_t<true, true, PLANAR, YUV>), grid, block, 0, s, frames, chroma, rows, area_rows, list, entry_of_row, crop);
    else if (chroma)
        hipLaunchKernelGGL((paste_kernel_t<true, false, PLANAR, YUV>), grid, block, 0, s, frames, chroma, rows, area_rows, list, entry_of_row, crop);
    else if (area_rows)
        hipLaunchKernelGGL((paste_kernel_t<false, true, PLANAR, false>), grid, block, 0, s, frames, PasteNone{}, rows, area_rows, list, entry_of_row, crop);
    else
        hipLaunchKernelGGL((paste_kernel_t<false, false, PLANAR, false>), grid, block, 0, s, frames, PasteNone{}, rows, PasteNone{}, list, entry_of_row, crop);
}

void sdm_launch_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const PasteRow* rows, const PasteAreaRow* area_rows, const int* list,
                      const int* entry_of_row, int N, const PasteCropDev& crop, bool planar, bool yuv, hipStream_t s)
{
    if (planar && yuv) launch_paste<true, true>(frames, chroma, rows, area_rows, list, entry_of_row, N, crop, s);
    else if (planar) launch_paste<true, false>(frames, chroma, rows, area_rows, list, entry_of_row, N, crop, s);
    else if (yuv) launch_paste<false, true>(frames, chroma, rows, area_rows, list, entry_of_row, N, crop, s);
    else launch_paste<false, false>(frames, chroma, rows, area_rows, list, entry_of_row, N, crop, s);
}
