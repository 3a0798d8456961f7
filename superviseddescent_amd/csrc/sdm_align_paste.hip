// sdm_align_paste.hip -- crop tensors pasted back into frames on gfx950 (include/sdm.h, "Pasting crops back"), behind the fit of
// sdm_align_crops or a caller's matrices.
//
//   paste_prepare_kernel   one lane per row: the inverse map W (double, rounded once to float32), the flags and the footprint's box in
//                          the row's frame, written as one PasteRow record; the final flags go back into the fit's record
//   paste_kernel           the tile walk of csrc/sdm_paste.h over the row's box.  A lane's pixel is pasted by the lowest-numbered row
//                          of the frame whose footprint holds it (paste_pixel, paste_owned): every frame byte has at most one reader
//                          and writer in the launch, whatever the order the workgroups run in.  Stores are per pixel, byte by byte:
//                          nothing a neighbour owns is touched.
//
//   paste_area_prepare_kernel, paste_area_kernel   the filtered calls' pair: the prepare stage also leaves S and the working footprint
//                          of every row (PasteAreaRow); the paste is the same tile walk and the same ownership rule on the shape
//                          PasteRigidArea.  S is uniform for a workgroup (one row) and, in the owner loop, per list entry: every
//                          sub-sample loop has a wave-uniform trip count.  Rows with S = 1 take paste_kernel's per-pixel code.
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

__global__ __launch_bounds__(PASTE_BLOCK) void paste_kernel(const PasteFrameDev* __restrict__ frames, const PasteRow* __restrict__ rows,
                                                            const int* __restrict__ list, const int* __restrict__ entry_of_row, PasteCropDev c)
{
    // the row, its list entry and its frame: uniform for the workgroup
    const int n = blockIdx.x;
    const int k = entry_of_row[n];
    const PasteRow r = rows[n];
    const int bw = r.x1 - r.x0, bh = r.y1 - r.y0;
    if (bw <= 0 || bh <= 0) return;
    const PasteFrameDev f = frames[r.frame];
    const int tx = paste_tiles_x(bw), ty = paste_tiles_y(bh);
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
        const int X = r.x0 + paste_tile_x(t, tx) + lx, Y = r.y0 + paste_tile_y(t, tx) + ly;
        if (X < r.x1 && Y < r.y1) paste_pixel(f, rows, list, k, c, X, Y);
    }
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

__global__ __launch_bounds__(PASTE_BLOCK) void paste_area_kernel(const PasteFrameDev* __restrict__ frames, const PasteRow* __restrict__ rows,
                                                                 const PasteAreaRow* __restrict__ area_rows, const int* __restrict__ list,
                                                                 const int* __restrict__ entry_of_row, PasteCropDev c)
{
    const int n = blockIdx.x;
    const int k = entry_of_row[n];
    const PasteRow r = rows[n];
    const int bw = r.x1 - r.x0, bh = r.y1 - r.y0;
    if (bw <= 0 || bh <= 0) return;
    const PasteFrameDev f = frames[r.frame];
    const int tx = paste_tiles_x(bw), ty = paste_tiles_y(bh);
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
        const int X = r.x0 + paste_tile_x(t, tx) + lx, Y = r.y0 + paste_tile_y(t, tx) + ly;
        if (X < r.x1 && Y < r.y1) paste_area_pixel(f, rows, area_rows, list, k, c, X, Y);
    }
}

}  // namespace

void sdm_launch_paste_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                              PasteRow* rows, hipStream_t s)
{
    hipLaunchKernelGGL(paste_prepare_kernel, dim3((unsigned)((N + PASTE_PREPARE_BLOCK - 1) / PASTE_PREPARE_BLOCK)), dim3(PASTE_PREPARE_BLOCK), 0, s,
                       faces, frame_of_row, frames, N, cw, ch, fitted ? 1 : 0, rows);
}

void sdm_launch_paste(const PasteFrameDev* frames, const PasteRow* rows, const int* list, const int* entry_of_row, int N,
                      const PasteCropDev& crop, hipStream_t s)
{
    hipLaunchKernelGGL(paste_kernel, dim3((unsigned)N, (unsigned)paste_groups(crop)), dim3(PASTE_BLOCK), 0, s, frames, rows, list, entry_of_row,
                       crop);
}

void sdm_launch_paste_area_prepare(AlignFace* faces, const int* frame_of_row, const PasteFrameDev* frames, int N, int cw, int ch, bool fitted,
                                   const AlignAreaDev& area, PasteRow* rows, PasteAreaRow* area_rows, int* samples, hipStream_t s)
{
    hipLaunchKernelGGL(paste_area_prepare_kernel, dim3((unsigned)((N + PASTE_PREPARE_BLOCK - 1) / PASTE_PREPARE_BLOCK)), dim3(PASTE_PREPARE_BLOCK),
                       0, s, faces, frame_of_row, frames, N, cw, ch, fitted ? 1 : 0, area, rows, area_rows, samples);
}

void sdm_launch_paste_area(const PasteFrameDev* frames, const PasteRow* rows, const PasteAreaRow* area_rows, const int* list,
                           const int* entry_of_row, int N, const PasteCropDev& crop, hipStream_t s)
{
    hipLaunchKernelGGL(paste_area_kernel, dim3((unsigned)N, (unsigned)paste_groups(crop)), dim3(PASTE_BLOCK), 0, s, frames, rows, area_rows, list,
                       entry_of_row, crop);
}
