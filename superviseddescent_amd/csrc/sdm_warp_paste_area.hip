// sdm_warp_paste_area.hip -- the filtered piecewise-affine paste on gfx950 (include/sdm.h, "Pasting warped faces back, filtered"), behind
// warp_fit_kernel of csrc/sdm_warp.hip and warp_paste_prepare_kernel of csrc/sdm_warp_paste.hip, which stays as it is.
//
//   warp_paste_area_counts_kernel   one thread per (row, triangle): (Sx, Sy) from the record's W_t and the row's flags, packed into two
//                          bytes in an array of its own beside the records -- WarpPasteTri is staged whole in LDS by the unfiltered
//                          kernels and keeps its 68 bytes -- and as two ints for the host.
//   warp_paste_area_kernel warp_paste_nv12_kernel's structure: the frame's format is uniform for a workgroup, the row's T records are
//                          staged in LDS once (17 272 bytes at T = 254) with its T packed counts behind them (508 bytes more), the
//                          tile walk of csrc/sdm_paste.h, the strip cull by four ballots, the ascending walk over the candidates,
//                          2 x 2 blocks on an NV12 frame.  The footprint and the ownership rule are the unfiltered ones: the filter
//                          changes what a row contributes to a pixel it holds (paste_taps of PasteMeshAreaOwn), never which pixels it
//                          holds.  The owner answers from LDS; every other row of the frame reads its records and counts from device
//                          memory.  A pixel whose triangle has (1, 1) runs paste_sample_taps, any other the Sx x Sy loops through its
//                          own W_t: lanes of a wave run loops of different counts, which is accepted here as it is for the filtered
//                          warp.
//
// The tile walk, the strip cull and the candidate walk of both branches are warp_paste_nv12_kernel's, text for text, and its per-pixel
// branch is in turn warp_paste_kernel's (csrc/sdm_warp_paste.hip): a third copy, to be kept in step with the other two BY HAND.  The copy
// is deliberate: those two kernels are pinned instruction for instruction (profiles/warp_paste_area_isa_identity.txt), and sharing the
// walk through a function moved their instructions when it was tried (the note above warp_paste_nv12_kernel).  A fix to the cull or to
// the walk has to reach all three kernels.
//
// The per-pixel arithmetic is csrc/sdm_warp_paste_area_device.h on top of csrc/sdm_warp_paste_device.h.
#include "sdm_paste.h"
#include "sdm_warp_paste_area_device.h"

#pragma clang fp contract(off)

namespace {

#define WPASTE_WORDS ((SDM_WARP_MAX_TRIANGLES + 63) / 64)
#define WPASTE_REC_INTS ((int)(sizeof(WarpPasteTri) / sizeof(int)))
#define WPASTE_COUNTS_BLOCK 256

__global__ __launch_bounds__(WPASTE_COUNTS_BLOCK) void warp_paste_area_counts_kernel(const WarpPasteRow* __restrict__ rows,
                                                                                     const WarpPasteTri* __restrict__ tris, int N, int T,
                                                                                     AlignAreaDev area, WarpPasteCounts* __restrict__ counts,
                                                                                     int* __restrict__ samples)
{
    const long long e = (long long)blockIdx.x * WPASTE_COUNTS_BLOCK + threadIdx.x;
    if (e >= (long long)N * T) return;
    const WarpPasteCounts cnt = warp_paste_area_counts(tris[e], rows[e / T].flags, area.mode, area.max_samples, area.min2);
    counts[e] = cnt;
    samples[2 * e] = cnt & 255;
    samples[2 * e + 1] = cnt >> 8;
}

__global__ __launch_bounds__(PASTE_BLOCK) void warp_paste_area_kernel(const PasteFrameDev* __restrict__ frames, uint8_t* const* __restrict__ chroma,
                                                                       const WarpPasteRow* __restrict__ rows, const WarpPasteTri* __restrict__ tris,
                                                                       const WarpPasteCounts* __restrict__ counts, int T,
                                                                       const int* __restrict__ list, const int* __restrict__ entry_of_row,
                                                                       const uint8_t* __restrict__ labels, PasteCropDev c)
{
    __shared__ WarpPasteTri lds[SDM_WARP_MAX_TRIANGLES];
    __shared__ WarpPasteCounts lds_counts[SDM_WARP_MAX_TRIANGLES];
    const int n = blockIdx.x;
    const int k = entry_of_row[n];
    const WarpPasteRow r = rows[n];
    const int bw = r.x1 - r.x0, bh = r.y1 - r.y0;
    if (bw <= 0 || bh <= 0) return;
    const PasteFrameDev f = frames[r.frame];
    {
        const int* src = (const int*)(tris + (long long)n * T);
        int* dst = (int*)lds;
        for (int e = threadIdx.x; e < T * WPASTE_REC_INTS; e += PASTE_BLOCK) dst[e] = src[e];
        for (int e = threadIdx.x; e < T; e += PASTE_BLOCK) lds_counts[e] = counts[(long long)n * T + e];
    }
    __syncthreads();
    const PasteMeshArea shape{PasteMesh{rows, tris, T, labels}, counts, -1};
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    if (f.format != SDM_FRAME_NV12) {
        const int tx = paste_tiles_x(bw), ty = paste_tiles_y(bh);
        for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
            const int X0 = r.x0 + paste_tile_x(t, tx), Y = r.y0 + paste_tile_y(t, tx) + ly;
            if (Y >= r.y1) continue;                                    // (the whole wave)
            const int X = X0 + lx, X1 = X0 + PASTE_TILE_W < r.x1 ? X0 + PASTE_TILE_W : r.x1;
            // the wave's candidates: triangles whose box meets its strip of pixels
            unsigned long long cand[WPASTE_WORDS];
#pragma unroll
            for (int w = 0; w < WPASTE_WORDS; ++w) {
                const int tt = w * 64 + lx;
                cand[w] = __ballot(tt < T && warp_paste_hits(lds[tt < T ? tt : 0], X0, Y, X1, Y + 1));
            }
            int mine = -1;
            bool open = X < r.x1;                                       // still looking
#pragma unroll
            for (int w = 0; w < WPASTE_WORDS; ++w) {
                unsigned long long m = cand[w];
                while (m != 0ull && __ballot(open) != 0ull) {
                    const int tt = w * 64 + __builtin_ctzll(m);
                    m &= m - 1ull;
                    if (open && warp_paste_inside(lds[tt], X, Y)) { mine = tt; open = false; }
                }
            }
            AlignPos q;
            if (mine >= 0 && paste_position(lds[mine].w, c.cw, c.ch, X, Y, q)) {
                PasteMeshAreaOwn own{shape, n, 0xffffffffu, lds, lds_counts};
                own.area.tri = mine;
                paste_owned(f, own, list, k, c, X, Y, q);
            }
        }
        return;
    }
    // the blocks of the box widened to even coordinates: [bx0, bx1) x [by0, by1)
    uint8_t* const uv = chroma[r.frame];
    const int bx0 = r.x0 >> 1, by0 = r.y0 >> 1, bx1 = (r.x1 + 1) >> 1, by1 = (r.y1 + 1) >> 1;
    const int tx = paste_tiles_x(bx1 - bx0), ty = paste_tiles_y(by1 - by0);
    for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
        const int B0 = bx0 + paste_tile_x(t, tx), BY = by0 + paste_tile_y(t, tx) + ly;
        if (BY >= by1) continue;                                        // (the whole wave)
        const int BX = B0 + lx;
        // the wave's candidates: triangles whose box meets its strip of 128 x 2 pixels
        unsigned long long cand[WPASTE_WORDS];
#pragma unroll
        for (int w = 0; w < WPASTE_WORDS; ++w) {
            const int tt = w * 64 + lx;
            cand[w] = __ballot(tt < T && warp_paste_hits(lds[tt < T ? tt : 0], 2 * B0, 2 * BY, 2 * B0 + 2 * PASTE_TILE_W, 2 * BY + 2));
        }
        // the block's pixels inside the row's box (hence inside the frame) are still looking, bit i for pixel i
        int open = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int X = 2 * BX + (i & 1), Y = 2 * BY + (i >> 1);
            if (X >= r.x0 && X < r.x1 && Y >= r.y0 && Y < r.y1) open |= 1 << i;
        }
        uint32_t winners = 0xffffffffu;
#pragma unroll
        for (int w = 0; w < WPASTE_WORDS; ++w) {
            unsigned long long m = cand[w];
            while (m != 0ull && __ballot(open != 0) != 0ull) {
                const int tt = w * 64 + __builtin_ctzll(m);
                m &= m - 1ull;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((open >> i & 1) && warp_paste_inside(lds[tt], 2 * BX + (i & 1), 2 * BY + (i >> 1))) {
                        winners = (winners & ~(255u << (8 * i))) | (uint32_t)tt << (8 * i);
                        open &= ~(1 << i);
                    }
            }
        }
        // (a lane whose block the row does not hold -- beyond bx1 too: nothing was open -- leaves before any ownership test)
        if (winners != 0xffffffffu) paste_owned_block(f, uv, PasteMeshAreaOwn{shape, n, winners, lds, lds_counts}, list, k, c, BX, BY);
    }
}

}  // namespace

void sdm_launch_warp_paste_area_counts(const WarpPasteRow* rows, const WarpPasteTri* tris, int N, int T, const AlignAreaDev& area,
                                       uint16_t* counts, int* samples, hipStream_t s)
{
    const long long total = (long long)N * T;
    hipLaunchKernelGGL(warp_paste_area_counts_kernel, dim3((unsigned)((total + WPASTE_COUNTS_BLOCK - 1) / WPASTE_COUNTS_BLOCK)),
                       dim3(WPASTE_COUNTS_BLOCK), 0, s, rows, tris, N, T, area, counts, samples);
}

void sdm_launch_warp_paste_area(const PasteFrameDev* frames, uint8_t* const* chroma, const WarpPasteRow* rows, const WarpPasteTri* tris,
                                const uint16_t* counts, int T, const int* list, const int* entry_of_row, int N, const uint8_t* labels,
                                const PasteCropDev& crop, hipStream_t s)
{
    hipLaunchKernelGGL(warp_paste_area_kernel, dim3((unsigned)N, (unsigned)paste_groups(crop)), dim3(PASTE_BLOCK), 0, s, frames, chroma, rows, tris,
                       counts, T, list, entry_of_row, labels, crop);
}
