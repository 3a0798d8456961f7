// sdm_warp_paste.hip -- warped face tensors pasted back into frames on gfx950 (include/sdm.h, "Pasting warped faces back", "... into NV12
// frames", "..., filtered"), behind warp_fit_kernel of csrc/sdm_warp.hip.
//
//   warp_paste_prepare_kernel   one wave per row, one lane per triangle (T > 64: in turns), as warp_fit_kernel: the lanes first look at
//                          the mesh's K landmarks -- DEGENERATE, PARTIAL against the destination frame, the extremes, reduced across the
//                          wave into the row's box --, then every lane turns its triangle's A_t into one WarpPasteTri record in device
//                          memory: W_t, the corners in edge-function order, the triangle's box, the "covers nothing" bit.  FOLDED is the
//                          bit warp_fit_kernel left in the row's record; lane 0 writes the row's record: nothing is atomic, nothing
//                          depends on an execution order.
//   warp_paste_area_counts_kernel   the filtered calls' stage behind it.  One thread per (row, triangle): (Sx, Sy) from the record's W_t
//                          and the row's flags, packed into two bytes in an array of its own beside the records -- WarpPasteTri is
//                          staged whole in LDS and keeps its 68 bytes -- and as two ints for the host.
//   warp_paste_kernel_t<NV12, AREA>   the paste, one text for its three instantiations: <false, false> the calls whose frames are never
//                          NV12, <true, false> the calls that take NV12 destinations, <true, true> the filtered calls.  Grid and tile
//                          walk are csrc/sdm_paste.h's.  The row's T records are staged in LDS once per workgroup (68 bytes each:
//                          17 272 bytes at T = 254), AREA: with its T packed counts behind them (508 bytes more).
//                          A frame that is not NV12 -- the format is uniform for a workgroup, so that a mixed list costs one launch --
//                          is walked per pixel.  Per tile a wave culls: lane l tests the boxes of triangles l, l + 64, ... against the
//                          wave's strip of pixels, four ballots give the candidate set in scalar registers, and every lane walks the
//                          set bits in ascending order up to the first triangle that holds its pixel -- by warp_paste_inside, which
//                          tests the pixel against the triangle's box itself, so the strip cull only leaves out triangles that the
//                          pixel's own test refuses, and this walk and the ownership path's (warp_paste_footprint) decide every pixel
//                          alike.  The ownership test against earlier rows of the frame and the application of later rows read those
//                          rows' records from device memory, the row box first (paste_owned).  One owner per pixel, no atomics, one pass.
//                          On an NV12 frame the tile walk runs over the 2 x 2 blocks of the row's box widened to even coordinates; a
//                          lane owns block (BX, BY), a wave covers 64 blocks of one block row, a strip of 128 x 2 luma pixels.  The
//                          cull is taken once per wave against that strip as it is: every triangle's box lies inside the row's box, so
//                          a triangle left out is one whose own box test refuses every pixel of the strip.  Every lane then walks the
//                          candidates in ascending order and tests the up-to-four pixels of its block that are still looking (those
//                          inside the row's box), until no lane has one: the four winners, 255 for none, pack into one register.  The
//                          block rule is paste_owned_block on the shape PasteMeshOwn, which answers for the owner's row from the
//                          winners and the staged records and for every other row through warp_paste_footprint: every byte of both
//                          planes has at most one reader and writer in the launch.
//                          AREA changes what a row contributes to a pixel it holds (paste_taps of PasteMeshAreaOwn), never which
//                          pixels it holds: the footprint and the ownership rule are the unfiltered ones.  The owner answers from
//                          LDS; every other row of the frame reads its records and counts from device memory.  A pixel whose triangle
//                          has (1, 1) runs paste_sample_taps, any other the Sx x Sy loops through its own W_t: lanes of a wave run
//                          loops of different counts, which is accepted here as it is for the filtered warp.
//
// The staging, the cull and the walk exist once.  They are shared as a kernel template, not through a __forceinline__ function: that
// was tried four ways and moved the unfiltered kernel's instructions each time, where the three instantiations
// are the three earlier kernels' instructions (profiles/paste_template_isa_identity.txt).
//
// The per-pixel arithmetic is csrc/sdm_warp_paste_area_device.h on top of csrc/sdm_warp_paste_device.h and csrc/sdm_paste_device.h.
#include "sdm_paste.h"
#include "sdm_warp_paste_area_device.h"

#pragma clang fp contract(off)

namespace {

#define WPASTE_PREPARE_BLOCK 256      // four rows per workgroup
#define WPASTE_COUNTS_BLOCK 256
#define WPASTE_WORDS ((SDM_WARP_MAX_TRIANGLES + 63) / 64)
#define WPASTE_REC_INTS ((int)(sizeof(WarpPasteTri) / sizeof(int)))

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(WPASTE_PREPARE_BLOCK) void warp_paste_prepare_kernel(const float* __restrict__ x, int N, int L,
                                                                                  const int* __restrict__ lm, int K,
                                                                                  const WarpTri* __restrict__ tri, int T,
                                                                                  const WarpFace* __restrict__ faces,
                                                                                  const float* __restrict__ matrices,
                                                                                  const int* __restrict__ frame_of_row,
                                                                                  const PasteFrameDev* __restrict__ frames,
                                                                                  WarpPasteRow* __restrict__ rows, WarpPasteTri* __restrict__ tris)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (WPASTE_PREPARE_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= N) return;                                             // (the whole wave)
    const float* xr = x + (long long)r * 2 * L;
    const int fi = frame_of_row[r];
    const int fw = frames[fi].w, fh = frames[fi].h;
    WarpPasteScan s;
    warp_paste_scan_init(s);
    for (int k = lane; k < K; k += 64) warp_paste_scan_point(xr[lm[k]], xr[L + lm[k]], fw, fh, s);
    s.bad = __ballot(s.bad) != 0;
    s.outside = __ballot(s.outside) != 0;
    // (a NaN among the landmarks: s.bad, and the extremes are not read)
    s.xlo = wave_min(s.xlo); s.xhi = wave_max(s.xhi); s.ylo = wave_min(s.ylo); s.yhi = wave_max(s.yhi);
    // FOLDED is the fit's own answer (warp_fit_triangle, ORed over the row by warp_fit_kernel); its PARTIAL is the source's, not read
    WarpPasteRow row;
    warp_paste_row(s, (faces[r].flags & SDM_WARP_FOLDED) != 0, fi, fw, fh, row);
    const float* mrow = matrices + (long long)r * T * 6;
    WarpPasteTri* trow = tris + (long long)r * T;
    for (int t = lane; t < T; t += 64) {
        const WarpTri tr = tri[t];
        const float pa[2] = {xr[tr.ia], xr[L + tr.ia]}, pb[2] = {xr[tr.ib], xr[L + tr.ib]}, pc[2] = {xr[tr.ic], xr[L + tr.ic]};
        float m[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) m[e] = mrow[6 * t + e];
        WarpPasteTri rec;
        warp_paste_triangle(m, pa, pb, pc, row.x0, row.y0, row.x1, row.y1, rec);
        trow[t] = rec;
    }
    if (lane == 0) rows[r] = row;
}

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

// (the PasteMesh is built where it is used: a named one ahead of the walk renumbers registers in <false, false>)
// PLANAR: the frame list holds a planar colour frame (paste_kernel_t's rule, csrc/sdm_align_paste.hip)
// YUV: an NV12 frame of the list carries a colour description -- the block path takes its constants from the frame's table row
// (csrc/sdm_yuv_device.h); lists of value 5 alone run the text they always ran
template <bool NV12, bool AREA, bool PLANAR, bool YUV>
__global__ __launch_bounds__(PASTE_BLOCK) void warp_paste_kernel_t(const PasteFrameDev* __restrict__ frames,
                                                                    PasteOpt<NV12, uint8_t* const* __restrict__> chroma,
                                                                    const WarpPasteRow* __restrict__ rows, const WarpPasteTri* __restrict__ tris,
                                                                    PasteOpt<AREA, const WarpPasteCounts* __restrict__> counts, int T,
                                                                    const int* __restrict__ list, const int* __restrict__ entry_of_row,
                                                                    const uint8_t* __restrict__ labels, PasteCropDev c)
{
    __shared__ WarpPasteTri lds[SDM_WARP_MAX_TRIANGLES];
    __shared__ WarpPasteCounts lds_counts[AREA ? SDM_WARP_MAX_TRIANGLES : 1];
    // the row, its list entry and its frame: uniform for the workgroup
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
        if constexpr (AREA)
            for (int e = threadIdx.x; e < T; e += PASTE_BLOCK) lds_counts[e] = counts[(long long)n * T + e];
    }
    __syncthreads();
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    if (!NV12 || (YUV ? SDM_FRAME_BASE(f.format) : f.format) != SDM_FRAME_NV12) {
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
                if constexpr (AREA) {
                    PasteMeshAreaOwn own{PasteMeshArea{PasteMesh{rows, tris, T, labels}, counts, -1}, n, 0xffffffffu, lds, lds_counts};
                    own.area.tri = mine;
                    paste_owned<PLANAR>(f, own, list, k, c, X, Y, q);
                } else {
                    paste_owned<PLANAR>(f, PasteMesh{rows, tris, T, labels}, list, k, c, X, Y, q);
                }
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
            if (winners != 0xffffffffu) {
                if constexpr (AREA)
                    paste_owned_block<YUV>(f, uv, PasteMeshAreaOwn{PasteMeshArea{PasteMesh{rows, tris, T, labels}, counts, -1}, n, winners, lds, lds_counts},
                                      list, k, c, BX, BY);
                else
                    paste_owned_block<YUV>(f, uv, PasteMeshOwn{PasteMesh{rows, tris, T, labels}, n, winners, lds}, list, k, c, BX, BY);
            }
        }
    }
}

}  // namespace

void sdm_launch_warp_paste_prepare(const float* x, int N, int L, const int* lm, int K, const WarpTri* tri, int T, const WarpFace* faces,
                                   const float* matrices, const int* frame_of_row, const PasteFrameDev* frames, WarpPasteRow* rows,
                                   WarpPasteTri* tris, hipStream_t s)
{
    const int per = WPASTE_PREPARE_BLOCK / 64;
    hipLaunchKernelGGL(warp_paste_prepare_kernel, dim3((unsigned)((N + per - 1) / per)), dim3(WPASTE_PREPARE_BLOCK), 0, s, x, N, L, lm, K, tri, T,
                       faces, matrices, frame_of_row, frames, rows, tris);
}

void sdm_launch_warp_paste_area_counts(const WarpPasteRow* rows, const WarpPasteTri* tris, int N, int T, const AlignAreaDev& area,
                                       uint16_t* counts, int* samples, hipStream_t s)
{
    const long long total = (long long)N * T;
    hipLaunchKernelGGL(warp_paste_area_counts_kernel, dim3((unsigned)((total + WPASTE_COUNTS_BLOCK - 1) / WPASTE_COUNTS_BLOCK)),
                       dim3(WPASTE_COUNTS_BLOCK), 0, s, rows, tris, N, T, area, counts, samples);
}

template <bool PLANAR, bool YUV>
static void launch_warp_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const WarpPasteRow* rows, const WarpPasteTri* tris,
                              const uint16_t* counts, int T, const int* list, const int* entry_of_row, int N, const uint8_t* labels,
                              const PasteCropDev& crop, hipStream_t s)
{
    const dim3 grid((unsigned)N, (unsigned)paste_groups(crop)), block(PASTE_BLOCK);
    if (counts)
        hipLaunchKernelGGL((warp_paste_kernel_t<true, true, PLANAR, YUV>), grid, block, 0, s, frames, chroma, rows, tris, counts, T, list, entry_of_row, labels, crop);
    else if (chroma)
        hipLaunchKernelGGL((warp_paste_kernel_t<true, false, PLANAR, YUV>), grid, block, 0, s, frames, chroma, rows, tris, PasteNone{}, T, list, entry_of_row,
                           labels, crop);
    else
        hipLaunchKernelGGL((warp_paste_kernel_t<false, false, PLANAR, false>), grid, block, 0, s, frames, PasteNone{}, rows, tris, PasteNone{}, T, list,
                           entry_of_row, labels, crop);
}

void sdm_launch_warp_paste(const PasteFrameDev* frames, uint8_t* const* chroma, const WarpPasteRow* rows, const WarpPasteTri* tris,
                           const uint16_t* counts, int T, const int* list, const int* entry_of_row, int N, const uint8_t* labels,
                           const PasteCropDev& crop, bool planar, bool yuv, hipStream_t s)
{
    if (planar && yuv) launch_warp_paste<true, true>(frames, chroma, rows, tris, counts, T, list, entry_of_row, N, labels, crop, s);
    else if (planar) launch_warp_paste<true, false>(frames, chroma, rows, tris, counts, T, list, entry_of_row, N, labels, crop, s);
    else if (yuv) launch_warp_paste<false, true>(frames, chroma, rows, tris, counts, T, list, entry_of_row, N, labels, crop, s);
    else launch_warp_paste<false, false>(frames, chroma, rows, tris, counts, T, list, entry_of_row, N, labels, crop, s);
}
