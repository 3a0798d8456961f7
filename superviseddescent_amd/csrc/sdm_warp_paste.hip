// sdm_warp_paste.hip -- warped face tensors pasted back into frames on gfx950 (include/sdm.h, "Pasting warped faces back"), behind
// warp_fit_kernel of csrc/sdm_warp.hip.
//
//   warp_paste_prepare_kernel   one wave per row, one lane per triangle (T > 64: in turns), as warp_fit_kernel: the lanes first look at
//                          the mesh's K landmarks -- DEGENERATE, PARTIAL against the destination frame, the extremes, reduced across the
//                          wave into the row's box --, then every lane turns its triangle's A_t into one WarpPasteTri record in device
//                          memory: W_t, the corners in edge-function order, the triangle's box, the "covers nothing" bit.  FOLDED is the
//                          bit warp_fit_kernel left in the row's record; lane 0 writes the row's record: nothing is atomic, nothing
//                          depends on an execution order.
//   warp_paste_kernel      the tile walk of csrc/sdm_paste.h over the row's box.  The row's T records are staged in LDS once per
//                          workgroup (68 bytes each: 17 272 bytes at T = 254).  Per tile a wave culls: lane l tests the boxes of
//                          triangles l, l + 64, ... against the wave's strip of pixels, four ballots give the candidate set in scalar
//                          registers, and every lane walks the set bits in ascending order up to the first triangle that holds its
//                          pixel -- by warp_paste_inside, which tests the pixel against the triangle's box itself, so the strip cull
//                          only leaves out triangles that the pixel's own test refuses, and this walk and the ownership path's
//                          (warp_paste_footprint) decide every pixel alike.  The ownership
//                          test against earlier rows of the frame and the application of later rows read those rows' records from
//                          device memory, the row box first (paste_owned).  One owner per pixel, no atomics, one pass.
//   warp_paste_nv12_kernel   the calls that take NV12 destinations (include/sdm.h, "Pasting warped faces back into NV12 frames"), behind
//                          the same two kernels.  The frame's format is uniform for a workgroup: any other frame takes
//                          warp_paste_kernel's per-pixel body, so that a mixed list costs one launch.  On an NV12 frame the tile walk
//                          runs over the 2 x 2 blocks of the row's box widened to even coordinates; a wave covers 64 blocks of one block
//                          row, a strip of 128 x 2 luma pixels.  The cull is taken once per wave against that strip; every lane then
//                          walks the candidates in ascending order and tests the up-to-four pixels of its block that are still looking
//                          (those inside the row's box), until no lane has one: the four winners, 255 for none, pack into one
//                          register.  The block rule is paste_owned_block on the shape PasteMeshOwn, which answers for the owner's row
//                          from the winners and the staged records and for every other row through warp_paste_footprint: every byte
//                          of both planes has at most one reader and writer in the launch.
//
// The per-pixel arithmetic is csrc/sdm_warp_paste_device.h on top of csrc/sdm_paste_device.h.
#include "sdm_paste.h"

#pragma clang fp contract(off)

namespace {

#define WPASTE_PREPARE_BLOCK 256      // four rows per workgroup
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

__global__ __launch_bounds__(PASTE_BLOCK) void warp_paste_kernel(const PasteFrameDev* __restrict__ frames, const WarpPasteRow* __restrict__ rows,
                                                                  const WarpPasteTri* __restrict__ tris, int T, const int* __restrict__ list,
                                                                  const int* __restrict__ entry_of_row, const uint8_t* __restrict__ labels,
                                                                  PasteCropDev c)
{
    __shared__ WarpPasteTri lds[SDM_WARP_MAX_TRIANGLES];
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
    }
    __syncthreads();
    const int tx = paste_tiles_x(bw), ty = paste_tiles_y(bh);
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
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
        if (mine >= 0 && paste_position(lds[mine].w, c.cw, c.ch, X, Y, q)) paste_owned(f, PasteMesh{rows, tris, T, labels}, list, k, c, X, Y, q);
    }
}

// The calls that take NV12 destinations.  The non-NV12 branch is warp_paste_kernel's body, text for text: a copy, to be kept in step
// by hand.  Sharing it through a __forceinline__ function was tried three ways (the staged records as a pointer, as an array
// reference, the parameters without __restrict__) and each moved warp_paste_kernel's instructions (scripts/isa_kernel_identity.py:
// 2 826 lines of text became 2 868, 2 868 and 2 873), which that kernel's record does not allow.  On an NV12 frame a lane owns block (BX, BY) of the row's box widened to even coordinates; a wave's
// 64 blocks are a strip of 128 x 2 luma pixels.  The strip cull tests the triangles' boxes against that strip as it is: every
// triangle's box lies inside the row's box, so a triangle left out is one whose own box test refuses every pixel of the strip.
__global__ __launch_bounds__(PASTE_BLOCK) void warp_paste_nv12_kernel(const PasteFrameDev* __restrict__ frames, uint8_t* const* __restrict__ chroma,
                                                                       const WarpPasteRow* __restrict__ rows, const WarpPasteTri* __restrict__ tris,
                                                                       int T, const int* __restrict__ list, const int* __restrict__ entry_of_row,
                                                                       const uint8_t* __restrict__ labels, PasteCropDev c)
{
    __shared__ WarpPasteTri lds[SDM_WARP_MAX_TRIANGLES];
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
    }
    __syncthreads();
    const int lx = threadIdx.x & (PASTE_TILE_W - 1), ly = threadIdx.x / PASTE_TILE_W;
    if (f.format != SDM_FRAME_NV12) {
        const int tx = paste_tiles_x(bw), ty = paste_tiles_y(bh);
        for (long long t = blockIdx.y; t < (long long)tx * ty; t += gridDim.y) {
            const int X0 = r.x0 + paste_tile_x(t, tx), Y = r.y0 + paste_tile_y(t, tx) + ly;
            if (Y >= r.y1) continue;                                    // (the whole wave)
            const int X = X0 + lx, X1 = X0 + PASTE_TILE_W < r.x1 ? X0 + PASTE_TILE_W : r.x1;
            unsigned long long cand[WPASTE_WORDS];
#pragma unroll
            for (int w = 0; w < WPASTE_WORDS; ++w) {
                const int tt = w * 64 + lx;
                cand[w] = __ballot(tt < T && warp_paste_hits(lds[tt < T ? tt : 0], X0, Y, X1, Y + 1));
            }
            int mine = -1;
            bool open = X < r.x1;
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
            if (mine >= 0 && paste_position(lds[mine].w, c.cw, c.ch, X, Y, q)) paste_owned(f, PasteMesh{rows, tris, T, labels}, list, k, c, X, Y, q);
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
        if (winners != 0xffffffffu)
            paste_owned_block(f, uv, PasteMeshOwn{PasteMesh{rows, tris, T, labels}, n, winners, lds}, list, k, c, BX, BY);
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

void sdm_launch_warp_paste(const PasteFrameDev* frames, const WarpPasteRow* rows, const WarpPasteTri* tris, int T, const int* list,
                           const int* entry_of_row, int N, const uint8_t* labels, const PasteCropDev& crop, hipStream_t s)
{
    hipLaunchKernelGGL(warp_paste_kernel, dim3((unsigned)N, (unsigned)paste_groups(crop)), dim3(PASTE_BLOCK), 0, s, frames, rows, tris, T, list,
                       entry_of_row, labels, crop);
}

void sdm_launch_warp_paste_nv12(const PasteFrameDev* frames, uint8_t* const* chroma, const WarpPasteRow* rows, const WarpPasteTri* tris, int T,
                                const int* list, const int* entry_of_row, int N, const uint8_t* labels, const PasteCropDev& crop, hipStream_t s)
{
    hipLaunchKernelGGL(warp_paste_nv12_kernel, dim3((unsigned)N, (unsigned)paste_groups(crop)), dim3(PASTE_BLOCK), 0, s, frames, chroma, rows, tris,
                       T, list, entry_of_row, labels, crop);
}
