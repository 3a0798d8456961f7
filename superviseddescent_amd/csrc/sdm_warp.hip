// sdm_warp.hip -- piecewise-affine warped faces as a network's input tensor on gfx950 (include/sdm.h, "Warped faces",
// sdm_warp_crops_tensor): every triangle of the mesh carries its own crop -> source matrix, so every landmark lands on its template point.
//
//   warp_fit_kernel     one wave per row, one lane per triangle (T > 64: in turns): the lanes first look at the mesh's K landmarks --
//                       DEGENERATE, PARTIAL --, then every lane forms its triangle's matrix in double (warp_fit_triangle) and writes
//                       six floats of the N x T x 6 table; FOLDED and the other bits are ORed across the wave by ballot, and lane 0
//                       writes the row's record: the flag word does not depend on any execution order, nothing is atomic.
//   align_tensor_kernel<WarpMesh, DT, LAYOUT, CH>   the kernel frame of sdm_align_tensor_kernel.h: workgroups of face n (blockIdx.x), a lane
//                       owns 4 consecutive pixels of one crop row, the row's record or frame entry is read once per workgroup.  The
//                       workgroup first stages its face's T x 6 floats in LDS (records of 6 floats, at most 6 096 bytes), every lane
//                       in front of the barrier; a lane reads its 4 labels (one dword when the four lie in the crop row and the address
//                       is a multiple of 4, bytes otherwise) and fetches each pixel's matrix from LDS by its label -- neighbouring lanes
//                       mostly share a triangle, so most reads are broadcasts.  A pixel without a triangle reads no source byte.
//
// The frame (grid, row source, channel / element stage, stores, dispatch) is sdm_align_tensor_kernel.h; the per-pixel arithmetic is
// sdm_warp_device.h on top of align_fetch_segment of sdm_align_tensor_device.h (also compiled for the host by tests/cpp/warp_host.cpp).
#include "sdm_warp.h"
#include "sdm_align_tensor_kernel.h"

#pragma clang fp contract(off)

namespace {

#define WARP_FIT_BLOCK 256            // four rows per workgroup
#define WARP_LDS_REC 6                // floats per triangle in LDS

__global__ __launch_bounds__(WARP_FIT_BLOCK) void warp_fit_kernel(const float* __restrict__ x, int N, int L, const int* __restrict__ lm, int K,
                                                                  const WarpTri* __restrict__ tri, int T, AlignSourceDev src,
                                                                  const int* __restrict__ img_idx, WarpFace* __restrict__ faces,
                                                                  float* __restrict__ matrices)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (WARP_FIT_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= N) return;                                             // (the whole wave)
    const float* xr = x + (long long)r * 2 * L;
    // the row's image: an entry of the context's image set, or of the equally sized external stack
    WarpFace f;
    const int im = img_idx ? img_idx[r] : r;
    if (src.ctx.base) {
        f.off = src.ctx.offset[im]; f.w = src.ctx.w[im]; f.h = src.ctx.h[im]; f.stride = src.ctx.stride[im];
    } else {
        f.off = (long long)im * src.height * src.stride; f.w = src.width; f.h = src.height; f.stride = src.stride;
    }
    bool bad = false, outside = false;
    const float xmax = (float)(f.w - 1), ymax = (float)(f.h - 1);
    for (int k = lane; k < K; k += 64) {
        const float ax = xr[lm[k]], ay = xr[L + lm[k]];
        bad = bad || !(isfinite(ax) && isfinite(ay));
        outside = outside || !(ax >= 0.0f && ax <= xmax && ay >= 0.0f && ay <= ymax);
    }
    const bool degenerate = __ballot(bad) != 0;
    const bool partial = __ballot(outside) != 0;
    bool folded = false;
    float2* mrow = (float2*)(matrices + (long long)r * T * 6);      // (records of 24 bytes in an 8-byte aligned table)
    for (int t = lane; t < T; t += 64) {
        float m[6];
        if (degenerate) {
#pragma unroll
            for (int e = 0; e < 6; ++e) m[e] = __builtin_nanf("");
        } else {
            const WarpTri tr = tri[t];
            const float pa[2] = {xr[tr.ia], xr[L + tr.ia]}, pb[2] = {xr[tr.ib], xr[L + tr.ib]}, pc[2] = {xr[tr.ic], xr[L + tr.ic]};
            folded = warp_fit_triangle(tr, pa, pb, pc, m) || folded;
        }
        mrow[3 * t] = make_float2(m[0], m[1]); mrow[3 * t + 1] = make_float2(m[2], m[3]); mrow[3 * t + 2] = make_float2(m[4], m[5]);
    }
    const bool any_folded = __ballot(folded) != 0;
    if (lane == 0) {
        f.flags = degenerate ? SDM_WARP_DEGENERATE : (partial ? SDM_WARP_PARTIAL : 0) | (any_folded ? SDM_WARP_FOLDED : 0);
        faces[r] = f;
    }
}

struct WarpMesh {
    typedef WarpFace Face;
    struct Args { const float* matrices; int T; const uint8_t* labels; };
    const float* tm;
    // the face's matrices: T x 6 floats into LDS
    __device__ __forceinline__ void enter(const Args& a, const WarpFace&, int n, int)
    {
        __shared__ float lds[SDM_WARP_MAX_TRIANGLES * WARP_LDS_REC];
        const float* mrow = a.matrices + (long long)n * a.T * 6;
        for (int e = threadIdx.x; e < a.T * 6; e += ALIGN_T_BLOCK) {
            const int tt = e / 6;
            lds[tt * WARP_LDS_REC + (e - tt * 6)] = mrow[e];
        }
        __syncthreads();
        tm = lds;
    }
    template <bool WIDE>
    __device__ __forceinline__ void pixels(const Args& a, const WarpFace&, AlignRow& r, int i, int j0, int npx, int out_w, uint32_t px[4][3])
    {
        // the 4 labels (out_w * out_h <= 2^20)
        const int at = i * out_w + j0;
        uint32_t lab[4];
        if (npx == 4 && (at & 3) == 0) {
            const uint32_t v = *(const uint32_t*)(a.labels + at);
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = (v >> (8 * k)) & 255u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = k < npx ? (uint32_t)a.labels[at + k] : (uint32_t)SDM_WARP_NO_TRIANGLE;
        }
        float sx[4], sy[4];
        bool on[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            on[k] = lab[k] != SDM_WARP_NO_TRIANGLE;
            sx[k] = sy[k] = 0.0f;
            if (on[k]) {
                float m[6];
#pragma unroll
                for (int e = 0; e < 6; ++e) m[e] = tm[lab[k] * WARP_LDS_REC + e];
                warp_position(m, j0 + k, i, sx[k], sy[k]);
            }
        }
        align_fetch_segment<WIDE>(r, sx, sy, on, px);
    }
};

}  // namespace

void sdm_launch_warp_fit(const float* x, int N, int L, const int* lm, int K, const WarpTri* tri, int T, const AlignSourceDev& src,
                         const int* img_idx, WarpFace* faces, float* matrices, hipStream_t s)
{
    const int rows = WARP_FIT_BLOCK / 64;
    hipLaunchKernelGGL(warp_fit_kernel, dim3((unsigned)((N + rows - 1) / rows)), dim3(WARP_FIT_BLOCK), 0, s, x, N, L, lm, K, tri, T, src, img_idx,
                       faces, matrices);
}

void sdm_launch_warp_tensor(const uint8_t* base, const WarpFace* faces, const float* matrices, int T, const uint8_t* labels,
                            const AlignFrameDev* frames, const int* img_idx, int src_format, int N, int out_w, int out_h, int dtype,
                            int layout, int channels, const AlignTensorDev& spec, void* out, hipStream_t s)
{
    align_tensor_launch<WarpMesh>(base, faces, frames, img_idx, src_format, N, out_w, out_h, dtype, layout, channels, spec, {matrices, T, labels}, out, s);
}
