// sdm_warp.hip -- piecewise-affine warped faces as a network's input tensor on gfx950 (include/sdm.h, "Warped faces",
// sdm_warp_crops_tensor): every triangle of the mesh carries its own crop -> source matrix, so every landmark lands on its template point.
//
//   warp_fit_kernel     one wave per row, one lane per triangle (T > 64: in turns): the lanes first look at the mesh's K landmarks --
//                       DEGENERATE, PARTIAL --, then every lane forms its triangle's matrix in double (warp_fit_triangle) and writes
//                       six floats of the N x T x 6 table; FOLDED and the other bits are ORed across the wave by ballot, and lane 0
//                       writes the row's record: the flag word does not depend on any execution order, nothing is atomic.
//   warp_tensor_kernel<DT, LAYOUT, CH>   the shape of align_tensor_kernel: workgroups of face n (blockIdx.x), a lane owns 4 consecutive
//                       pixels of one crop row, the row's record or frame entry is read once per workgroup.  The workgroup first stages
//                       its face's T x 6 floats in LDS (records of 6 floats, at most 6 096 bytes); a lane reads its 4 labels (one dword
//                       when the four lie in the crop row and the address is a multiple of 4, bytes otherwise) and fetches each pixel's
//                       matrix from LDS by its label -- neighbouring lanes mostly share a triangle, so most reads are broadcasts.  A
//                       pixel without a triangle reads no source byte.  Stores: store_run, as the crop tensor's.
//
// The per-pixel arithmetic is sdm_warp_device.h on top of sdm_align_tensor_device.h (also compiled for the host by tests/cpp/warp_host.cpp).
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

template <int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(ALIGN_T_BLOCK) void warp_tensor_kernel(const uint8_t* __restrict__ base, const WarpFace* __restrict__ faces,
                                                                    const float* __restrict__ matrices, int T,
                                                                    const uint8_t* __restrict__ labels, const AlignFrameDev* __restrict__ frames,
                                                                    const int* __restrict__ img_idx, int src_format, int out_w, int out_h,
                                                                    AlignTensorDev t, void* __restrict__ out)
{
    typedef typename AlignElem<DT>::T E;
    __shared__ float tm[SDM_WARP_MAX_TRIANGLES * WARP_LDS_REC];
    const int n = blockIdx.x;
    // the face's matrices: T x 6 floats into LDS
    const float* mrow = matrices + (long long)n * T * 6;
    for (int e = threadIdx.x; e < T * 6; e += ALIGN_T_BLOCK) {
        const int tt = e / 6;
        tm[tt * WARP_LDS_REC + (e - tt * 6)] = mrow[e];
    }
    __syncthreads();
    const int segs = (out_w + 3) >> 2;                               // 4-pixel segments of a crop row
    const int lane = blockIdx.y * ALIGN_T_BLOCK + threadIdx.x;       // (at most 1024 * 256 segments per face)
    if (lane >= segs * out_h) return;
    const int i = lane / segs, j0 = (lane - i * segs) * 4;
    const int npx = out_w - j0 < 4 ? out_w - j0 : 4;
    // the row's record: uniform for the workgroup
    const WarpFace f = faces[n];
    AlignRow r;
    r.w = f.w; r.h = f.h;
    if (frames) {
        const AlignFrameDev fr = frames[img_idx ? img_idx[n] : n];
        r.p0 = fr.p0; r.p1 = fr.p1; r.stride = fr.stride; r.cstride = fr.cstride; r.format = fr.format;
    } else {
        r.p0 = base + f.off; r.p1 = nullptr; r.stride = f.stride; r.cstride = 0; r.format = src_format;
    }
    if (CH == 1 && r.format == SDM_FRAME_NV12) r.format = SDM_FRAME_GRAY;        // Y as it is: the chroma plane is not read
    const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
    const bool narrow = (long long)r.h * r.stride <= (long long)INT_MAX &&
                        (r.format != SDM_FRAME_NV12 || (long long)((r.h + 1) >> 1) * r.cstride <= (long long)INT_MAX);
    // the 4 labels (out_w * out_h <= 2^20)
    const int at = i * out_w + j0;
    uint32_t lab[4];
    if (npx == 4 && (at & 3) == 0) {
        const uint32_t v = *(const uint32_t*)(labels + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) lab[k] = (v >> (8 * k)) & 255u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) lab[k] = k < npx ? (uint32_t)labels[at + k] : (uint32_t)SDM_WARP_NO_TRIANGLE;
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
    uint32_t px[4][3];
    if (narrow) warp_segment<false>(r, sx, sy, on, px);
    else warp_segment<true>(r, sx, sy, on, px);

    if constexpr (LAYOUT == SDM_ALIGN_NCHW) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            E vals[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                vals[k] = make_elem<DT>(align_channel<CH>(px[k], c, weigh, t.order, t.wb, t.wg, t.wr, t.gray_shift), t.scale[c], t.bias[c]);
            store_run<E, 4>(out, (((long long)n * CH + c) * out_h + i) * out_w + j0, vals, npx);
        }
    } else {
        E vals[4 * CH];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < CH; ++c)
                vals[k * CH + c] = make_elem<DT>(align_channel<CH>(px[k], c, weigh, t.order, t.wb, t.wg, t.wr, t.gray_shift), t.scale[c], t.bias[c]);
        store_run<E, 4 * CH>(out, (((long long)n * out_h + i) * out_w + j0) * CH, vals, npx * CH);
    }
}

#define WARP_LAUNCH(DT, LAYOUT, CH) \
    hipLaunchKernelGGL((warp_tensor_kernel<DT, LAYOUT, CH>), grid, dim3(ALIGN_T_BLOCK), 0, s, base, faces, matrices, T, labels, frames, img_idx, \
                       src_format, out_w, out_h, t, out)

template <int DT>
void launch_layout(int layout, int channels, dim3 grid, hipStream_t s, const uint8_t* base, const WarpFace* faces, const float* matrices, int T,
                   const uint8_t* labels, const AlignFrameDev* frames, const int* img_idx, int src_format, int out_w, int out_h,
                   const AlignTensorDev& t, void* out)
{
    // one channel: the two layouts are the same addresses
    if (channels == 1) WARP_LAUNCH(DT, SDM_ALIGN_NCHW, 1);
    else if (layout == SDM_ALIGN_NCHW) WARP_LAUNCH(DT, SDM_ALIGN_NCHW, 3);
    else WARP_LAUNCH(DT, SDM_ALIGN_NHWC, 3);
}

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
    const int lanes = ((out_w + 3) / 4) * out_h;
    const dim3 grid((unsigned)N, (unsigned)((lanes + ALIGN_T_BLOCK - 1) / ALIGN_T_BLOCK));
    if (dtype == SDM_ALIGN_U8) launch_layout<SDM_ALIGN_U8>(layout, channels, grid, s, base, faces, matrices, T, labels, frames, img_idx, src_format, out_w, out_h, spec, out);
    else if (dtype == SDM_ALIGN_F16) launch_layout<SDM_ALIGN_F16>(layout, channels, grid, s, base, faces, matrices, T, labels, frames, img_idx, src_format, out_w, out_h, spec, out);
    else launch_layout<SDM_ALIGN_F32>(layout, channels, grid, s, base, faces, matrices, T, labels, frames, img_idx, src_format, out_w, out_h, spec, out);
}
