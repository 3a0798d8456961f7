// sdm_align_tensor_kernel.h -- the one kernel frame of the three crop-tensor calls (csrc/sdm_align_tensor.hip, csrc/sdm_align_area.hip,
// csrc/sdm_warp.hip): the workgroup size, the element types and the stores, align_tensor_kernel -- lane -> 4 pixels, the row's source,
// the channel / element / layout stage -- and its dtype x layout x channels dispatch.  A call brings a policy P for what is its own:
//   P::Face    the per-row record its fit wrote: w, h, stride, off (AlignFace, WarpFace)
//   P::Args    its own kernel arguments, one struct by value
//   enter(a, f, n, lane)    run by EVERY lane of the workgroup before the bounds return: the one place for a barrier
//   pixels<WIDE>(a, f, r, i, j0, npx, out_w, px)    (B, G, R) of the lane's 4 pixels (row i, columns j0 ... j0 + npx - 1; (0, 0, 0) beyond)
//                           from the row's source r (r.m is the policy's to fill), 32-bit offsets inside a plane unless WIDE
// The per-pixel arithmetic is sdm_align_tensor_device.h.  Device code only.
#pragma once
#include "sdm_kernels.h"
#include "sdm_align_tensor_device.h"

#include <limits.h>

#pragma clang fp contract(off)

#define ALIGN_T_BLOCK 256

template <int DT> struct AlignElem;
template <> struct AlignElem<SDM_ALIGN_U8> { typedef uint8_t T; };
template <> struct AlignElem<SDM_ALIGN_F16> { typedef _Float16 T; };
template <> struct AlignElem<SDM_ALIGN_F32> { typedef float T; };

template <int DT>
__device__ __forceinline__ typename AlignElem<DT>::T make_elem(uint32_t v, float scale, float bias)
{
    if constexpr (DT == SDM_ALIGN_U8) return (uint8_t)v;
    else if constexpr (DT == SDM_ALIGN_F32) return align_element(v, scale, bias);
    else return (_Float16)align_element(v, scale, bias);          // round to nearest even
}

// output channel c of CH of a warped (B, G, R) as the tensor's element
template <int DT, int CH>
__device__ __forceinline__ typename AlignElem<DT>::T channel_elem(const uint32_t bgr[3], int c, bool weigh, const AlignTensorDev& t)
{
    return make_elem<DT>(align_channel<CH>(bgr, c, weigh, t.order, t.wb, t.wg, t.wr, t.gray_shift), t.scale[c], t.bias[c]);
}

// cnt <= CNT consecutive elements from element index e of out (16-byte aligned): whole groups of 4 as one vector store when e is a
// multiple of 4, the rest element by element
template <class T, int CNT>
__device__ __forceinline__ void store_run(void* out, long long e, const T (&vals)[CNT], int cnt)
{
    struct alignas(4 * sizeof(T)) Vec { T v[4]; };
    T* o = (T*)out + e;
    const bool aligned = (e & 3) == 0;
#pragma unroll
    for (int g = 0; g < CNT / 4; ++g) {
        if (aligned && cnt >= 4 * g + 4) {
            Vec v;
#pragma unroll
            for (int b = 0; b < 4; ++b) v.v[b] = vals[4 * g + b];
            *(Vec*)(o + 4 * g) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * g + b < cnt) o[4 * g + b] = vals[4 * g + b];
        }
    }
}

// a similarity row's matrix, for align_segment / align_area_segment
__device__ __forceinline__ void align_row_matrix(const AlignFace& f, AlignRow& r)
{
#pragma unroll
    for (int e = 0; e < 6; ++e) r.m[e] = f.m[e];
}

// workgroups of face n (blockIdx.x) read the fit's record and -- frame-list source -- the frame's table entry with scalar loads.  A lane
// owns 4 consecutive pixels of one crop row; each plane's 4 elements (NCHW) or the 4 * CH interleaved elements (NHWC) leave through
// store_run.
template <class P, int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(ALIGN_T_BLOCK) void align_tensor_kernel(const uint8_t* __restrict__ base, const typename P::Face* __restrict__ faces,
                                                                     const AlignFrameDev* __restrict__ frames, const int* __restrict__ img_idx,
                                                                     int src_format, int out_w, int out_h, AlignTensorDev t, typename P::Args a,
                                                                     void* __restrict__ out)
{
    typedef typename AlignElem<DT>::T T;
    const int n = blockIdx.x;
    const int segs = (out_w + 3) >> 2;                               // 4-pixel segments of a crop row
    const int lane = blockIdx.y * ALIGN_T_BLOCK + threadIdx.x;       // (at most 1024 * 256 segments per face)
    // the row's record: uniform for the workgroup
    const typename P::Face f = faces[n];
    P p;
    p.enter(a, f, n, lane);
    if (lane >= segs * out_h) return;
    const int i = lane / segs, j0 = (lane - i * segs) * 4;
    const int npx = out_w - j0 < 4 ? out_w - j0 : 4;
    AlignRow r;
    r.w = f.w; r.h = f.h;
    if (frames) {
        const AlignFrameDev fr = frames[img_idx ? img_idx[n] : n];
        r.p0 = fr.p0; r.p1 = fr.p1; r.stride = fr.stride; r.cstride = fr.cstride; r.format = fr.format;
        r.pd = (long long)((uintptr_t)fr.p1 - (uintptr_t)fr.p0);      // (a planar frame's p1 is its second plane; not read otherwise)
    } else {
        r.p0 = base + f.off; r.p1 = nullptr; r.stride = f.stride; r.cstride = 0; r.format = src_format; r.pd = 0;
    }
    const int fbase = SDM_FRAME_BASE(r.format);
    if (CH == 1 && fbase == SDM_FRAME_NV12) r.format = SDM_FRAME_GRAY;          // Y as it is, whatever the description: the chroma plane is not read
    if (CH == 1 && fbase == SDM_FRAME_P010) r.format |= YUV_LUMA_ONLY;          // the 10-bit luma alone
    const bool weigh = (r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA) || align_planar(r.format);
    // offsets inside a plane are 32-bit when rows * stride (bytes) fit 31 bits
    const bool two = fbase == SDM_FRAME_P010 || (CH != 1 && fbase == SDM_FRAME_NV12);
    const bool narrow = (long long)r.h * r.stride <= (long long)INT_MAX &&
                        (!two || (long long)((r.h + 1) >> 1) * r.cstride <= (long long)INT_MAX);
    uint32_t px[4][3];
    if (narrow) p.template pixels<false>(a, f, r, i, j0, npx, out_w, px);
    else p.template pixels<true>(a, f, r, i, j0, npx, out_w, px);

    if constexpr (LAYOUT == SDM_ALIGN_NCHW) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            T vals[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                vals[k] = channel_elem<DT, CH>(px[k], c, weigh, t);
            store_run<T, 4>(out, (((long long)n * CH + c) * out_h + i) * out_w + j0, vals, npx);
        }
    } else {
        T vals[4 * CH];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < CH; ++c)
                vals[k * CH + c] = channel_elem<DT, CH>(px[k], c, weigh, t);
        store_run<T, 4 * CH>(out, (((long long)n * out_h + i) * out_w + j0) * CH, vals, npx * CH);
    }
}

template <class P, int DT>
auto align_tensor_kernel_of(int layout, int channels) -> decltype(&align_tensor_kernel<P, DT, SDM_ALIGN_NCHW, 1>)
{
    // one channel: the two layouts are the same addresses
    return channels == 1 ? align_tensor_kernel<P, DT, SDM_ALIGN_NCHW, 1>
         : layout == SDM_ALIGN_NCHW ? align_tensor_kernel<P, DT, SDM_ALIGN_NCHW, 3> : align_tensor_kernel<P, DT, SDM_ALIGN_NHWC, 3>;
}

// the launch of P's kernel for N faces: grid (N, segments of a face / ALIGN_T_BLOCK)
template <class P>
void align_tensor_launch(const uint8_t* base, const typename P::Face* faces, const AlignFrameDev* frames, const int* img_idx, int src_format, int N,
                         int out_w, int out_h, int dtype, int layout, int channels, const AlignTensorDev& spec, const typename P::Args& a,
                         void* out, hipStream_t s)
{
    const int lanes = ((out_w + 3) / 4) * out_h;
    const dim3 grid((unsigned)N, (unsigned)((lanes + ALIGN_T_BLOCK - 1) / ALIGN_T_BLOCK));
    const auto kernel = dtype == SDM_ALIGN_U8 ? align_tensor_kernel_of<P, SDM_ALIGN_U8>(layout, channels)
                      : dtype == SDM_ALIGN_F16 ? align_tensor_kernel_of<P, SDM_ALIGN_F16>(layout, channels)
                                               : align_tensor_kernel_of<P, SDM_ALIGN_F32>(layout, channels);
    hipLaunchKernelGGL(kernel, grid, dim3(ALIGN_T_BLOCK), 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, a, out);
}
