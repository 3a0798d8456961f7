// sdm_align_tensor.hip -- aligned crops written as a network's input tensor on gfx950 (include/sdm.h, sdm_align_crops_tensor): the
// warp of sdm_align.hip from GRAY / BGR / RGB / BGRA / RGBA / NV12 frames used in place, the NV12 conversion, the channel rules
// (order, colour -> gray), the element formula (u8, or float32 / float16 of v * scale + bias) and the layout (NHWC / NCHW) in ONE launch
// behind align_fit_kernel, which is reused as it is.
//
//   align_tensor_kernel<DT, LAYOUT, CH>   workgroups of face n (blockIdx.x) read the fit's record and -- frame-list source -- the
//                       frame's table entry with scalar loads and switch on the source format once.  A lane owns 4 consecutive pixels
//                       of one crop row: the products M01 i, M11 i are shared, offsets inside a plane are 32-bit when rows * stride
//                       fit 31 bits, and each plane's 4 elements (NCHW) or the 4 * CH interleaved elements (NHWC) leave as
//                       4-element vectors (dword / 8 bytes / 16 bytes) when the element index is a multiple of 4, one by one otherwise.
//   align_frame_rows_kernel   sdm_align_crops on a frame list of one pixel size: the fit's records re-pointed at the frames
//
// The per-pixel arithmetic is sdm_align_tensor_device.h (also compiled for the host by tests/cpp/align_tensor_host.cpp); the element types
// and the stores are sdm_align_tensor_kernel.h, shared with csrc/sdm_align_area.hip.  No LDS.
#include "sdm_align_tensor_kernel.h"

namespace {

template <int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(ALIGN_T_BLOCK) void align_tensor_kernel(const uint8_t* __restrict__ base, const AlignFace* __restrict__ faces,
                                                                     const AlignFrameDev* __restrict__ frames, const int* __restrict__ img_idx,
                                                                     int src_format, int out_w, int out_h, AlignTensorDev t, void* __restrict__ out)
{
    typedef typename AlignElem<DT>::T T;
    const int n = blockIdx.x;
    const int segs = (out_w + 3) >> 2;                               // 4-pixel segments of a crop row
    const int lane = blockIdx.y * ALIGN_T_BLOCK + threadIdx.x;       // (at most 1024 * 256 segments per face)
    if (lane >= segs * out_h) return;
    const int i = lane / segs, j0 = (lane - i * segs) * 4;
    const int npx = out_w - j0 < 4 ? out_w - j0 : 4;
    // the row's record: uniform for the workgroup
    const AlignFace f = faces[n];
    AlignRow r;
#pragma unroll
    for (int e = 0; e < 6; ++e) r.m[e] = f.m[e];
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
    uint32_t px[4][3];
    if (narrow) align_segment<false>(r, i, j0, npx, px);
    else align_segment<true>(r, i, j0, npx, px);

    if constexpr (LAYOUT == SDM_ALIGN_NCHW) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            T vals[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                vals[k] = make_elem<DT>(align_channel<CH>(px[k], c, weigh, t.order, t.wb, t.wg, t.wr, t.gray_shift), t.scale[c], t.bias[c]);
            store_run<T, 4>(out, (((long long)n * CH + c) * out_h + i) * out_w + j0, vals, npx);
        }
    } else {
        T vals[4 * CH];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < CH; ++c)
                vals[k * CH + c] = make_elem<DT>(align_channel<CH>(px[k], c, weigh, t.order, t.wb, t.wg, t.wr, t.gray_shift), t.scale[c], t.bias[c]);
        store_run<T, 4 * CH>(out, (((long long)n * out_h + i) * out_w + j0) * CH, vals, npx * CH);
    }
}

__global__ __launch_bounds__(256) void align_frame_rows_kernel(AlignFace* __restrict__ faces, const AlignFrameDev* __restrict__ frames,
                                                               const int* __restrict__ img_idx, const uint8_t* base, int N)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const AlignFrameDev fr = frames[img_idx ? img_idx[r] : r];
    faces[r].off = (long long)(fr.p0 - base);
    faces[r].stride = fr.stride;
}

template <int DT>
void launch_nchw(int channels, dim3 grid, hipStream_t s, const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames,
               const int* img_idx, int src_format, int out_w, int out_h, const AlignTensorDev& t, void* out)
{
    if (channels == 1)
        hipLaunchKernelGGL((align_tensor_kernel<DT, SDM_ALIGN_NCHW, 1>), grid, dim3(ALIGN_T_BLOCK), 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, out);
    else
        hipLaunchKernelGGL((align_tensor_kernel<DT, SDM_ALIGN_NCHW, 3>), grid, dim3(ALIGN_T_BLOCK), 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, out);
}

template <int DT>
void launch_layout(int layout, int channels, dim3 grid, hipStream_t s, const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames,
                   const int* img_idx, int src_format, int out_w, int out_h, const AlignTensorDev& t, void* out)
{
    // one channel: the two layouts are the same addresses
    if (layout == SDM_ALIGN_NCHW || channels == 1) launch_nchw<DT>(channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, out);
    else hipLaunchKernelGGL((align_tensor_kernel<DT, SDM_ALIGN_NHWC, 3>), grid, dim3(ALIGN_T_BLOCK), 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, out);
}

}  // namespace

void sdm_launch_align_tensor(const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, int src_format,
                             int N, int out_w, int out_h, int dtype, int layout, int channels, const AlignTensorDev& spec, void* out,
                             hipStream_t s)
{
    const int lanes = ((out_w + 3) / 4) * out_h;
    const dim3 grid((unsigned)N, (unsigned)((lanes + ALIGN_T_BLOCK - 1) / ALIGN_T_BLOCK));
    if (dtype == SDM_ALIGN_U8) launch_layout<SDM_ALIGN_U8>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, out);
    else if (dtype == SDM_ALIGN_F16) launch_layout<SDM_ALIGN_F16>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, out);
    else launch_layout<SDM_ALIGN_F32>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, out);
}

void sdm_launch_align_frame_rows(AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, const uint8_t* base, int N, hipStream_t s)
{
    hipLaunchKernelGGL(align_frame_rows_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, faces, frames, img_idx, base, N);
}
