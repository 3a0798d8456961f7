// sdm_align_area.hip -- sdm_align_crops_tensor_filtered on gfx950 (include/sdm.h): the crop tensor of sdm_align_tensor.hip with every
// pixel of a minifying row averaged over S x S bilinear sub-samples of its footprint, in ONE launch behind align_fit_kernel.
//
//   align_area_kernel<DT, LAYOUT, CH>   the grid, the row's record and the stores of align_tensor_kernel.  A workgroup belongs to one
//                       face, so S -- computed here from the M the fit wrote, and reported through `samples` by the face's first lane -- is
//                       uniform in it.  S == 1: align_segment, the code of sdm_align_crops_tensor, no loop around it.  S > 1, the direct
//                       form: a lane loops over the S x S sub-samples of its 4 pixels and keeps uint32 sums per pixel and channel; the
//                       neighbouring sub-samples' taps overlap, which the vector L1 absorbs.
//
// The per-pixel arithmetic is sdm_align_area_device.h (also compiled for the host by tests/cpp/align_area_host.cpp).  No LDS.
#include "sdm_align_tensor_kernel.h"
#include "sdm_align_area_device.h"

namespace {

template <int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(ALIGN_T_BLOCK) void align_area_kernel(const uint8_t* __restrict__ base, const AlignFace* __restrict__ faces,
                                                                   const AlignFrameDev* __restrict__ frames, const int* __restrict__ img_idx,
                                                                   int src_format, int out_w, int out_h, AlignTensorDev t, AlignAreaDev a,
                                                                   int* __restrict__ samples, void* __restrict__ out)
{
    typedef typename AlignElem<DT>::T T;
    const int n = blockIdx.x;
    const int segs = (out_w + 3) >> 2;                               // 4-pixel segments of a crop row
    const int lane = blockIdx.y * ALIGN_T_BLOCK + threadIdx.x;       // (at most 1024 * 256 segments per face)
    // the row's record: uniform for the workgroup
    const AlignFace f = faces[n];
    const int S = align_area_samples(f.m, f.flags, a.mode, a.max_samples, a.min2);
    if (lane == 0) samples[n] = S;
    if (lane >= segs * out_h) return;
    const int i = lane / segs, j0 = (lane - i * segs) * 4;
    const int npx = out_w - j0 < 4 ? out_w - j0 : 4;
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
    if (CH == 1 && r.format == SDM_FRAME_NV12) r.format = SDM_FRAME_GRAY;        // the averaged Y as it is: the chroma plane is not read
    const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
    const bool narrow = (long long)r.h * r.stride <= (long long)INT_MAX &&
                        (r.format != SDM_FRAME_NV12 || (long long)((r.h + 1) >> 1) * r.cstride <= (long long)INT_MAX);
    uint32_t px[4][3];
    if (S == 1) {
        if (narrow) align_segment<false>(r, i, j0, npx, px);
        else align_segment<true>(r, i, j0, npx, px);
    } else {
        if (narrow) align_area_segment<false>(r, i, j0, npx, S, px);
        else align_area_segment<true>(r, i, j0, npx, S, px);
    }

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

template <int DT>
void launch_layout(int layout, int channels, dim3 grid, hipStream_t s, const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames,
                   const int* img_idx, int src_format, int out_w, int out_h, const AlignTensorDev& t, const AlignAreaDev& a, int* samples, void* out)
{
    const dim3 block(ALIGN_T_BLOCK);
    // one channel: the two layouts are the same addresses
    if (channels == 1)
        hipLaunchKernelGGL((align_area_kernel<DT, SDM_ALIGN_NCHW, 1>), grid, block, 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, a, samples, out);
    else if (layout == SDM_ALIGN_NCHW)
        hipLaunchKernelGGL((align_area_kernel<DT, SDM_ALIGN_NCHW, 3>), grid, block, 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, a, samples, out);
    else
        hipLaunchKernelGGL((align_area_kernel<DT, SDM_ALIGN_NHWC, 3>), grid, block, 0, s, base, faces, frames, img_idx, src_format, out_w, out_h, t, a, samples, out);
}

}  // namespace

void sdm_launch_align_area(const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, int src_format,
                           int N, int out_w, int out_h, int dtype, int layout, int channels, const AlignTensorDev& spec,
                           const AlignAreaDev& area, int* samples, void* out, hipStream_t s)
{
    const int lanes = ((out_w + 3) / 4) * out_h;
    const dim3 grid((unsigned)N, (unsigned)((lanes + ALIGN_T_BLOCK - 1) / ALIGN_T_BLOCK));
    if (dtype == SDM_ALIGN_U8) launch_layout<SDM_ALIGN_U8>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, area, samples, out);
    else if (dtype == SDM_ALIGN_F16) launch_layout<SDM_ALIGN_F16>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, area, samples, out);
    else launch_layout<SDM_ALIGN_F32>(layout, channels, grid, s, base, faces, frames, img_idx, src_format, out_w, out_h, spec, area, samples, out);
}
