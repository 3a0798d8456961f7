// sdm_align_area.hip -- sdm_align_crops_tensor_filtered on gfx950 (include/sdm.h): the crop tensor of sdm_align_tensor.hip with every
// pixel of a minifying row averaged over S x S bilinear sub-samples of its footprint, in ONE launch behind align_fit_kernel.
//
//   align_tensor_kernel<AlignArea, DT, LAYOUT, CH>   the kernel frame of sdm_align_tensor_kernel.h.  A workgroup belongs to one face, so
//                       S -- computed here from the M the fit wrote, and reported through `samples` by the face's first lane -- is
//                       uniform in it.  S == 1: align_segment, the code of sdm_align_crops_tensor, no loop around it.  S > 1, the direct
//                       form: a lane loops over the S x S sub-samples of its 4 pixels and keeps uint32 sums per pixel and channel; the
//                       neighbouring sub-samples' taps overlap, which the vector L1 absorbs.
//
// The frame (grid, row source, channel / element stage, stores, dispatch) is sdm_align_tensor_kernel.h; the per-pixel arithmetic is
// sdm_align_area_device.h on top of sdm_align_tensor_device.h (also compiled for the host by tests/cpp/align_area_host.cpp).  No LDS.
#include "sdm_align_tensor_kernel.h"
#include "sdm_align_area_device.h"

namespace {

struct AlignArea {
    typedef AlignFace Face;
    struct Args { AlignAreaDev area; int* samples; };
    int S;
    __device__ __forceinline__ void enter(const Args& a, const AlignFace& f, int n, int lane)
    {
        S = align_area_samples(f.m, f.flags, a.area.mode, a.area.max_samples, a.area.min2);
        if (lane == 0) a.samples[n] = S;
    }
    template <bool WIDE>
    __device__ __forceinline__ void pixels(const Args&, const AlignFace& f, AlignRow& r, int i, int j0, int npx, int, uint32_t px[4][3])
    {
        align_row_matrix(f, r);
        if (S == 1) align_segment<WIDE>(r, i, j0, npx, px);
        else align_area_segment<WIDE>(r, i, j0, npx, S, px);
    }
};

}  // namespace

void sdm_launch_align_area(const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, int src_format,
                           int N, int out_w, int out_h, int dtype, int layout, int channels, const AlignTensorDev& spec,
                           const AlignAreaDev& area, int* samples, void* out, hipStream_t s)
{
    align_tensor_launch<AlignArea>(base, faces, frames, img_idx, src_format, N, out_w, out_h, dtype, layout, channels, spec, {area, samples}, out, s);
}
