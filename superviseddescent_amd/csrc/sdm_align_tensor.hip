// sdm_align_tensor.hip -- aligned crops written as a network's input tensor on gfx950 (include/sdm.h, sdm_align_crops_tensor): the
// warp of sdm_align.hip from GRAY / BGR / RGB / BGRA / RGBA / NV12 frames used in place, the NV12 conversion, the channel rules
// (order, colour -> gray), the element formula (u8, or float32 / float16 of v * scale + bias) and the layout (NHWC / NCHW) in ONE launch
// behind align_fit_kernel, which is reused as it is.
//
//   align_tensor_kernel<AlignBilinear, DT, LAYOUT, CH>   the kernel frame of sdm_align_tensor_kernel.h with nothing added: a lane's 4 pixels
//                       are align_segment through the row's one matrix.
//   align_frame_rows_kernel   sdm_align_crops on a frame list of one pixel size: the fit's records re-pointed at the frames
//
// The frame (grid, row source, channel / element stage, stores, dispatch) is sdm_align_tensor_kernel.h, shared with csrc/sdm_align_area.hip
// and csrc/sdm_warp.hip; the per-pixel arithmetic is sdm_align_tensor_device.h (also compiled for the host by
// tests/cpp/align_tensor_host.cpp).  No LDS.
#include "sdm_align_tensor_kernel.h"

namespace {

struct AlignBilinear {
    typedef AlignFace Face;
    struct Args {};
    __device__ __forceinline__ void enter(const Args&, const AlignFace&, int, int) {}
    template <bool WIDE>
    __device__ __forceinline__ void pixels(const Args&, const AlignFace& f, AlignRow& r, int i, int j0, int npx, int, uint32_t px[4][3])
    {
        align_row_matrix(f, r);
        align_segment<WIDE>(r, i, j0, npx, px);
    }
};

__global__ __launch_bounds__(256) void align_frame_rows_kernel(AlignFace* __restrict__ faces, const AlignFrameDev* __restrict__ frames,
                                                               const int* __restrict__ img_idx, const uint8_t* base, int N)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const AlignFrameDev fr = frames[img_idx ? img_idx[r] : r];
    faces[r].off = (long long)(fr.p0 - base);
    faces[r].stride = fr.stride;
}

}  // namespace

void sdm_launch_align_tensor(const uint8_t* base, const AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, int src_format,
                             int N, int out_w, int out_h, int dtype, int layout, int channels, const AlignTensorDev& spec, void* out,
                             hipStream_t s)
{
    align_tensor_launch<AlignBilinear>(base, faces, frames, img_idx, src_format, N, out_w, out_h, dtype, layout, channels, spec, {}, out, s);
}

void sdm_launch_align_frame_rows(AlignFace* faces, const AlignFrameDev* frames, const int* img_idx, const uint8_t* base, int N, hipStream_t s)
{
    hipLaunchKernelGGL(align_frame_rows_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, faces, frames, img_idx, base, N);
}
