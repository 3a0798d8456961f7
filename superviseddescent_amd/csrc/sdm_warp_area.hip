// sdm_warp_area.hip -- sdm_warp_crops_tensor_filtered on gfx950 (include/sdm.h, "Warped faces, filtered"): the warped tensor of
// sdm_warp.hip with every pixel of a minifying triangle averaged over Sx x Sy bilinear sub-samples of its footprint, the counts chosen per
// triangle and per axis, in ONE launch behind warp_fit_kernel.
//
//   align_tensor_kernel<WarpMeshArea, DT, LAYOUT, CH>   the kernel frame of sdm_align_tensor_kernel.h.  The workgroup stages its face's
//                       triangles in LDS, records of 8 words (WarpAreaRec, at most 8 128 bytes): the thread that stages triangle t reads its six
//                       floats, computes (Sx, Sy) from them and the filter and stores the record; the face's first workgroup also writes
//                       the pair to `samples`.  A lane reads its 4 labels as WarpMesh does and first only the counts of its pixels'
//                       triangles -- neighbouring lanes mostly share a triangle, so most LDS reads are broadcasts.  When every live
//                       pixel of the lane has Sx = Sy = 1: warp_position and align_fetch_segment, the code of
//                       sdm_warp_crops_tensor.  Otherwise warp_area_segment: every pixel's own pair of loops over its Sx x Sy sub-samples
//                       (DESIGN 4.22 has the choice against one loop to the lane's largest count).
//
// The frame (grid, row source, channel / element stage, stores, dispatch) is sdm_align_tensor_kernel.h; the per-pixel arithmetic is
// sdm_warp_area_device.h (also compiled for the host by tests/cpp/warp_area_host.cpp).
#include "sdm_warp.h"
#include "sdm_align_tensor_kernel.h"
#include "sdm_warp_area_device.h"

#pragma clang fp contract(off)

namespace {

struct WarpMeshArea {
    typedef WarpFace Face;
    struct Args { const float* matrices; int T; const uint8_t* labels; AlignAreaDev area; int* samples; };
    const WarpAreaRec* tm;
    // the face's triangles: T records (M00 ... M12, Sx, Sy) into LDS, one thread per triangle (T <= 254 < ALIGN_T_BLOCK)
    __device__ __forceinline__ void enter(const Args& a, const WarpFace& f, int n, int)
    {
        __shared__ WarpAreaRec lds[SDM_WARP_MAX_TRIANGLES];
        const int t = threadIdx.x;
        if (t < a.T) {
            const float2* mt = (const float2*)(a.matrices + ((long long)n * a.T + t) * 6);      // (records of 24 bytes, 8-byte aligned)
            const float2 m01 = mt[0], m23 = mt[1], m45 = mt[2];
            WarpAreaRec rec;
            rec.m[0] = m01.x; rec.m[1] = m01.y; rec.m[2] = m23.x; rec.m[3] = m23.y; rec.m[4] = m45.x; rec.m[5] = m45.y;
            warp_area_samples(rec.m, f.flags, a.area.mode, a.area.max_samples, a.area.min2, rec.Sx, rec.Sy);
            lds[t] = rec;
            if (blockIdx.y == 0) ((int2*)a.samples)[(long long)n * a.T + t] = make_int2(rec.Sx, rec.Sy);
        }
        __syncthreads();
        tm = lds;
    }
    template <bool WIDE>
    __device__ __forceinline__ void pixels(const Args& a, const WarpFace&, AlignRow& r, int i, int j0, int npx, int out_w, uint32_t px[4][3])
    {
        // the 4 labels (out_w * out_h <= 2^20)
        const int at = i * out_w + j0;
        int lab[4];
        if (npx == 4 && (at & 3) == 0) {
            const uint32_t v = *(const uint32_t*)(a.labels + at);
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = (int)((v >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = k < npx ? (int)a.labels[at + k] : SDM_WARP_NO_TRIANGLE;
        }
        bool plain = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lab[k] == SDM_WARP_NO_TRIANGLE) lab[k] = -1;
            else plain = plain && tm[lab[k]].Sx == 1 && tm[lab[k]].Sy == 1;
        }
        if (plain) {
            float sx[4], sy[4];
            bool on[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                on[k] = lab[k] >= 0;
                sx[k] = sy[k] = 0.0f;
                if (on[k]) warp_position(tm[lab[k]].m, j0 + k, i, sx[k], sy[k]);
            }
            align_fetch_segment<WIDE>(r, sx, sy, on, px);
        } else {
            warp_area_segment<WIDE>(r, tm, lab, i, j0, px);
        }
    }
};

}  // namespace

void sdm_launch_warp_area(const uint8_t* base, const WarpFace* faces, const float* matrices, int T, const uint8_t* labels,
                          const AlignFrameDev* frames, const int* img_idx, int src_format, int N, int out_w, int out_h, int dtype,
                          int layout, int channels, const AlignTensorDev& spec, const AlignAreaDev& area, int* samples, void* out,
                          hipStream_t s)
{
    align_tensor_launch<WarpMeshArea>(base, faces, frames, img_idx, src_format, N, out_w, out_h, dtype, layout, channels, spec,
                                      {matrices, T, labels, area, samples}, out, s);
}
