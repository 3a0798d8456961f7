// sdm_track.hip -- multi-stream face tracking on gfx950: the hand-offs between a table of S stream slots (each slot's landmark
// row, face box and status, in HBM) and the detect cascade's state x.  The cascade between them is sdm_detect_batch's, unchanged.
//
//   track_start_kernel    (re)start: slot ids[i] takes box i and the status STARTED
//   track_gather_kernel   step, before the cascade: row i of x (and a copy, the init) from slot ids[i] --
//                           STARTED   align_mean(mean, box): the arithmetic of sdm_apply.hip::init_boxes_kernel
//                           PREVIOUS  the slot's landmarks (rcr::detection_model::detect(image, initialisation))
//                           REALIGN   the mean placed in the enclosing box of the slot's landmarks
//   track_commit_kernel   step, after the cascade: row i back into slot ids[i], and the lost decision (bit mask, 0 = tracked)
//
// One 64-lane wave per row; the 2L coordinates are strided over the lanes, min / max reduced across the lanes (exact in any
// order).  float32 throughout, -ffp-contract=off (csrc/Makefile): every operation is rounded as written.
#include "sdm_kernels.h"
#include "../../include/sdm.h"

#pragma clang fp contract(off)
#include "sdm_ied.h"           // device_ied_rows

namespace {

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_or(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// enclosing box of a landmark row: min / max of the x and of the y coordinates
__device__ __forceinline__ void row_bounds(const float* __restrict__ xr, int L, int lane, float& x0, float& x1, float& y0, float& y1)
{
    float a = INFINITY, b = -INFINITY, c = INFINITY, d = -INFINITY;
    for (int j = lane; j < L; j += 64) {
        const float vx = xr[j], vy = xr[L + j];
        a = fminf(a, vx); b = fmaxf(b, vx);
        c = fminf(c, vy); d = fmaxf(d, vy);
    }
    x0 = wave_min(a); x1 = wave_max(b); y0 = wave_min(c); y1 = wave_max(d);
}

__global__ void track_start_kernel(const int* __restrict__ ids, const int* __restrict__ boxes, int n, int* __restrict__ slot_box,
                                   int* __restrict__ slot_status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    for (int k = 0; k < 4; ++k) slot_box[4 * id + k] = boxes[4 * i + k];
    slot_status[id] = SDM_TRACK_STARTED;
}

__global__ __launch_bounds__(64) void track_gather_kernel(const int* __restrict__ ids, int L, int mode, const int* __restrict__ slot_status,
                                                          const int* __restrict__ slot_box, const float* __restrict__ slot_x,
                                                          const float* __restrict__ mean, float4 mb, const float* __restrict__ shift,
                                                          float* __restrict__ x, float* __restrict__ init)
{
    const int i = blockIdx.x, lane = threadIdx.x, M = 2 * L;
    const int id = ids[i];
    const float* prev = slot_x + (long long)id * M;
    // the motion search's shift of a tracked slot's landmarks as they are read (csrc/sdm_track_motion.hip); (0, 0) and no pointer: the bits
    const float sx = shift ? shift[2 * i] : 0.0f, sy = shift ? shift[2 * i + 1] : 0.0f;
    const bool moved = sx != 0.0f || sy != 0.0f;
    float* xo = x + (long long)i * M;
    float* io = init ? init + (long long)i * M : nullptr;
    const int st = slot_status[id];           // (uniform over the wave: every branch below is taken by all lanes or none)
    if (st == SDM_TRACK_STARTED) {
        // init_boxes_kernel (sdm_apply.hip) without perturbation: (m * 1 + 0.5 + 0) * extent + origin, model.hpp:73-74
        const int bx = slot_box[4 * id], by = slot_box[4 * id + 1], bw = slot_box[4 * id + 2], bh = slot_box[4 * id + 3];
        for (int j = lane; j < M; j += 64) {
            const float m = mean[j];
            const float v = j < L ? (m * 1.0f + 0.5f + 0.0f) * (float)bw + (float)bx : (m * 1.0f + 0.5f + 0.0f) * (float)bh + (float)by;
            xo[j] = v;
            if (io) io[j] = v;
        }
    } else if (mode == SDM_TRACK_INIT_PREVIOUS) {
        for (int j = lane; j < M; j += 64) {
            const float v = moved ? prev[j] + (j < L ? sx : sy) : prev[j];
            xo[j] = v;
            if (io) io[j] = v;
        }
    } else {
        // the mean in the enclosing box of the previous landmarks: x0[j] = ((m[j] - mx0) / (mx1 - mx0)) * (bx1 - bx0) + bx0
        float bx0, bx1, by0, by1;
        row_bounds(prev, L, lane, bx0, bx1, by0, by1);
        if (moved) { bx0 = bx0 + sx; bx1 = bx1 + sx; by0 = by0 + sy; by1 = by1 + sy; }      // (min / max of the shifted row: the add is monotonic)
        for (int j = lane; j < M; j += 64) {
            const float m = mean[j];
            const float v = j < L ? ((m - mb.x) / (mb.y - mb.x)) * (bx1 - bx0) + bx0 : ((m - mb.z) / (mb.w - mb.z)) * (by1 - by0) + by0;
            xo[j] = v;
            if (io) io[j] = v;
        }
    }
}

__global__ __launch_bounds__(64) void track_commit_kernel(const int* __restrict__ ids, int n, int L, const float* __restrict__ x,
                                                          const float* __restrict__ init, const int* __restrict__ img_idx,
                                                          const int* __restrict__ img_w, const int* __restrict__ img_h, EyeIdxDev eyes,
                                                          float min_size, float max_scale_change, float* __restrict__ slot_x,
                                                          int* __restrict__ slot_status, int* __restrict__ masks,
                                                          const int* __restrict__ status_word)
{
    const int i = blockIdx.x, lane = threadIdx.x, M = 2 * L;
    const int id = ids[i];
    const float* xr = x + (long long)i * M;
    float* so = slot_x + (long long)id * M;
    int bad = 0;
    for (int j = lane; j < M; j += 64) {
        const float v = xr[j];
        bad |= !isfinite(v);
        so[j] = v;                              // (a lost slot keeps its last landmarks for inspection)
    }
    bad = wave_or(bad);
    float bx0, bx1, by0, by1;
    row_bounds(xr, L, lane, bx0, bx1, by0, by1);
    if (lane != 0) return;
    int mask = 0;
    if (bad) {
        mask = SDM_TRACK_LOST_NONFINITE;        // (the other rules are not evaluated on a non-finite row)
    } else {
        if (bx1 - bx0 < min_size || by1 - by0 < min_size) mask |= SDM_TRACK_LOST_SMALL;
        const int im = img_idx ? img_idx[i] : i;
        const float cx = (bx0 + bx1) * 0.5f, cy = (by0 + by1) * 0.5f;
        if (!(cx >= 0.0f && cx < (float)img_w[im] && cy >= 0.0f && cy < (float)img_h[im])) mask |= SDM_TRACK_LOST_OUTSIDE;
        if (eyes.nre > 0 && eyes.nle > 0 && max_scale_change > 0.0f) {
            const double r = device_ied_rows(xr, L, eyes), s = device_ied_rows(init + (long long)i * M, L, eyes);
            const double k = (double)max_scale_change;
            if (r > s * k || r * k < s) mask |= SDM_TRACK_LOST_SCALE;
        }
    }
    slot_status[id] = mask ? SDM_TRACK_LOST : SDM_TRACK_TRACKED;
    masks[i] = mask;
    if (i == 0) masks[n] = *status_word;        // the context's kernel status, returned with the masks (one copy, one synchronise)
}

}  // namespace

void sdm_launch_track_start(const int* ids, const int* boxes, int n, int* slot_box, int* slot_status, hipStream_t s)
{
    hipLaunchKernelGGL(track_start_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, boxes, n, slot_box, slot_status);
}

void sdm_launch_track_gather(const int* ids, int n, int L, int mode, const int* slot_status, const int* slot_box, const float* slot_x,
                             const float* mean, const float mean_bounds[4], float* x, float* init, hipStream_t s, const float* shift)
{
    const float4 mb = make_float4(mean_bounds[0], mean_bounds[1], mean_bounds[2], mean_bounds[3]);
    hipLaunchKernelGGL(track_gather_kernel, dim3((unsigned)n), dim3(64), 0, s, ids, L, mode, slot_status, slot_box, slot_x, mean, mb, shift, x,
                       init);
}

void sdm_launch_track_commit(const int* ids, int n, int L, const float* x, const float* init, const int* img_idx, const int* img_w,
                             const int* img_h, const EyeIdxDev& eyes, float min_size, float max_scale_change, float* slot_x,
                             int* slot_status, int* masks, const int* status_word, hipStream_t s)
{
    hipLaunchKernelGGL(track_commit_kernel, dim3((unsigned)n), dim3(64), 0, s, ids, n, L, x, init, img_idx, img_w, img_h, eyes, min_size,
                       max_scale_change, slot_x, slot_status, masks, status_word);
}
