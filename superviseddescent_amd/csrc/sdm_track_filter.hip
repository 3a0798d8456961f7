// sdm_track_filter.hip -- the tracker's temporal landmark filter on gfx950 (include/sdm.h, "Tracking, filtered"): behind
// track_commit_kernel (csrc/sdm_track.hip) one launch takes the raw result rows of a step through the One-Euro filter of their
// slots and leaves the filtered rows as the current x.  The slots' landmark rows stay raw: what the next step starts from, the lost
// rule and sdm_track_get are those of a tracker without the filter.
//
//   track_filter_kernel          step: row i of x through the filter state of slot ids[i], in place
//   track_filter_unprime_kernel  (re)start: the named slots' filters forget what they held
//   track_filter_get_kernel      the named slots' filtered rows, derivative rows and primed flags, zeros where a slot is not primed
//
// Shaped like track_gather_kernel and track_commit_kernel: one 64-lane wave per row, the 2L coordinates strided over the lanes, the
// face size from min / max reduced across the lanes (exact in any order); no LDS, no scratch.  The arithmetic is
// csrc/sdm_track_filter_device.h's: float32, -ffp-contract=off, every operation rounded as written.
#include "sdm_kernels.h"
#include "sdm_track_filter_device.h"

#pragma clang fp contract(off)

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

// state: S x 2L each; masks: what track_commit_kernel wrote for this step's rows; dt: n step times in seconds
__global__ __launch_bounds__(64) void track_filter_kernel(const int* __restrict__ ids, int L, const int* __restrict__ masks,
                                                          const float* __restrict__ dt, TrackFilterParams p, float* __restrict__ x,
                                                          float* __restrict__ state_r, float* __restrict__ state_d,
                                                          float* __restrict__ state_f, int* __restrict__ primed)
{
    const int i = blockIdx.x, lane = threadIdx.x, M = 2 * L;
    const int id = ids[i];
    float* xr = x + (long long)i * M;
    const long long at = (long long)id * M;
    const int action = track_filter_action(masks[i], primed[id]);     // (uniform over the wave)
    float w = 0.0f;
    if (action == TRACK_FILTER_RUN) {
        float x0, x1, y0, y1;
        track_filter_bounds(xr, L, lane, 64, x0, x1, y0, y1);
        w = track_filter_weight(p.beta, wave_min(x0), wave_max(x1), wave_min(y0), wave_max(y1));
    }
    track_filter_row(xr, state_r + at, state_d + at, state_f + at, M, lane, 64, action, dt[i], w, p);
    if (lane == 0) primed[id] = action != TRACK_FILTER_PASS;
}

__global__ void track_filter_unprime_kernel(const int* __restrict__ ids, int n, int* __restrict__ primed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) primed[ids[i]] = 0;
}

__global__ __launch_bounds__(64) void track_filter_get_kernel(const int* __restrict__ ids, int M, const float* __restrict__ state_d,
                                                              const float* __restrict__ state_f, const int* __restrict__ primed,
                                                              float* __restrict__ out_f, float* __restrict__ out_d,
                                                              int* __restrict__ out_primed)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const int id = ids[i];
    const int on = primed[id];
    const long long at = (long long)id * M, to = (long long)i * M;
    for (int j = lane; j < M; j += 64) {
        out_f[to + j] = on ? state_f[at + j] : 0.0f;
        out_d[to + j] = on ? state_d[at + j] : 0.0f;
    }
    if (lane == 0) out_primed[i] = on != 0;
}

}  // namespace

void sdm_launch_track_filter(const int* ids, int n, int L, const int* masks, const float* dt, float min_cutoff, float beta, float d_cutoff,
                             float* x, float* state_r, float* state_d, float* state_f, int* primed, hipStream_t s)
{
    const TrackFilterParams p{min_cutoff, beta, d_cutoff};
    hipLaunchKernelGGL(track_filter_kernel, dim3((unsigned)n), dim3(64), 0, s, ids, L, masks, dt, p, x, state_r, state_d, state_f, primed);
}

void sdm_launch_track_filter_unprime(const int* ids, int n, int* primed, hipStream_t s)
{
    hipLaunchKernelGGL(track_filter_unprime_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, primed);
}

void sdm_launch_track_filter_get(const int* ids, int n, int L, const float* state_d, const float* state_f, const int* primed, float* out_f,
                                 float* out_d, int* out_primed, hipStream_t s)
{
    hipLaunchKernelGGL(track_filter_get_kernel, dim3((unsigned)n), dim3(64), 0, s, ids, 2 * L, state_d, state_f, primed, out_f, out_d,
                       out_primed);
}
