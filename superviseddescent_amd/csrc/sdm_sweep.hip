// sdm_sweep.hip -- kernels of the regulariser sweep (sdm_capi_sweep.hip): the unregularised normal equations kept beside G while the
// candidates are factored in place, and the held-out / fit score of one candidate's update.
//   Regulariser::get_matrix per candidate   regressors.hpp:126-148  (the reference tunes the one parameter by hand: one whole
//                                           learn() per value, apps/rcr/data/rcr_training_22.cfg)
//   score                                   calculate_normalised_landmark_errors, apps/rcr/rcr-train.cpp:200-212, over a row range
#include "sdm_kernels.h"
#include "sdm_ied.h"

namespace {

#define TILE 128

// ---- snapshot / restore -------------------------------------------------------------------------------------------
// What sdm_gram_rhs writes and the factorisation overwrites: the 128 x 128 tiles with tile row <= tile column of the T factor tile
// rows, and their TR right-hand-side tiles.  They are kept in the exchange buffer's order (sdm_solve.hip, tiles_pack_kernel: tile row
// ti holds the tiles tj >= ti, then the right-hand sides; tile-major, each tile row-major), so a tile is one contiguous 64 KB run
// of the snapshot: a workgroup moves one tile, a lane 16 bytes per step on both sides (a row of a tile = 32 lanes = 512 bytes).
template <bool RESTORE>
__global__ __launch_bounds__(256) void sweep_tiles_kernel(float* __restrict__ G, long long ldg, int T, int TR, float* __restrict__ snap)
{
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj < T && tj < ti) return;                     // (below the diagonal: neither written nor read)
    const long long tile = (long long)ti * (T + TR) - (long long)ti * (ti - 1) / 2 + (tj - ti);
    float4* s = (float4*)(snap + tile * TILE * TILE);
    float* g0 = G + (long long)ti * TILE * ldg + (long long)tj * TILE;
#pragma unroll 4
    for (int e = threadIdx.x; e < TILE * TILE / 4; e += 256) {
        const int r = e / (TILE / 4), c4 = e % (TILE / 4);
        float4* g = (float4*)(g0 + (long long)r * ldg) + c4;
        if (RESTORE) *g = s[e]; else s[e] = *g;
    }
}

// ---- score ---------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: the held-out rows [n_fit, N), 1: the fit rows [0, n_fit).  Element t of a range (row-major over rows x L) is
// summed by a fixed thread of a fixed workgroup, the 256 sums of a workgroup by a fixed tree, the workgroups' sums by index: the
// same bits in every run.  The workgroup that delivers a range's last partial sum adds them up (agent-scope release before the
// ticket, acquire behind it: the partial sums were written on other compute units).
__global__ __launch_bounds__(256) void sweep_score_kernel(const float* __restrict__ x, const float* __restrict__ xstar, int N, int n_fit,
                                                          int L, EyeIdxDev eyes, double* part, unsigned* arrived, double* __restrict__ out)
{
    __shared__ double sh[256];
    const int range = blockIdx.y;
    const int row0 = range == 0 ? n_fit : 0, rows = range == 0 ? N - n_fit : n_fit;
    const long long n = (long long)rows * L;
    double s = 0.0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const int row = row0 + (int)(t / L), i = (int)(t % L);
        const float* xr = x + (long long)row * 2 * L;
        const float* gr = xstar + (long long)row * 2 * L;
        // (landmark_errors_kernel's arithmetic, sdm_apply.hip: f32 differences, squares summed and rooted in double, f32 quotient)
        const double dx = (double)(xr[i] - gr[i]), dy = (double)(xr[i + L] - gr[i + L]);
        const float e = (float)sqrt(dx * dx + dy * dy);
        const float inv = (float)(1.0f / device_ied_rows(xr, L, eyes));
        s += (double)(e * inv);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* mine = part + (size_t)range * gridDim.x;
    mine[blockIdx.x] = sh[0];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(arrived + range, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double total = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) total += mine[b];
    out[range] = n > 0 ? total / (double)n : 0.0;                      // cv::mean
    __hip_atomic_store(arrived + range, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

void sdm_launch_sweep_snapshot(const float* G, long long ldg, int F, int rhs_tiles, float* snap, hipStream_t stream)
{
    const int T = (F + TILE - 1) / TILE;
    hipLaunchKernelGGL(sweep_tiles_kernel<false>, dim3(T + rhs_tiles, T), dim3(256), 0, stream, const_cast<float*>(G), ldg, T, rhs_tiles, snap);
}

void sdm_launch_sweep_restore(float* G, long long ldg, int F, int rhs_tiles, const float* snap, hipStream_t stream)
{
    const int T = (F + TILE - 1) / TILE;
    hipLaunchKernelGGL(sweep_tiles_kernel<true>, dim3(T + rhs_tiles, T), dim3(256), 0, stream, G, ldg, T, rhs_tiles, const_cast<float*>(snap));
}

void sdm_launch_sweep_score(const float* x, const float* xstar, int N, int n_fit, int L, const EyeIdxDev& eyes, double* part,
                            unsigned* arrived, double* out, hipStream_t stream)
{
    // (the counters are cleared ahead of every launch: a launch that did not finish must not leave the next one a wrong ticket)
    (void)hipMemsetAsync(arrived, 0, 2 * sizeof(unsigned), stream);
    hipLaunchKernelGGL(sweep_score_kernel, dim3(SDM_SWEEP_SCORE_PARTS, 2), dim3(256), 0, stream, x, xstar, N, n_fit, L, eyes, part, arrived, out);
}
