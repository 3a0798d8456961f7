// sdm_track_motion.hip -- the tracker's motion-compensated initialisation on gfx950 (include/sdm.h, "Tracking, motion-compensated"):
// a block-matching estimate of each stream's translation between its last frame and the new one, taken before the cascade runs.
//
//   track_motion_store_kernel    behind track_commit_kernel: for a tracked row the grid (k, ox, oy) around its committed landmarks and
//                                the 32 x 32 chip of k x k block means there, into the slot's state; a lost row invalidates its slot
//   track_motion_search_kernel   ahead of the gather: for a TRACKED slot with a valid chip the window of (32 + 2S)^2 block means on the
//                                stored grid in the NEW image, the SAD of the chip at every offset in [-S, S]^2, the arg-min on
//                                (SAD, dx^2 + dy^2, dy, dx) and the acceptance rule; the row's shift in pixels for the gather
//
// One workgroup of 256 lanes per row.  Block means, one cell row at a time: every lane sums the k taps of a pixel column -- consecutive
// lanes read consecutive bytes of a frame row, whatever k --, the column sums go through LDS, four lanes add a cell's k sums and two
// shuffles join them.  The window and the chip stay in LDS as bytes; an offset's SAD reads nine aligned words per chip row, re-aligns
// them by v_alignbyte_b32 and takes four pixels per v_sad_u8.  The offsets are spread over the lanes; the arg-min is a wave reduction
// on the packed key and one pass over the four waves' results.  No scratch; offsets into a frame are 64-bit; a tap is guarded by the
// image's own width and height.  The arithmetic is csrc/sdm_track_motion_device.h's.
#include "sdm_kernels.h"
#include "../../include/sdm.h"
#include "sdm_track_motion_device.h"

#pragma clang fp contract(off)

namespace {

#define TM_LANES 256
#define TM_WINDOW_MAX (TRACK_MOTION_C + 2 * TRACK_MOTION_MAX_S)      // 64 cells

__device__ __forceinline__ float tm_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float tm_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ TrackMotionImage tm_image(const ImageSetDev& fr, const int* __restrict__ img_idx, int i)
{
    const int im = img_idx ? img_idx[i] : i;
    TrackMotionImage r;
    r.p = fr.base + fr.offset[im]; r.w = fr.w[im]; r.h = fr.h[im]; r.stride = fr.stride[im];
    return r;
}

// n x n cells (n <= 64) from the pixel origin (X0, Y0) into `out`, `pitch` bytes per row; colsum: n k ints of LDS
__device__ __forceinline__ void tm_build_cells(const TrackMotionImage& im, int X0, int Y0, int k, int n, uint8_t* out, int pitch, int* colsum)
{
    const int lane = threadIdx.x, c = lane >> 2, q = lane & 3, npx = n * k;
    for (int r = 0; r < n; ++r) {
        track_motion_columns(im, X0, Y0 + r * k, k, npx, lane, TM_LANES, colsum);
        __syncthreads();
        int s = c < n ? track_motion_cell_part(colsum, c, q, k) : 0;
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (c < n && q == 0) out[r * pitch + c] = track_motion_mean(s, k);
        __syncthreads();
    }
}

// state: per slot {valid, k, ox, oy}; chips: per slot 32 x 32 bytes; x: the step's committed raw rows, masks: the commit's
__global__ __launch_bounds__(TM_LANES) void track_motion_store_kernel(const int* __restrict__ ids, int L, const float* __restrict__ x,
                                                                      const int* __restrict__ masks, ImageSetDev fr,
                                                                      const int* __restrict__ img_idx, float scale, int* __restrict__ state,
                                                                      uint8_t* __restrict__ chips)
{
    __shared__ int colsum[TRACK_MOTION_C * TRACK_MOTION_MAX_K];
    __shared__ uint32_t chip[TRACK_MOTION_C * TRACK_MOTION_C / 4];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int id = ids[i];
    if (masks[i] != 0) {                          // (uniform over the workgroup)
        if (lane == 0) state[4 * id] = 0;
        return;
    }
    // the row's enclosing box, in every wave
    const float* xr = x + (long long)i * 2 * L;
    float a = INFINITY, b = -INFINITY, c = INFINITY, d = -INFINITY;
    for (int j = lane & 63; j < L; j += 64) {
        const float vx = xr[j], vy = xr[L + j];
        a = fminf(a, vx); b = fmaxf(b, vx);
        c = fminf(c, vy); d = fmaxf(d, vy);
    }
    const TrackMotionGrid g = track_motion_grid(tm_wave_min(a), tm_wave_max(b), tm_wave_min(c), tm_wave_max(d), scale);
    const TrackMotionImage im = tm_image(fr, img_idx, i);
    tm_build_cells(im, g.ox, g.oy, g.k, TRACK_MOTION_C, (uint8_t*)chip, TRACK_MOTION_C, colsum);
    ((uint32_t*)(chips + (long long)id * TRACK_MOTION_C * TRACK_MOTION_C))[lane] = chip[lane];
    if (lane == 0) { state[4 * id] = 1; state[4 * id + 1] = g.k; state[4 * id + 2] = g.ox; state[4 * id + 3] = g.oy; }
}

// shift: n x 2 floats for the gather; last: per slot {dx_px, dy_px, sad_best, sad_zero, k, searched}
__global__ __launch_bounds__(TM_LANES) void track_motion_search_kernel(const int* __restrict__ ids, const int* __restrict__ slot_status,
                                                                       const int* __restrict__ state, const uint8_t* __restrict__ chips,
                                                                       ImageSetDev fr, const int* __restrict__ img_idx, int S, int min_gain,
                                                                       float* __restrict__ shift, int* __restrict__ last)
{
    __shared__ int colsum[TM_WINDOW_MAX * TRACK_MOTION_MAX_K];
    __shared__ uint32_t cur[(TM_WINDOW_MAX + 4) * TM_WINDOW_MAX / 4];
    __shared__ uint32_t ref[TRACK_MOTION_C * TRACK_MOTION_C / 4];
    __shared__ unsigned long long wave_best[TM_LANES / 64];
    __shared__ int sad_zero;
    const int i = blockIdx.x, lane = threadIdx.x;
    const int id = ids[i];
    const int* st = state + 4 * id;
    if (slot_status[id] != SDM_TRACK_TRACKED || st[0] == 0) {      // (uniform over the workgroup)
        if (lane == 0) {
            shift[2 * i] = 0.0f; shift[2 * i + 1] = 0.0f;
            for (int e = 0; e < 6; ++e) last[6 * id + e] = 0;
        }
        return;
    }
    const int k = st[1], ox = st[2], oy = st[3];
    ref[lane] = ((const uint32_t*)(chips + (long long)id * TRACK_MOTION_C * TRACK_MOTION_C))[lane];
    const TrackMotionImage im = tm_image(fr, img_idx, i);
    tm_build_cells(im, ox - S * k, oy - S * k, k, track_motion_window(S), (uint8_t*)cur, track_motion_pitch(S), colsum);
    unsigned long long best = track_motion_search(cur, ref, S, lane, TM_LANES, &sad_zero);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if ((lane & 63) == 0) wave_best[lane >> 6] = best;
    __syncthreads();
    if (lane != 0) return;
    for (int w = 1; w < TM_LANES / 64; ++w) best = wave_best[w] < best ? wave_best[w] : best;
    const int sad = track_motion_key_sad(best), zero = sad_zero;
    const bool take = track_motion_accept(sad, zero, min_gain);
    const int dx = take ? track_motion_key_dx(best) * k : 0, dy = take ? track_motion_key_dy(best) * k : 0;
    shift[2 * i] = (float)dx; shift[2 * i + 1] = (float)dy;
    int* o = last + 6 * id;
    o[0] = dx; o[1] = dy; o[2] = sad; o[3] = zero; o[4] = k; o[5] = 1;
}

__global__ void track_motion_invalidate_kernel(const int* __restrict__ ids, int n, int* __restrict__ state)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) state[4 * ids[i]] = 0;
}

// the named slots' last results, grids and chips in ids order
__global__ __launch_bounds__(TM_LANES) void track_motion_get_kernel(const int* __restrict__ ids, const int* __restrict__ state,
                                                                    const uint8_t* __restrict__ chips, const int* __restrict__ last,
                                                                    int* __restrict__ out_motion, int* __restrict__ out_grid,
                                                                    uint8_t* __restrict__ out_chips)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const int id = ids[i];
    const int valid = state[4 * id];
    if (lane < 6) out_motion[6 * i + lane] = last[6 * id + lane];
    if (lane < 3) out_grid[3 * i + lane] = valid ? state[4 * id + 1 + lane] : 0;
    ((uint32_t*)out_chips)[(long long)i * TM_LANES + lane] = valid ? ((const uint32_t*)chips)[(long long)id * TM_LANES + lane] : 0u;
}

}  // namespace

void sdm_launch_track_motion_store(const int* ids, int n, int L, const float* x, const int* masks, const ImageSetDev& frames,
                                   const int* img_idx, float scale, int* state, uint8_t* chips, hipStream_t s)
{
    hipLaunchKernelGGL(track_motion_store_kernel, dim3((unsigned)n), dim3(TM_LANES), 0, s, ids, L, x, masks, frames, img_idx, scale, state, chips);
}

void sdm_launch_track_motion_search(const int* ids, int n, const int* slot_status, const int* state, const uint8_t* chips,
                                    const ImageSetDev& frames, const int* img_idx, int search, int min_gain, float* shift, int* last,
                                    hipStream_t s)
{
    hipLaunchKernelGGL(track_motion_search_kernel, dim3((unsigned)n), dim3(TM_LANES), 0, s, ids, slot_status, state, chips, frames, img_idx,
                       search, min_gain, shift, last);
}

void sdm_launch_track_motion_invalidate(const int* ids, int n, int* state, hipStream_t s)
{
    hipLaunchKernelGGL(track_motion_invalidate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, state);
}

void sdm_launch_track_motion_get(const int* ids, int n, const int* state, const uint8_t* chips, const int* last, int* out_motion,
                                 int* out_grid, uint8_t* out_chips, hipStream_t s)
{
    hipLaunchKernelGGL(track_motion_get_kernel, dim3((unsigned)n), dim3(TM_LANES), 0, s, ids, state, chips, last, out_motion, out_grid,
                       out_chips);
}
