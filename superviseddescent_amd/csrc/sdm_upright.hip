// sdm_upright.hip -- upright-normalised detect and tracking on gfx950 (include/sdm.h, "Rolled faces"): every row's face is cut out of
// its frame as a chip x chip gray image in which it stands upright, the unchanged cascade runs on the stack of chips, and the result
// rows are mapped back into the frame.
//
//   upright_setup_kernel   one wave per row: the rotation (c, s) and the integer centre (ix, iy) -- from the call's box and roll, or
//                          from a tracked slot's eye line and enclosing box --, the chip -> frame matrix M, its inverse W, the row's
//                          frame and the PARTIAL flag as one UprightRow record; the chip's entry of the image table; the row's
//                          initialisation in chip coordinates (align_mean on the chip box, or the realign rule on W p)
//   upright_chip_kernel    one workgroup per 64 x 16 chip pixels, one lane per four consecutive pixels: the taps of a pixel row pair
//                          are one 2-byte load when both lie inside the frame row, byte loads at its ends, 0 outside; four pixels are
//                          one dword store (sdm_align.hip's scheme; the form staged through LDS measured slower:
//                          scripts/experiments/upright_chip_staged_lds.patch)
//   upright_back_kernel    one wave per row: x through M, in place, and the NEAR_EDGE flag
//   upright_slot_cs_kernel (c, s) of started tracker slots
//
// Positions and points are float32 with every operation rounded (-ffp-contract=off, csrc/Makefile): (A00 x + A01 y) + A02.
#include "sdm_kernels.h"
#include "../../include/sdm.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

#define UP_TILE_W 64                  // a workgroup's tile of chip pixels: 16 lanes x 4 pixels wide, 16 rows
#define UP_TILE_H 16
#define UP_MAX_POS 1048576.0f         // 2^20: a position beyond gives 0 (the rule of sdm_align_crops)

__device__ __forceinline__ float up_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float up_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int up_wave_or(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float up_px(const float* m, float x, float y) { return (m[0] * x + m[1] * y) + m[2]; }
__device__ __forceinline__ float up_py(const float* m, float x, float y) { return (m[3] * x + m[4] * y) + m[5]; }

__global__ __launch_bounds__(64) void upright_setup_kernel(UprightSetupDev a, int L, int chip, int cstride, ImageSetDev fr,
                                                           const int* __restrict__ img_idx, EyeIdxDev eyes, UprightRow* __restrict__ rows,
                                                           long long* __restrict__ c_off, int* __restrict__ c_w, int* __restrict__ c_h,
                                                           int* __restrict__ c_stride, float* __restrict__ x, float* __restrict__ init)
{
    const int i = blockIdx.x, lane = threadIdx.x, M = 2 * L, hc = chip / 2;
    float* xo = x + (long long)i * M;
    float* io = init ? init + (long long)i * M : nullptr;
    // (everything up to the record is uniform over the wave)
    const int* box = nullptr;
    const float* prev = nullptr;
    double c = 1.0, s = 0.0;
    // the motion search's shift of a tracked slot's landmarks p, ahead of the roll, the centre and W (csrc/sdm_track_motion.hip)
    const float mx = a.shift ? a.shift[2 * i] : 0.0f, my = a.shift ? a.shift[2 * i + 1] : 0.0f;
    const bool moved = mx != 0.0f || my != 0.0f;
#define UP_PX(j) (moved ? prev[j] + mx : prev[j])
#define UP_PY(j) (moved ? prev[(j) + L] + my : prev[(j) + L])
    if (a.ids) {
        const int id = a.ids[i];
        if (a.slot_status[id] == SDM_TRACK_STARTED) { box = a.slot_box + 4 * id; c = a.slot_cs[2 * id]; s = a.slot_cs[2 * id + 1]; }
        else prev = a.slot_x + (long long)id * M;
    } else {
        box = a.boxes + 4 * i; c = a.cs[2 * i]; s = a.cs[2 * i + 1];
    }
    int ix, iy, bw = 0, bh = 0;
    if (box) {
        bw = box[2]; bh = box[3];
        ix = box[0] + bw / 2; iy = box[1] + bh / 2;
    } else {
        // the roll of a tracked slot: its eye line, the eye centres as device_ied_rows forms them (float32 sums in index order)
        float rx = 0.0f, ry = 0.0f, lx = 0.0f, ly = 0.0f;
        for (int k = 0; k < eyes.nre; ++k) { rx += UP_PX(eyes.re[k]); ry += UP_PY(eyes.re[k]); }
        for (int k = 0; k < eyes.nle; ++k) { lx += UP_PX(eyes.le[k]); ly += UP_PY(eyes.le[k]); }
        rx /= (float)eyes.nre; ry /= (float)eyes.nre;
        lx /= (float)eyes.nle; ly /= (float)eyes.nle;
        const float dxf = lx - rx, dyf = ly - ry;
        const double dx = dxf, dy = dyf;
        const double n = sqrt(dx * dx + dy * dy);
        if (n == 0.0 || !isfinite(n)) { c = 1.0; s = 0.0; }
        else { c = dx / n; s = dy / n; }
        float b0 = INFINITY, b1 = -INFINITY, b2 = INFINITY, b3 = -INFINITY;
        for (int j = lane; j < L; j += 64) {
            const float vx = UP_PX(j), vy = UP_PY(j);
            b0 = fminf(b0, vx); b1 = fmaxf(b1, vx);
            b2 = fminf(b2, vy); b3 = fmaxf(b3, vy);
        }
        b0 = up_wave_min(b0); b1 = up_wave_max(b1); b2 = up_wave_min(b2); b3 = up_wave_max(b3);
        const float cx = fminf(fmaxf((b0 + b1) * 0.5f, -UP_MAX_POS), UP_MAX_POS);
        const float cy = fminf(fmaxf((b2 + b3) * 0.5f, -UP_MAX_POS), UP_MAX_POS);
        ix = (int)floorf(cx); iy = (int)floorf(cy);
    }
    UprightRow r;
    const double dh = (double)hc, dix = (double)ix, diy = (double)iy;
    r.m[0] = (float)c; r.m[1] = (float)(-s); r.m[2] = (float)(dix - (c * dh - s * dh));
    r.m[3] = (float)s; r.m[4] = (float)c;    r.m[5] = (float)(diy - (s * dh + c * dh));
    r.w[0] = (float)c; r.w[1] = (float)s;    r.w[2] = (float)(dh - (c * dix + s * diy));
    r.w[3] = (float)(-s); r.w[4] = (float)c; r.w[5] = (float)(dh - (c * diy - s * dix));
    const int im = img_idx ? img_idx[i] : i;
    r.off = fr.offset[im]; r.iw = fr.w[im]; r.ih = fr.h[im]; r.stride = fr.stride[im];
    // PARTIAL: a chip corner samples outside [0, w - 1] x [0, h - 1] (the rule of SDM_ALIGN_PARTIAL)
    int flags = 0;
    const float cj[2] = {0.0f, (float)(chip - 1)};
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 2; ++v) {
            const float sx = up_px(r.m, cj[u], cj[v]), sy = up_py(r.m, cj[u], cj[v]);
            if (!(sx >= 0.0f && sx <= (float)(r.iw - 1) && sy >= 0.0f && sy <= (float)(r.ih - 1))) flags = SDM_UPRIGHT_PARTIAL;
        }
    r.flags = flags;
    if (lane == 0) {
        rows[i] = r;
        c_off[i] = (long long)i * cstride * chip; c_w[i] = chip; c_h[i] = chip; c_stride[i] = cstride;
    }
    if (box) {
        // align_mean(mean, (hc - w / 2, hc - h / 2, w, h)) in the arithmetic of sdm_apply.hip::init_boxes_kernel
        const int bx = hc - bw / 2, by = hc - bh / 2;
        for (int j = lane; j < M; j += 64) {
            const float m = a.mean[j];
            const float v = j < L ? (m * 1.0f + 0.5f + 0.0f) * (float)bw + (float)bx : (m * 1.0f + 0.5f + 0.0f) * (float)bh + (float)by;
            xo[j] = v;
            if (io) io[j] = v;
        }
    } else {
        // the realign rule of sdm_track.hip on q = W p
        float b0 = INFINITY, b1 = -INFINITY, b2 = INFINITY, b3 = -INFINITY;
        for (int j = lane; j < L; j += 64) {
            const float vx = UP_PX(j), vy = UP_PY(j);
            const float qx = up_px(r.w, vx, vy), qy = up_py(r.w, vx, vy);
            b0 = fminf(b0, qx); b1 = fmaxf(b1, qx);
            b2 = fminf(b2, qy); b3 = fmaxf(b3, qy);
        }
        b0 = up_wave_min(b0); b1 = up_wave_max(b1); b2 = up_wave_min(b2); b3 = up_wave_max(b3);
        const float4 mb = a.mb;
        for (int j = lane; j < M; j += 64) {
            const float m = a.mean[j];
            const float v = j < L ? ((m - mb.x) / (mb.y - mb.x)) * (b1 - b0) + b0 : ((m - mb.z) / (mb.w - mb.z)) * (b3 - b2) + b2;
            xo[j] = v;
            if (io) io[j] = v;
        }
    }
#undef UP_PX
#undef UP_PY
}

// taps (x0, y) and (x0 + 1, y) of one frame row: one 2-byte load when both lie inside the row, byte loads at its ends, 0 outside the
// frame -- no byte outside [row start, row start + width) is touched, whatever the frame's alignment
__device__ __forceinline__ void up_row_pair(const uint8_t* __restrict__ base, const UprightRow& r, int x0, int y, uint32_t& a, uint32_t& b)
{
    a = 0u; b = 0u;
    if (y < 0 || y >= r.ih) return;
    const uint8_t* row = base + (long long)y * r.stride;
    if (x0 >= 0 && x0 + 1 < r.iw) {
        uint16_t t; __builtin_memcpy(&t, row + x0, 2);
        a = t & 255u; b = t >> 8;
        return;
    }
    if (x0 >= 0 && x0 < r.iw) a = row[x0];
    if (x0 + 1 >= 0 && x0 + 1 < r.iw) b = row[x0 + 1];
}

__global__ __launch_bounds__(256) void upright_chip_kernel(const uint8_t* __restrict__ img, const UprightRow* __restrict__ rows, int chip,
                                                           int cstride, int tiles_x, int tiles, uint8_t* __restrict__ chips)
{
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const UprightRow r = rows[n];
    const int i = ty * UP_TILE_H + (threadIdx.x >> 4), j = tx * UP_TILE_W + 4 * (threadIdx.x & 15);
    if (i >= chip || j >= cstride) return;
    const uint8_t* base = img + r.off;
    const float fi = (float)i;
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (j + k >= chip) continue;                        // (the padding of a chip row is written as zeros)
        const float fj = (float)(j + k);
        const float sx = up_px(r.m, fj, fi), sy = up_py(r.m, fj, fi);
        if (!(fabsf(sx) <= UP_MAX_POS) || !(fabsf(sy) <= UP_MAX_POS)) continue;
        const int X = (int)floorf(sx * 32.0f + 0.5f), Y = (int)floorf(sy * 32.0f + 0.5f);
        const int x0 = X >> 5, fx = X & 31, y0 = Y >> 5, fy = Y & 31;
        uint32_t p00, p10, p01, p11;
        up_row_pair(base, r, x0, y0, p00, p10);
        up_row_pair(base, r, x0, y0 + 1, p01, p11);
        const uint32_t w00 = (32 - fx) * (32 - fy), w10 = fx * (32 - fy), w01 = (32 - fx) * fy, w11 = fx * fy;
        word |= ((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 512u) >> 10) << (8 * k);
    }
    *(uint32_t*)(chips + ((long long)n * chip + i) * cstride + j) = word;
}

__global__ __launch_bounds__(64) void upright_back_kernel(UprightRow* __restrict__ rows, int L, int chip, int guard, float* __restrict__ x)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    float* xr = x + (long long)i * 2 * L;
    float m[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) m[e] = rows[i].m[e];
    const float g = (float)guard, hi = (float)(chip - 1);
    int near = 0;
    for (int j = lane; j < L; j += 64) {
        const float qx = xr[j], qy = xr[L + j];
        // NEAR_EDGE: less than `guard` pixels between the landmark and the border of the chip's pixel centres, [0, chip - 1]^2
        near |= !(qx >= g && qy >= g && hi - qx >= g && hi - qy >= g);
        xr[j] = up_px(m, qx, qy);
        xr[L + j] = up_py(m, qx, qy);
    }
    near = up_wave_or(near);
    if (lane == 0 && near) rows[i].flags |= SDM_UPRIGHT_NEAR_EDGE;
}

__global__ void upright_slot_cs_kernel(const int* __restrict__ ids, const double* __restrict__ cs, int n, double* __restrict__ slot_cs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    slot_cs[2 * id] = cs ? cs[2 * i] : 1.0;
    slot_cs[2 * id + 1] = cs ? cs[2 * i + 1] : 0.0;
}

}  // namespace

void sdm_launch_upright_setup(const UprightSetupDev& a, int n, int L, int chip, const ImageSetDev& frames, const int* img_idx,
                              const EyeIdxDev& eyes, UprightRow* rows, long long* chip_off, int* chip_w, int* chip_h, int* chip_stride,
                              float* x, float* init, hipStream_t s)
{
    hipLaunchKernelGGL(upright_setup_kernel, dim3((unsigned)n), dim3(64), 0, s, a, L, chip, sdm_upright_chip_stride(chip), frames, img_idx, eyes,
                       rows, chip_off, chip_w, chip_h, chip_stride, x, init);
}

void sdm_launch_upright_chips(const uint8_t* img, const UprightRow* rows, int n, int chip, uint8_t* chips, hipStream_t s)
{
    const int cstride = sdm_upright_chip_stride(chip);
    const int tiles_x = (cstride + UP_TILE_W - 1) / UP_TILE_W, tiles = tiles_x * ((chip + UP_TILE_H - 1) / UP_TILE_H);
    hipLaunchKernelGGL(upright_chip_kernel, dim3((unsigned)n * (unsigned)tiles), dim3(256), 0, s, img, rows, chip, cstride, tiles_x, tiles, chips);
}

void sdm_launch_upright_back(UprightRow* rows, int n, int L, int chip, int guard, float* x, hipStream_t s)
{
    hipLaunchKernelGGL(upright_back_kernel, dim3((unsigned)n), dim3(64), 0, s, rows, L, chip, guard, x);
}

void sdm_launch_upright_slot_cs(const int* ids, const double* cs, int n, double* slot_cs, hipStream_t s)
{
    hipLaunchKernelGGL(upright_slot_cs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, cs, n, slot_cs);
}
