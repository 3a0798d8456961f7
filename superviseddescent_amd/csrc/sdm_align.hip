// sdm_align.hip -- aligned face crops on gfx950 (include/sdm.h, sdm_align_*): a similarity fitted to K landmarks of every current
// row, then an integer bilinear warp of the row's image into an out_w x out_h x C crop.
//
//   align_fit_kernel    one lane per row: the least-squares similarity (double), its inverse rounded to float32 (crop -> source),
//                       the flags (DEGENERATE, PARTIAL) and the row's image (offset, size, stride), written as one AlignFace record
//   align_warp_kernel   one lane per 4 consecutive output pixels of the flat N x H x W pixel sequence: 4 C-byte pixels are one
//                       dword (C = 1), three dwords (C = 3) or one dwordx4 (C = 4) store; the taps of a pixel row pair are read with
//                       one load of 2C bytes when both lie inside the image, byte by byte at the border
//
// The positions are float32 with every operation rounded (-ffp-contract=off, csrc/Makefile): sx = (M00 j + M01 i) + M02.
#include "sdm_kernels.h"
#include "../../include/sdm.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

#define ALIGN_BLOCK 256
#define ALIGN_FIT_BLOCK 64            // one wave per 64 rows: 64 workgroups at N = 4 096 (256 rows per workgroup: 14.1 us, 64: 11.3 us)
#define ALIGN_MAX_POS 1048576.0f      // 2^20: a position beyond gives 0

// the row's image: an entry of the context's image set, or of the equally sized external stack
__device__ __forceinline__ void img_of_row(const AlignSourceDev& src, const int* __restrict__ img_idx, int row, AlignFace& f)
{
    const int im = img_idx ? img_idx[row] : row;
    if (src.ctx.base) {
        f.off = src.ctx.offset[im]; f.w = src.ctx.w[im]; f.h = src.ctx.h[im]; f.stride = src.ctx.stride[im];
    } else {
        f.off = (long long)im * src.height * src.stride; f.w = src.width; f.h = src.height; f.stride = src.stride;
    }
}

__global__ __launch_bounds__(ALIGN_FIT_BLOCK) void align_fit_kernel(const float* __restrict__ x, int N, int L, const int* __restrict__ lm,
                                                                const float* __restrict__ tmpl, int K, AlignSourceDev src,
                                                                const int* __restrict__ img_idx, int out_w, int out_h,
                                                                AlignFace* __restrict__ faces)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float* xr = x + (long long)r * 2 * L;
    AlignFace f;
    img_of_row(src, img_idx, r, f);
    // centres of both point sets (double)
    double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0;
    bool finite = true;
    for (int k = 0; k < K; ++k) {
        const float ax = xr[lm[k]], ay = xr[L + lm[k]];
        finite = finite && isfinite(ax) && isfinite(ay);
        px += (double)ax; py += (double)ay;
        qx += (double)tmpl[2 * k]; qy += (double)tmpl[2 * k + 1];
    }
    px /= K; py /= K; qx /= K; qy /= K;
    double spp = 0.0, sa = 0.0, sb = 0.0;
    if (finite) {
        for (int k = 0; k < K; ++k) {
            const double ux = (double)xr[lm[k]] - px, uy = (double)xr[L + lm[k]] - py;
            const double vx = (double)tmpl[2 * k] - qx, vy = (double)tmpl[2 * k + 1] - qy;
            spp += ux * ux + uy * uy;
            sa += ux * vx + uy * vy;
            sb += ux * vy - uy * vx;
        }
    }
    if (!finite || spp == 0.0) {
        for (int e = 0; e < 6; ++e) f.m[e] = __builtin_nanf("");
        f.flags = SDM_ALIGN_DEGENERATE;
        faces[r] = f;
        return;
    }
    // source -> crop: q = A p + t, A = [[a, -b], [b, a]], t = q_bar - A p_bar.  Crop -> source: p = A^-1 q + (p_bar - A^-1 q_bar),
    // A^-1 = [[a, b], [-b, a]] / (a^2 + b^2)
    const double a = sa / spp, b = sb / spp, d = a * a + b * b;
    const double i00 = a / d, i01 = b / d, i10 = -b / d, i11 = a / d;
    f.m[0] = (float)i00; f.m[1] = (float)i01; f.m[2] = (float)(px - (i00 * qx + i01 * qy));
    f.m[3] = (float)i10; f.m[4] = (float)i11; f.m[5] = (float)(py - (i10 * qx + i11 * qy));
    // PARTIAL: a crop corner samples outside [0, w - 1] x [0, h - 1] (the warp's float32 positions)
    int flags = 0;
    const float cj[2] = {0.0f, (float)(out_w - 1)}, ci[2] = {0.0f, (float)(out_h - 1)};
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 2; ++v) {
            const float sx = (f.m[0] * cj[u] + f.m[1] * ci[v]) + f.m[2];
            const float sy = (f.m[3] * cj[u] + f.m[4] * ci[v]) + f.m[5];
            if (!(sx >= 0.0f && sx <= (float)(f.w - 1) && sy >= 0.0f && sy <= (float)(f.h - 1))) flags = SDM_ALIGN_PARTIAL;
        }
    f.flags = flags;
    faces[r] = f;
}

// 2C bytes at p into v (unaligned: the loads are as wide as the byte count allows)
template <int C>
__device__ __forceinline__ void load_pair(const uint8_t* p, uint32_t v[2])
{
    if constexpr (C == 1) {
        uint16_t t; __builtin_memcpy(&t, p, 2); v[0] = t; v[1] = 0;
    } else if constexpr (C == 3) {
        uint32_t lo; uint16_t hi; __builtin_memcpy(&lo, p, 4); __builtin_memcpy(&hi, p + 4, 2); v[0] = lo; v[1] = hi;
    } else {
        uint64_t t; __builtin_memcpy(&t, p, 8); v[0] = (uint32_t)t; v[1] = (uint32_t)(t >> 32);
    }
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t v[2], int b) { return (b < 4 ? v[0] >> (8 * b) : v[1] >> (8 * (b - 4))) & 255u; }

// taps (x0, y) and (x0 + 1, y) of one source row: 2C bytes, 0 outside the image
template <int C>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ img, const AlignFace& f, int x0, int y, uint32_t v[2])
{
    v[0] = 0u; v[1] = 0u;
    if (y < 0 || y >= f.h) return;
    const uint8_t* row = img + f.off + (long long)y * f.stride;
    if (x0 >= 0 && x0 + 1 < f.w) {
        load_pair<C>(row + (long long)x0 * C, v);
        return;
    }
    // border: each tap on its own
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int xx = x0 + t;
        if (xx < 0 || xx >= f.w) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t byte = row[(long long)xx * C + c];
            const int b = t * C + c;
            if (b < 4) v[0] |= byte << (8 * b);
            else v[1] |= byte << (8 * (b - 4));
        }
    }
}

// one output pixel (column j, row i): C channel values
template <int C>
__device__ __forceinline__ void sample(const uint8_t* __restrict__ img, const AlignFace& f, int i, int j, uint32_t out[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0u;
    const float fj = (float)j, fi = (float)i;
    const float sx = (f.m[0] * fj + f.m[1] * fi) + f.m[2];
    const float sy = (f.m[3] * fj + f.m[4] * fi) + f.m[5];
    if (!(fabsf(sx) <= ALIGN_MAX_POS) || !(fabsf(sy) <= ALIGN_MAX_POS)) return;    // (also NaN: a degenerate row's M)
    const int X = (int)floorf(sx * 32.0f + 0.5f), Y = (int)floorf(sy * 32.0f + 0.5f);
    const int x0 = X >> 5, fx = X & 31, y0 = Y >> 5, fy = Y & 31;
    uint32_t r0[2], r1[2];
    load_row<C>(img, f, x0, y0, r0);
    load_row<C>(img, f, x0, y0 + 1, r1);
    const uint32_t w00 = (32 - fx) * (32 - fy), w10 = fx * (32 - fy), w01 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
    for (int c = 0; c < C; ++c)
        out[c] = (w00 * byte_of(r0, c) + w10 * byte_of(r0, C + c) + w01 * byte_of(r1, c) + w11 * byte_of(r1, C + c) + 512u) >> 10;
}

template <int C>
__global__ __launch_bounds__(ALIGN_BLOCK) void align_warp_kernel(const uint8_t* __restrict__ img, const AlignFace* __restrict__ faces, int N,
                                                                 int out_w, int out_h, uint8_t* __restrict__ out)
{
    // face n owns the groups of 4 pixels whose first pixel is one of its own: t in [ceil(n HW / 4), ceil((n + 1) HW / 4))
    const int n = blockIdx.x;
    const long long HW = (long long)out_w * out_h;
    const long long t0 = ((long long)n * HW + 3) >> 2, t1 = ((long long)(n + 1) * HW + 3) >> 2;
    const long long t = t0 + (long long)blockIdx.y * ALIGN_BLOCK + threadIdx.x;
    if (t >= t1) return;
    int loc = (int)(4 * t - (long long)n * HW);          // first pixel's index within face n, [0, HW)
    int i = loc / out_w, j = loc - i * out_w, fn = n;
    const AlignFace fa = faces[n];
    uint32_t px[4][C];
    bool full = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k > 0 && ++j == out_w) { j = 0; if (++i == out_h) { i = 0; ++fn; } }
        if (fn == n) {
            sample<C>(img, fa, i, j, px[k]);
        } else if (fn < N) {                              // the group runs into the next face(s): rare, one lane per face boundary
            const AlignFace fb = faces[fn];
            sample<C>(img, fb, i, j, px[k]);
        } else {
            full = false;                                 // past the last pixel of the stack
#pragma unroll
            for (int c = 0; c < C; ++c) px[k][c] = 0u;
        }
    }
    uint8_t* o = out + 4 * t * C;
    if (full) {
        uint32_t w[C];                                    // 4 pixels x C bytes = C dwords
#pragma unroll
        for (int d = 0; d < C; ++d) {
            uint32_t v = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= px[(4 * d + b) / C][(4 * d + b) % C] << (8 * b);
            w[d] = v;
        }
        if constexpr (C == 1) {
            *(uint32_t*)o = w[0];
        } else if constexpr (C == 3) {
            uint32_t* q = (uint32_t*)o;
            q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
        } else {
            *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        const long long left = (long long)N * HW - 4 * t; // pixels of this group inside the stack (1 .. 3)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < left)
#pragma unroll
                for (int c = 0; c < C; ++c) o[k * C + c] = (uint8_t)px[k][c];
    }
}

}  // namespace

void sdm_launch_align_fit(const float* x, int N, int L, const int* lm, const float* tmpl, int K, const AlignSourceDev& src,
                          const int* img_idx, int out_w, int out_h, AlignFace* faces, hipStream_t s)
{
    hipLaunchKernelGGL(align_fit_kernel, dim3((unsigned)((N + ALIGN_FIT_BLOCK - 1) / ALIGN_FIT_BLOCK)), dim3(ALIGN_FIT_BLOCK), 0, s, x, N, L, lm, tmpl, K, src,
                       img_idx, out_w, out_h, faces);
}

void sdm_launch_align_warp(const uint8_t* img, const AlignFace* faces, int N, int out_w, int out_h, int C, uint8_t* out, hipStream_t s)
{
    const long long HW = (long long)out_w * out_h;
    const long long groups = (HW + 3) / 4 + 1;            // most groups any face owns
    const dim3 grid((unsigned)N, (unsigned)((groups + ALIGN_BLOCK - 1) / ALIGN_BLOCK));
    if (C == 1) hipLaunchKernelGGL(align_warp_kernel<1>, grid, dim3(ALIGN_BLOCK), 0, s, img, faces, N, out_w, out_h, out);
    else if (C == 3) hipLaunchKernelGGL(align_warp_kernel<3>, grid, dim3(ALIGN_BLOCK), 0, s, img, faces, N, out_w, out_h, out);
    else hipLaunchKernelGGL(align_warp_kernel<4>, grid, dim3(ALIGN_BLOCK), 0, s, img, faces, N, out_w, out_h, out);
}
