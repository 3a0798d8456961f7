// sdm_align_tensor_device.h -- the per-pixel arithmetic of the crop tensors (include/sdm.h: sdm_align_crops_tensor, its filtered form and
// sdm_warp_crops_tensor): positions, taps (bytes, and the 16-bit words of P010), the integer bilinear blend, the NV12 conversion (a
// described YUV frame's: sdm_yuv_device.h), the channel rules and the element formula.
// The one pixel fetch of the three calls is here: align_fetch_segment takes four source positions (the warp's, one matrix per pixel),
// align_segment forms them from a row's one matrix, and align_taps is the weighted tap sum under both align_bilinear and the area
// sums of sdm_align_area_device.h.  Plain C++ behind one macro, so the same text is the device code of the kernel frame
// (csrc/sdm_align_tensor_kernel.h) and -- compiled for the host, tests/cpp/align_tensor_host.cpp -- a program that runs under the host
// sanitizers on source buffers of exactly the frames' bytes.
//
// Every float operation is rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off elsewhere); everything
// else is int32 / uint32 arithmetic.
#pragma once
#include "../../include/sdm.h"
#include "sdm_yuv_device.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ALIGN_HD __device__ __forceinline__
#else
#define ALIGN_HD static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define ALIGN_T_MAX_POS 1048576.0f      // 2^20: a position beyond gives 0 (sdm_align_crops' rule)

// one row's source, as the warp reads it
struct AlignRow {
    float m[6];                 // crop -> source
    int w, h, stride;           // plane 0: pixels, rows, bytes per row
    int cstride;                // NV12: bytes per row of the UV plane
    int format;                 // SDM_FRAME_*, a YUV frame's with its matrix and range bits
    const uint8_t* p0;          // plane 0 (gray, Y or interleaved pixels)
    const uint8_t* p1;          // NV12, P010: the interleaved UV plane
    long long pd;               // planar colour: bytes from plane c to plane c + 1, of any sign
};

// SDM_FRAME_BGR_PLANAR | SDM_FRAME_RGB_PLANAR: three planes of one byte per pixel, plane c at p0 + c * pd
ALIGN_HD bool align_planar(int format) { return format == SDM_FRAME_BGR_PLANAR || format == SDM_FRAME_RGB_PLANAR; }
ALIGN_HD bool align_red_first(int format) { return format == SDM_FRAME_RGB || format == SDM_FRAME_RGBA || format == SDM_FRAME_RGB_PLANAR; }

struct AlignPos { int x0, fx, y0, fy; };

// what the element stage and the pastes' decode need: per TENSOR channel scale and bias, the channel order, the colour -> gray weights
struct AlignTensorDev {
    float scale[3], bias[3];
    int order;                  // SDM_ALIGN_ORDER_*
    int wb, wg, wr, gray_shift;
};

// gray_shift and its weight set: sdm_upload_images_bgr_u8's two, 14 (OpenCV 2.4 ... 3.x) or 15 (later releases).  Host code: the C-ABI
// fills the record with it, and so do the host programs of tests/cpp.
static inline void align_gray_weights(int gray_shift, AlignTensorDev& t)
{
    t.gray_shift = gray_shift;
    if (gray_shift == 14) { t.wb = 1868; t.wg = 9617; t.wr = 4899; }
    else { t.wb = 3735; t.wg = 19235; t.wr = 9798; }
}

// 1/32-pixel position of (sx, sy); false: refused by the 2^20 rule (also NaN: a degenerate row's M)
ALIGN_HD bool align_quantise(float sx, float sy, AlignPos& q)
{
    if (!(fabsf(sx) <= ALIGN_T_MAX_POS) || !(fabsf(sy) <= ALIGN_T_MAX_POS)) return false;
    const int X = (int)floorf(sx * 32.0f + 0.5f), Y = (int)floorf(sy * 32.0f + 0.5f);
    q.x0 = X >> 5; q.fx = X & 31; q.y0 = Y >> 5; q.fy = Y & 31;
    return true;
}

// byte offset of (row y, byte xb) inside a plane: 32-bit when the plane's rows * stride fit 31 bits (y < rows, xb < stride)
template <bool WIDE>
ALIGN_HD const uint8_t* align_at(const uint8_t* p, int y, int stride, int xb)
{
    if constexpr (WIDE) return p + ((long long)y * stride + xb);
    else return p + (uint32_t)(y * stride + xb);
}

ALIGN_HD uint32_t align_byte(const uint32_t v[2], int b) { return (b < 4 ? v[0] >> (8 * b) : v[1] >> (8 * (b - 4))) & 255u; }

// the taps (x0, y) and (x0 + 1, y) of a plane of w x h elements of B bytes: 2B bytes packed into v, FILL for a tap outside.  The last
// byte read is the last byte of an element inside the plane.
template <int B, bool WIDE, uint32_t FILL>
ALIGN_HD void align_tap_row(const uint8_t* p, int w, int h, int stride, int x0, int y, uint32_t v[2])
{
    v[0] = FILL * 0x01010101u; v[1] = FILL * 0x01010101u;
    if (y < 0 || y >= h) return;
    if (x0 >= 0 && x0 + 1 < w) {
        const uint8_t* s = align_at<WIDE>(p, y, stride, x0 * B);
        if constexpr (B == 1) {
            uint16_t t; memcpy(&t, s, 2); v[0] = t;
        } else if constexpr (B == 2) {
            uint32_t t; memcpy(&t, s, 4); v[0] = t;
        } else if constexpr (B == 3) {
            uint32_t lo; uint16_t hi; memcpy(&lo, s, 4); memcpy(&hi, s + 4, 2); v[0] = lo; v[1] = hi;
        } else {
            uint32_t lo, hi; memcpy(&lo, s, 4); memcpy(&hi, s + 4, 4); v[0] = lo; v[1] = hi;
        }
        return;
    }
    // border: each tap on its own
    uint32_t a = 0u, b = 0u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int xx = x0 + t;
        const bool in = xx >= 0 && xx < w;
#pragma unroll
        for (int c = 0; c < B; ++c) {
            const uint32_t byte = in ? (uint32_t)*align_at<WIDE>(p, y, stride, xx * B + c) : FILL;
            const int k = t * B + c;
            if (k < 4) a |= byte << (8 * k);
            else b |= byte << (8 * (k - 4));
        }
    }
    v[0] = a; v[1] = b;
}

// the NCH un-rounded sums w00 p00 + w10 p10 + w01 p01 + w11 p11 of the element at q, per byte position: at most 255 * 1024
template <int B, int NCH, bool WIDE, uint32_t FILL>
ALIGN_HD void align_taps(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t sum[NCH])
{
    uint32_t r0[2], r1[2];
    align_tap_row<B, WIDE, FILL>(p, w, h, stride, q.x0, q.y0, r0);
    align_tap_row<B, WIDE, FILL>(p, w, h, stride, q.x0, q.y0 + 1, r1);
    const uint32_t w00 = (32 - q.fx) * (32 - q.fy), w10 = q.fx * (32 - q.fy), w01 = (32 - q.fx) * q.fy, w11 = q.fx * q.fy;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        sum[c] = w00 * align_byte(r0, c) + w10 * align_byte(r0, B + c) + w01 * align_byte(r1, c) + w11 * align_byte(r1, B + c);
}

// NCH values of the element at q: (align_taps + 512) >> 10
template <int B, int NCH, bool WIDE, uint32_t FILL>
ALIGN_HD void align_bilinear(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t out[NCH])
{
    align_taps<B, NCH, WIDE, FILL>(p, w, h, stride, q, out);
#pragma unroll
    for (int c = 0; c < NCH; ++c) out[c] = (out[c] + 512u) >> 10;
}

// P010 ("YUV colour description and 10-bit surfaces"): the taps (x0, y) and (x0 + 1, y) of a plane of w x h elements of E 16-bit words,
// each word >> 6, v[t * E + c]; FILL for a tap outside.  stride in bytes; the last byte read is the last byte of an element inside the
// plane.
template <int E, bool WIDE>
ALIGN_HD void align_tap_row16(const uint8_t* p, int w, int h, int stride, int x0, int y, uint32_t fill, uint32_t v[2 * E])
{
#pragma unroll
    for (int k = 0; k < 2 * E; ++k) v[k] = fill;
    if (y < 0 || y >= h) return;
    if (x0 >= 0 && x0 + 1 < w) {
        const uint8_t* s = align_at<WIDE>(p, y, stride, x0 * 2 * E);
        uint32_t t[E];
        memcpy(t, s, 4 * E);
#pragma unroll
        for (int k = 0; k < E; ++k) { v[2 * k] = (t[k] & 0xffffu) >> 6; v[2 * k + 1] = t[k] >> 22; }
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int xx = x0 + t;
        if (xx < 0 || xx >= w) continue;
#pragma unroll
        for (int c = 0; c < E; ++c) {
            uint16_t word;
            memcpy(&word, align_at<WIDE>(p, y, stride, (xx * E + c) * 2), 2);
            v[t * E + c] = (uint32_t)word >> 6;
        }
    }
}

// align_taps on 10-bit taps: E un-rounded sums, at most 1023 * 1024
template <int E, bool WIDE>
ALIGN_HD void align_taps16(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t fill, uint32_t sum[E])
{
    uint32_t r0[2 * E], r1[2 * E];
    align_tap_row16<E, WIDE>(p, w, h, stride, q.x0, q.y0, fill, r0);
    align_tap_row16<E, WIDE>(p, w, h, stride, q.x0, q.y0 + 1, fill, r1);
    const uint32_t w00 = (32 - q.fx) * (32 - q.fy), w10 = q.fx * (32 - q.fy), w01 = (32 - q.fx) * q.fy, w11 = q.fx * q.fy;
#pragma unroll
    for (int c = 0; c < E; ++c) sum[c] = w00 * r0[c] + w10 * r0[E + c] + w01 * r1[c] + w11 * r1[E + c];
}

template <int E, bool WIDE>
ALIGN_HD void align_bilinear16(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t fill, uint32_t out[E])
{
    align_taps16<E, WIDE>(p, w, h, stride, q, fill, out);
#pragma unroll
    for (int c = 0; c < E; ++c) out[c] = (out[c] + 512u) >> 10;
}

ALIGN_HD uint32_t align_clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// BT.601 limited range, the constants of OpenCV's COLOR_YUV2BGR_NV12 (20 fractional bits).  Every term stays below 2^30 in magnitude:
// y <= 239 * 1220542 = 2.92e8, |1673527 (V - 128)| <= 2.15e8, |2116026 (U - 128)| <= 2.71e8, |852492 (V - 128)| <= 1.10e8,
// |409993 (U - 128)| <= 5.3e7, and every sum below 2^31 (largest: y + 2116026 * 127 + 2^19 = 5.61e8).
ALIGN_HD void align_nv12_to_bgr(uint32_t Y, uint32_t U, uint32_t V, uint32_t bgr[3])
{
    const int yy = (int)Y - 16, y = (yy < 0 ? 0 : yy) * 1220542, u = (int)U - 128, v = (int)V - 128;
    bgr[0] = align_clamp255((y + 2116026 * u + (1 << 19)) >> 20);
    bgr[1] = align_clamp255((y - 852492 * v - 409993 * u + (1 << 19)) >> 20);
    bgr[2] = align_clamp255((y + 1673527 * v + (1 << 19)) >> 20);
}

// the warped pixel of up to 4 crop pixels at the source positions (sx[k], sy[k]) as (B, G, R); a gray source gives (g, g, g).  A pixel with
// on[k] false is (0, 0, 0) and reads no source byte.  The source format is switched on once, outside the pixel work.  r.m is not used.
template <bool WIDE>
ALIGN_HD void align_fetch_segment(const AlignRow& r, const float sx[4], const float sy[4], const bool on[4], uint32_t px[4][3])
{
    AlignPos q[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[k].x0 = q[k].fx = q[k].y0 = q[k].fy = 0;
        ok[k] = on[k] && align_quantise(sx[k], sy[k], q[k]);
        px[k][0] = px[k][1] = px[k][2] = 0u;
    }
    switch (SDM_FRAME_BASE(r.format)) {
    case SDM_FRAME_GRAY:
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) {
                uint32_t g[1];
                align_bilinear<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], g);
                px[k][0] = px[k][1] = px[k][2] = g[0];
            }
        break;
    case SDM_FRAME_BGR: case SDM_FRAME_RGB:
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) align_bilinear<3, 3, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], px[k]);
        break;
    case SDM_FRAME_BGRA: case SDM_FRAME_RGBA:
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) align_bilinear<4, 3, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], px[k]);
        break;
    case SDM_FRAME_BGR_PLANAR: case SDM_FRAME_RGB_PLANAR: {
        // the plane distance goes on the pointer in 64 bits; the offsets inside each plane are a one-byte format's
        const uint8_t* const pl1 = r.p0 + r.pd;
        const uint8_t* const pl2 = pl1 + r.pd;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) {
                align_bilinear<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], px[k]);
                align_bilinear<1, 1, WIDE, 0u>(pl1, r.w, r.h, r.stride, q[k], px[k] + 1);
                align_bilinear<1, 1, WIDE, 0u>(pl2, r.w, r.h, r.stride, q[k], px[k] + 2);
            }
        break;
    }
    case SDM_FRAME_P010: {
        // 10-bit taps, the decode of the frame's description; a one-channel tensor takes the luma alone
        const int cw = (r.w + 1) >> 1, ch = (r.h + 1) >> 1;
        const bool luma = (r.format & YUV_LUMA_ONLY) != 0;
        const YuvDecode t = yuv_tables.dec[yuv_decode_row(r.format)];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) {
                uint32_t y[1], uv[2] = {512u, 512u};
                align_bilinear16<1, WIDE>(r.p0, r.w, r.h, r.stride, q[k], 0u, y);
                if (luma) { px[k][0] = px[k][1] = px[k][2] = yuv_luma8_of_10(y[0]); continue; }
                AlignPos qc;
                if (align_quantise(sx[k] * 0.5f, sy[k] * 0.5f, qc))
                    align_bilinear16<2, WIDE>(r.p1, cw, ch, r.cstride, qc, 512u, uv);
                yuv_to_bgr(t, y[0], uv[0], uv[1], px[k]);
            }
        break;
    }
    default: {   // SDM_FRAME_NV12: value 5 with the constants it always had, a described frame with its table row
        const int cw = (r.w + 1) >> 1, ch = (r.h + 1) >> 1;
        if (r.format == SDM_FRAME_NV12) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    uint32_t y[1], uv[2] = {128u, 128u};
                    align_bilinear<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], y);
                    AlignPos qc;
                    if (align_quantise(sx[k] * 0.5f, sy[k] * 0.5f, qc))       // (exact halves: never refused behind an accepted luma position)
                        align_bilinear<2, 2, WIDE, 128u>(r.p1, cw, ch, r.cstride, qc, uv);
                    align_nv12_to_bgr(y[0], uv[0], uv[1], px[k]);
                }
            break;
        }
        const YuvDecode t = yuv_tables.dec[yuv_decode_row(r.format)];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k]) {
                uint32_t y[1], uv[2] = {128u, 128u};
                align_bilinear<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q[k], y);
                AlignPos qc;
                if (align_quantise(sx[k] * 0.5f, sy[k] * 0.5f, qc))
                    align_bilinear<2, 2, WIDE, 128u>(r.p1, cw, ch, r.cstride, qc, uv);
                yuv_to_bgr(t, y[0], uv[0], uv[1], px[k]);
            }
        break;
    }
    }
    if (align_red_first(r.format)) {                                        // byte 0 / plane 0 is R: (B, G, R) by byte position
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint32_t t = px[k][0]; px[k][0] = px[k][2]; px[k][2] = t; }
    }
}

// align_fetch_segment for the consecutive crop pixels (row i, columns j0 ... j0 + npx - 1) of a similarity row: the positions through r.m,
// the products M01 i, M11 i shared
template <bool WIDE>
ALIGN_HD void align_segment(const AlignRow& r, int i, int j0, int npx, uint32_t px[4][3])
{
    const float fi = (float)i;
    const float ax = r.m[1] * fi, ay = r.m[4] * fi;
    float sx[4], sy[4];
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fj = (float)(j0 + k);
        sx[k] = (r.m[0] * fj + ax) + r.m[2];
        sy[k] = (r.m[3] * fj + ay) + r.m[5];
        on[k] = k < npx;
    }
    align_fetch_segment<WIDE>(r, sx, sy, on, px);
}

// output channel c of CH from a warped (B, G, R); weigh: the source is BGR / RGB / BGRA / RGBA or planar colour (a gray or luma-only
// value passes)
template <int CH>
ALIGN_HD uint32_t align_channel(const uint32_t bgr[3], int c, bool weigh, int order, int wb, int wg, int wr, int shift)
{
    if constexpr (CH == 3) return order == SDM_ALIGN_ORDER_RGB ? bgr[2 - c] : bgr[c];
    else return weigh ? (bgr[0] * wb + bgr[1] * wg + bgr[2] * wr + (1u << (shift - 1))) >> shift : bgr[0];
}

// (float)v * scale + bias: the product rounded, then the sum rounded
ALIGN_HD float align_element(uint32_t v, float scale, float bias)
{
    const float p = (float)v * scale;
    return p + bias;
}
