// sdm_yuv_device.h -- the colour description of a YUV frame (include/sdm.h, "YUV colour description and 10-bit surfaces"): the matrix
// and range bits of sdm_frame.format, the Q20 constants of every (matrix, range, depth) derived by one rule from Kr and Kb, the decode
// (Y, U, V) -> (B, G, R) of the crop tensors and the encode (B, G, R) -> (Y, U, V) of the pastes.  SDM_FRAME_NV12 without a flag
// (value 5) is a table row of its own: OpenCV's three-decimal BT.601 constants, the bits of align_nv12_to_bgr, paste_nv12_luma and
// paste_nv12_chroma.  Plain C++ behind YUV_HD: device code, and -- compiled for the host -- the programs of tests/cpp.
//
// The tables are built by the compiler (IEEE double, floor(c * 2^20 + 0.5)) and sit in constant memory; a frame's format is uniform for
// a workgroup, so a kernel reads its row with scalar loads, once, outside the pixel work.  Everything is int32 / uint32 arithmetic.
#pragma once
#include "../../include/sdm.h"

#include <stdint.h>

#if defined(__HIPCC__)
#define YUV_HD __device__ __forceinline__
#else
#define YUV_HD static inline
#endif

#define SDM_FRAME_MATRIX(f) (((f) >> 8) & 15)          // 0: BT.601, 1: BT.709, 2: BT.2020 (non-constant luminance)
#define SDM_FRAME_FULL(f)   (((f) >> 12) & 1)
// bits a caller may set: the base, the matrix field and the range bit
#define SDM_FRAME_PUBLIC_BITS 0x1fff
// (inside the crop kernels only, never in a caller's sdm_frame) a one-channel tensor from a P010 frame: the luma alone, UV never read
#define YUV_LUMA_ONLY 0x10000

// decode: y = max(Y - y0, 0) cy, u = U - c0, v = V - c0; R = (y + cvr v + 2^19) >> 20, B = (y + cub u + 2^19) >> 20,
// G = (y - cvg v - cug u + 2^19) >> 20, each clamped to 0 ... 255
struct YuvDecode { int cy, cvr, cub, cvg, cug, y0, c0; };
// encode (8 bits): Y = (yr R + yg G + yb B + (y0 << 20) + 2^19) >> 20, U = (ub B - ug G - ur R + (128 << 20) + 2^19) >> 20,
// V = (vr R - vg G - vb B + (128 << 20) + 2^19) >> 20, U and V clamped
struct YuvEncode { int yr, yg, yb, y0, ub, ug, ur, vr, vg, vb; };

// Row 0 of either table -- BT.601 limited range at 8 bits by the one rule -- is reached by no format: SDM_FRAME_NV12 |
// SDM_FRAME_YUV_BT601 without the range bit IS value 5 and takes the last row.  It stays so that a row's index is a plain function of
// the bits, and the host program of tests/cpp checks it like the others.
#define YUV_DECODE_ROWS 13          // depth (8, 10) x matrix x range, then value 5's
#define YUV_DECODE_PLAIN 12
#define YUV_ENCODE_ROWS 7           // matrix x range, then value 5's
#define YUV_ENCODE_PLAIN 6
struct YuvTables { YuvDecode dec[YUV_DECODE_ROWS]; YuvEncode enc[YUV_ENCODE_ROWS]; };

constexpr int yuv_q20(double c) { return (int)(long long)(c * 1048576.0 + 0.5); }          // (c > 0: the cast is the floor)

constexpr YuvTables yuv_make_tables()
{
    YuvTables t{};
    const double kr[3] = {0.299, 0.2126, 0.2627}, kb[3] = {0.114, 0.0722, 0.0593};
    for (int m = 0; m < 3; ++m) {
        const double Kr = kr[m], Kb = kb[m], Kg = 1.0 - Kr - Kb;
        for (int full = 0; full < 2; ++full) {
            for (int deep = 0; deep < 2; ++deep) {
                const int d = deep ? 10 : 8;
                const double one = (double)(1 << (d - 8));
                const double ys = full ? 255.0 / (double)((1 << d) - 1) : 255.0 / (219.0 * one);
                const double cs = full ? 255.0 / (double)((1 << d) - 1) : 255.0 / (224.0 * one);
                YuvDecode& e = t.dec[deep * 6 + m * 2 + full];
                e.cy = yuv_q20(ys);
                e.cvr = yuv_q20(2.0 * (1.0 - Kr) * cs);
                e.cub = yuv_q20(2.0 * (1.0 - Kb) * cs);
                e.cvg = yuv_q20(2.0 * Kr * (1.0 - Kr) / Kg * cs);
                e.cug = yuv_q20(2.0 * Kb * (1.0 - Kb) / Kg * cs);
                e.y0 = full ? 0 : 16 << (d - 8);
                e.c0 = 1 << (d - 1);
            }
            const double sy = full ? 1.0 : 219.0 / 255.0, sc = full ? 1.0 : 224.0 / 255.0;
            YuvEncode& e = t.enc[m * 2 + full];
            e.yr = yuv_q20(Kr * sy); e.yg = yuv_q20(Kg * sy); e.yb = yuv_q20(Kb * sy);
            e.y0 = full ? 0 : 16;
            e.ub = yuv_q20(0.5 * sc); e.ug = yuv_q20(0.5 * Kg / (1.0 - Kb) * sc); e.ur = yuv_q20(0.5 * Kr / (1.0 - Kb) * sc);
            e.vr = yuv_q20(0.5 * sc); e.vg = yuv_q20(0.5 * Kg / (1.0 - Kr) * sc); e.vb = yuv_q20(0.5 * Kb / (1.0 - Kr) * sc);
        }
    }
    // value 5: OpenCV's COLOR_YUV2BGR_NV12 and its counterpart, as they always were
    t.dec[YUV_DECODE_PLAIN] = YuvDecode{1220542, 1673527, 2116026, 852492, 409993, 16, 128};
    t.enc[YUV_ENCODE_PLAIN] = YuvEncode{269484, 528482, 102760, 16, 460324, 305135, 155188, 460324, 385875, 74448};
    return t;
}
#if defined(__HIPCC__)
static __constant__ const YuvTables yuv_tables = yuv_make_tables();
#else
static const YuvTables yuv_tables = yuv_make_tables();
#endif

// the table rows of a checked format (base NV12 or P010): value 5 has its own
YUV_HD int yuv_decode_row(int format)
{
    if ((format & SDM_FRAME_PUBLIC_BITS) == SDM_FRAME_NV12) return YUV_DECODE_PLAIN;
    return (SDM_FRAME_BASE(format) == SDM_FRAME_P010 ? 6 : 0) + SDM_FRAME_MATRIX(format) * 2 + SDM_FRAME_FULL(format);
}
YUV_HD int yuv_encode_row(int format)
{
    if ((format & SDM_FRAME_PUBLIC_BITS) == SDM_FRAME_NV12) return YUV_ENCODE_PLAIN;
    return SDM_FRAME_MATRIX(format) * 2 + SDM_FRAME_FULL(format);
}

YUV_HD uint32_t yuv_clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// (Y, U, V) of t's depth -> 8-bit (B, G, R).  Every sum stays below 2^31: the largest, BT.2020 limited at 10 bits, is
// 1007 * 305236 + 561464 * 512 + 2^19 = 5.96e8
YUV_HD void yuv_to_bgr(const YuvDecode& t, uint32_t Y, uint32_t U, uint32_t V, uint32_t bgr[3])
{
    const int yy = (int)Y - t.y0, y = (yy < 0 ? 0 : yy) * t.cy, u = (int)U - t.c0, v = (int)V - t.c0;
    bgr[0] = yuv_clamp255((y + t.cub * u + (1 << 19)) >> 20);
    bgr[1] = yuv_clamp255((y - t.cvg * v - t.cug * u + (1 << 19)) >> 20);
    bgr[2] = yuv_clamp255((y + t.cvr * v + (1 << 19)) >> 20);
}

// 8-bit luma of a 10-bit one (the image set and one-channel tensors of a P010 frame)
YUV_HD uint32_t yuv_luma8_of_10(uint32_t y10) { const uint32_t v = (y10 + 2u) >> 2; return v > 255u ? 255u : v; }

YUV_HD uint32_t yuv_luma(const YuvEncode& t, const uint32_t bgr[3])
{
    return ((uint32_t)t.yr * bgr[2] + (uint32_t)t.yg * bgr[1] + (uint32_t)t.yb * bgr[0] + ((uint32_t)t.y0 << 20) + (1u << 19)) >> 20;
}

YUV_HD void yuv_chroma(const YuvEncode& t, const uint32_t m[3], uint32_t& u, uint32_t& v)
{
    const int b = (int)m[0], g = (int)m[1], r = (int)m[2];
    u = yuv_clamp255((t.ub * b - t.ug * g - t.ur * r + (128 << 20) + (1 << 19)) >> 20);
    v = yuv_clamp255((t.vr * r - t.vg * g - t.vb * b + (128 << 20) + (1 << 19)) >> 20);
}
