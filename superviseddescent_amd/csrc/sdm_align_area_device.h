// sdm_align_area_device.h -- the per-pixel arithmetic of sdm_align_crops_tensor_filtered (include/sdm.h) where a row minifies: S of a
// row, the sub-sample offsets, the un-rounded bilinear value q of a sub-sample and the average of S x S of them.  Built on
// sdm_align_tensor_device.h (quantisation, the tap sum align_taps, NV12 conversion), plain C++ behind ALIGN_HD like it: the device code of
// csrc/sdm_align_area.hip and -- compiled for the host, tests/cpp/align_area_host.cpp -- a program that runs under the host sanitizers.
//
// Float operations are rounded one by one (no contraction); sums and the average are uint32.
#pragma once
#include "sdm_align_tensor_device.h"

#include <float.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define ALIGN_AREA_MAX_S 16

// o[u] = (float)(2u + 1 - S) / (float)(2S) for S = 1 ... 16, S's entries at S (S - 1) / 2: divided by the compiler (IEEE, correctly
// rounded), so the device divides nothing
struct AlignAreaOffsets { float o[ALIGN_AREA_MAX_S * (ALIGN_AREA_MAX_S + 1) / 2]; };
constexpr AlignAreaOffsets align_area_make_offsets()
{
    AlignAreaOffsets t{};
    for (int S = 1; S <= ALIGN_AREA_MAX_S; ++S)
        for (int u = 0; u < S; ++u) t.o[S * (S - 1) / 2 + u] = (float)(2 * u + 1 - S) / (float)(2 * S);
    return t;
}
#if defined(__HIPCC__)
static __constant__ const AlignAreaOffsets align_area_offsets = align_area_make_offsets();
#else
static const AlignAreaOffsets align_area_offsets = align_area_make_offsets();
#endif

// S of a row: 1 for mode BILINEAR, a DEGENERATE row, s2 = M00^2 + M10^2 below min2 = min_scale^2 (float32) or not finite; else the
// smallest S in [1, max_samples] with (float)(S S) >= s2, max_samples when there is none
ALIGN_HD int align_area_samples(const float m[6], int flags, int mode, int max_samples, float min2)
{
    if (mode != SDM_ALIGN_FILTER_AREA || (flags & SDM_ALIGN_DEGENERATE)) return 1;
    const float a = m[0] * m[0], b = m[3] * m[3];
    const float s2 = a + b;
    if (!(s2 >= min2) || !(s2 <= FLT_MAX)) return 1;          // (NaN fails the first test, inf the second)
    int S = 1;
    while (S < max_samples && (float)(S * S) < s2) ++S;
    return S;
}

// x / d for x < 2^16 (10-bit taps: x < 2^18) and d in [2, 256]: the high word of x * ceil(2^32 / d).  Exact: with
// e = ceil(2^32 / d) d - 2^32 < d the high word is floor(x / d + x e / (2^32 d)), and x e < 2^24 (2^26) keeps the second term below the
// 1 / d that x / d lacks to the next integer.
ALIGN_HD uint32_t align_area_reciprocal(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }
ALIGN_HD uint32_t align_area_divide(uint32_t x, uint32_t rcp) { return (uint32_t)(((uint64_t)x * rcp) >> 32); }

// (sum of S S values q <= 255 * 1024 + 512 S S) / (1024 S S): the sum stays below 2^26 + 2^17, the shifted sum below 2^16 (P010, q <=
// 1023 * 1024: below 2^28 + 2^17 and 2^18)
ALIGN_HD uint32_t align_area_average(uint32_t sum, uint32_t n, uint32_t rcp) { return align_area_divide((sum + 512u * n) >> 10, rcp); }

// the NCH un-rounded values q of the element at q (align_taps), added to acc
template <int B, int NCH, bool WIDE, uint32_t FILL>
ALIGN_HD void align_area_add(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t acc[NCH])
{
    uint32_t v[NCH];
    align_taps<B, NCH, WIDE, FILL>(p, w, h, stride, q, v);
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] += v[c];
}

// align_area_add on the 10-bit taps of a P010 plane (E words per element)
template <int E, bool WIDE>
ALIGN_HD void align_area_add16(const uint8_t* p, int w, int h, int stride, const AlignPos& q, uint32_t fill, uint32_t acc[E])
{
    uint32_t v[E];
    align_taps16<E, WIDE>(p, w, h, stride, q, fill, v);
#pragma unroll
    for (int c = 0; c < E; ++c) acc[c] += v[c];
}

// KIND: the source as the taps see it
#define ALIGN_AREA_GRAY 0
#define ALIGN_AREA_BGR  1      // 3 bytes per pixel
#define ALIGN_AREA_BGRA 2      // 4 bytes per pixel, the fourth never read
#define ALIGN_AREA_NV12 3
#define ALIGN_AREA_PLANAR 4    // three planes of 1 byte per pixel, r.pd apart
#define ALIGN_AREA_P010 5      // 10-bit taps: sums of at most 256 values <= 1023 * 1024, below 2^32
#define ALIGN_AREA_P010_LUMA 6 // a one-channel tensor: the luma plane alone

// KIND of a row's format
ALIGN_HD int align_area_kind(int format)
{
    switch (SDM_FRAME_BASE(format)) {
    case SDM_FRAME_GRAY: return ALIGN_AREA_GRAY;
    case SDM_FRAME_BGR: case SDM_FRAME_RGB: return ALIGN_AREA_BGR;
    case SDM_FRAME_BGRA: case SDM_FRAME_RGBA: return ALIGN_AREA_BGRA;
    case SDM_FRAME_BGR_PLANAR: case SDM_FRAME_RGB_PLANAR: return ALIGN_AREA_PLANAR;
    case SDM_FRAME_P010: return (format & YUV_LUMA_ONLY) ? ALIGN_AREA_P010_LUMA : ALIGN_AREA_P010;
    default: return ALIGN_AREA_NV12;
    }
}

// the averaged values a of one pixel -- (g, -, -), (byte 0, 1, 2) or (Y, U, V) -- as (B, G, R): a YUV source is converted once, value 5
// with the constants it always had
ALIGN_HD void align_area_finish(int format, const uint32_t a[3], uint32_t px[3])
{
    const int base = SDM_FRAME_BASE(format);
    if (base == SDM_FRAME_GRAY) px[0] = px[1] = px[2] = a[0];
    else if (format == SDM_FRAME_NV12) align_nv12_to_bgr(a[0], a[1], a[2], px);
    else if (format & YUV_LUMA_ONLY) px[0] = px[1] = px[2] = yuv_luma8_of_10(a[0]);
    else if (base == SDM_FRAME_NV12 || base == SDM_FRAME_P010) yuv_to_bgr(yuv_tables.dec[yuv_decode_row(format)], a[0], a[1], a[2], px);
    else if (align_red_first(format)) { px[0] = a[2]; px[1] = a[1]; px[2] = a[0]; }
    else { px[0] = a[0]; px[1] = a[1]; px[2] = a[2]; }
}

// the sums over the S x S sub-samples of up to 4 consecutive crop pixels (row i, columns j0 ... j0 + npx - 1): acc[k] is (g, -, -),
// (byte 0, 1, 2) or (Y, U, V); ok[k] turns false when one of pixel k's sub-samples is refused by the 2^20 rule
template <int KIND, bool WIDE>
ALIGN_HD void align_area_sums(const AlignRow& r, int i, int j0, int npx, int S, uint32_t acc[4][3], bool ok[4])
{
    const float* o = align_area_offsets.o + S * (S - 1) / 2;
    const int cw = (r.w + 1) >> 1, ch = (r.h + 1) >> 1;
    for (int v = 0; v < S; ++v) {
        const float fi = (float)i + o[v];
        const float ax = r.m[1] * fi, ay = r.m[4] * fi;
        for (int u = 0; u < S; ++u) {
            const float ou = o[u];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float fj = (float)(j0 + k) + ou;
                const float sx = (r.m[0] * fj + ax) + r.m[2];
                const float sy = (r.m[3] * fj + ay) + r.m[5];
                AlignPos q;
                q.x0 = q.fx = q.y0 = q.fy = 0;
                const bool in = k < npx && align_quantise(sx, sy, q);
                ok[k] = ok[k] && in;
                if (!in) continue;
                if constexpr (KIND == ALIGN_AREA_GRAY) {
                    align_area_add<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q, acc[k]);
                } else if constexpr (KIND == ALIGN_AREA_BGR) {
                    align_area_add<3, 3, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q, acc[k]);
                } else if constexpr (KIND == ALIGN_AREA_BGRA) {
                    align_area_add<4, 3, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q, acc[k]);
                } else if constexpr (KIND == ALIGN_AREA_PLANAR) {
                    align_area_add<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q, acc[k]);
                    align_area_add<1, 1, WIDE, 0u>(r.p0 + r.pd, r.w, r.h, r.stride, q, acc[k] + 1);
                    align_area_add<1, 1, WIDE, 0u>(r.p0 + r.pd + r.pd, r.w, r.h, r.stride, q, acc[k] + 2);
                } else if constexpr (KIND == ALIGN_AREA_P010_LUMA) {
                    align_area_add16<1, WIDE>(r.p0, r.w, r.h, r.stride, q, 0u, acc[k]);
                } else if constexpr (KIND == ALIGN_AREA_P010) {
                    align_area_add16<1, WIDE>(r.p0, r.w, r.h, r.stride, q, 0u, acc[k]);
                    AlignPos qc;
                    if (align_quantise(sx * 0.5f, sy * 0.5f, qc))
                        align_area_add16<2, WIDE>(r.p1, cw, ch, r.cstride, qc, 512u, acc[k] + 1);
                    else { acc[k][1] += 512u * 1024u; acc[k][2] += 512u * 1024u; }
                } else {
                    align_area_add<1, 1, WIDE, 0u>(r.p0, r.w, r.h, r.stride, q, acc[k]);
                    AlignPos qc;
                    if (align_quantise(sx * 0.5f, sy * 0.5f, qc))         // (exact halves: never refused behind an accepted luma position)
                        align_area_add<2, 2, WIDE, 128u>(r.p1, cw, ch, r.cstride, qc, acc[k] + 1);
                    else { acc[k][1] += 128u * 1024u; acc[k][2] += 128u * 1024u; }
                }
            }
        }
    }
}

// align_segment of sdm_align_tensor_device.h for a row with S > 1: every pixel the average of its S x S sub-samples, (B, G, R); NV12 is
// converted once, from the averaged (Y, U, V); a pixel with a refused sub-sample is (0, 0, 0)
template <bool WIDE>
ALIGN_HD void align_area_segment(const AlignRow& r, int i, int j0, int npx, int S, uint32_t px[4][3])
{
    uint32_t acc[4][3];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { acc[k][0] = acc[k][1] = acc[k][2] = 0u; ok[k] = k < npx; }
    const int kind = align_area_kind(r.format);
    switch (kind) {
    case ALIGN_AREA_GRAY: align_area_sums<ALIGN_AREA_GRAY, WIDE>(r, i, j0, npx, S, acc, ok); break;
    case ALIGN_AREA_BGR: align_area_sums<ALIGN_AREA_BGR, WIDE>(r, i, j0, npx, S, acc, ok); break;
    case ALIGN_AREA_BGRA: align_area_sums<ALIGN_AREA_BGRA, WIDE>(r, i, j0, npx, S, acc, ok); break;
    case ALIGN_AREA_PLANAR: align_area_sums<ALIGN_AREA_PLANAR, WIDE>(r, i, j0, npx, S, acc, ok); break;
    case ALIGN_AREA_P010: align_area_sums<ALIGN_AREA_P010, WIDE>(r, i, j0, npx, S, acc, ok); break;
    case ALIGN_AREA_P010_LUMA: align_area_sums<ALIGN_AREA_P010_LUMA, WIDE>(r, i, j0, npx, S, acc, ok); break;
    default: align_area_sums<ALIGN_AREA_NV12, WIDE>(r, i, j0, npx, S, acc, ok); break;
    }
    const uint32_t n = (uint32_t)(S * S), rcp = align_area_reciprocal(n);
    const bool one = kind == ALIGN_AREA_GRAY || kind == ALIGN_AREA_P010_LUMA;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k][0] = px[k][1] = px[k][2] = 0u;
        if (!ok[k]) continue;
        uint32_t a[3] = {align_area_average(acc[k][0], n, rcp), 0u, 0u};
        if (!one) {
#pragma unroll
            for (int c = 1; c < 3; ++c) a[c] = align_area_average(acc[k][c], n, rcp);
        }
        align_area_finish(r.format, a, px[k]);
    }
}
