// sdm_warp_area_device.h -- the per-triangle and per-pixel arithmetic of sdm_warp_crops_tensor_filtered (include/sdm.h, "Warped faces,
// filtered"): (Sx, Sy) of a triangle from its matrix, and the average of a pixel's Sx x Sy bilinear sub-samples through its own triangle's
// matrix.  Built on sdm_align_area_device.h (the comparison ladder of S, the offset table, the un-rounded tap sums, the exact average) and
// sdm_warp_device.h, plain C++ behind ALIGN_HD like them: the device code of csrc/sdm_warp_area.hip and -- compiled for the host,
// tests/cpp/warp_area_host.cpp -- a program that runs under the host sanitizers.
//
// Float operations are rounded one by one (no contraction); sums and the average are uint32.
#pragma once
#include "sdm_align_area_device.h"
#include "sdm_warp_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// (Sx, Sy) of a triangle: align_area_samples' rule on cx2 = A00 A00 + A10 A10 (the source step per crop column, squared) and on
// cy2 = A01 A01 + A11 A11 (per crop row).  The rule reads entries 0 and 3 of a matrix, so each axis hands it its own column.
ALIGN_HD void warp_area_samples(const float m[6], int flags, int mode, int max_samples, float min2, int& Sx, int& Sy)
{
    const int fl = (flags & SDM_WARP_DEGENERATE) ? SDM_ALIGN_DEGENERATE : 0;
    const float col[6] = {m[0], 0.0f, 0.0f, m[3], 0.0f, 0.0f}, row[6] = {m[1], 0.0f, 0.0f, m[4], 0.0f, 0.0f};
    Sx = align_area_samples(col, fl, mode, max_samples, min2);
    Sy = align_area_samples(row, fl, mode, max_samples, min2);
}

// a triangle as the pixels read it: its matrix and its counts, 8 words (two 128-bit LDS reads)
struct alignas(16) WarpAreaRec {
    float m[6];
    int Sx, Sy;
};

// the sums over the Sx x Sy sub-samples of crop pixels (row i, columns j0 ... j0 + 3): pixel k belongs to triangle lab[k] of rec (-1: no
// triangle, or beyond the crop row -- nothing is read for it), every pixel goes through its own triangle's matrix.  acc[k] is (g, -, -),
// (byte 0, 1, 2) or (Y, U, V), n[k] = Sx Sy; ok[k] turns false when one of pixel k's sub-samples is refused by the 2^20 rule.  Every
// pixel fetches its record when its turn comes and runs its own pair of loops to its own counts (the form with one loop to
// the lane's largest count keeps no more loads in flight, needs 34 more registers and idles a pixel whose triangle asks for less).
template <int KIND, bool WIDE>
ALIGN_HD void warp_area_sums(const AlignRow& r, const WarpAreaRec* rec, const int lab[4], int i, int j0, uint32_t acc[4][3], uint32_t n[4],
                             bool ok[4])
{
    const int cw = (r.w + 1) >> 1, ch = (r.h + 1) >> 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = 1u;
        if (lab[k] < 0) continue;
        const WarpAreaRec t = rec[lab[k]];
        n[k] = (uint32_t)(t.Sx * t.Sy);
        const int ox = t.Sx * (t.Sx - 1) / 2, oy = t.Sy * (t.Sy - 1) / 2;      // where the counts' offsets start in the table
        for (int v = 0; v < t.Sy; ++v) {
            const float fi = (float)i + align_area_offsets.o[oy + v];
            const float ax = t.m[1] * fi, ay = t.m[4] * fi;
            for (int u = 0; u < t.Sx; ++u) {
                const float fj = (float)(j0 + k) + align_area_offsets.o[ox + u];
                const float sx = (t.m[0] * fj + ax) + t.m[2];
                const float sy = (t.m[3] * fj + ay) + t.m[5];
                AlignPos q;
                q.x0 = q.fx = q.y0 = q.fy = 0;
                const bool in = align_quantise(sx, sy, q);
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

// (sum + 512 n) / (1024 n) for n = Sx Sy in [1, 256]: align_area_average, whose reciprocal starts at 2; n = 1 is the shift of the
// unfiltered warp
ALIGN_HD uint32_t warp_area_average(uint32_t sum, uint32_t n, uint32_t rcp)
{
    return n == 1u ? (sum + 512u) >> 10 : align_area_average(sum, n, rcp);
}

// the filtered warp of up to 4 crop pixels (row i, columns j0 ... j0 + 3) as (B, G, R): every pixel the average of its Sx x Sy
// sub-samples; NV12 is converted once, from the averaged (Y, U, V); a pixel with a refused sub-sample, or without a triangle (lab[k] < 0),
// is (0, 0, 0) and the latter reads no source byte.  r.m is not used.
template <bool WIDE>
ALIGN_HD void warp_area_segment(const AlignRow& r, const WarpAreaRec* rec, const int lab[4], int i, int j0, uint32_t px[4][3])
{
    uint32_t acc[4][3], cnt[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { acc[k][0] = acc[k][1] = acc[k][2] = 0u; ok[k] = lab[k] >= 0; }
    const int kind = align_area_kind(r.format);
    switch (kind) {
    case ALIGN_AREA_GRAY: warp_area_sums<ALIGN_AREA_GRAY, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    case ALIGN_AREA_BGR: warp_area_sums<ALIGN_AREA_BGR, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    case ALIGN_AREA_BGRA: warp_area_sums<ALIGN_AREA_BGRA, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    case ALIGN_AREA_PLANAR: warp_area_sums<ALIGN_AREA_PLANAR, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    case ALIGN_AREA_P010: warp_area_sums<ALIGN_AREA_P010, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    case ALIGN_AREA_P010_LUMA: warp_area_sums<ALIGN_AREA_P010_LUMA, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    default: warp_area_sums<ALIGN_AREA_NV12, WIDE>(r, rec, lab, i, j0, acc, cnt, ok); break;
    }
    const bool one = kind == ALIGN_AREA_GRAY || kind == ALIGN_AREA_P010_LUMA;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k][0] = px[k][1] = px[k][2] = 0u;
        if (!ok[k]) continue;
        const uint32_t n = cnt[k], rcp = n > 1u ? align_area_reciprocal(n) : 0u;
        uint32_t a[3] = {warp_area_average(acc[k][0], n, rcp), 0u, 0u};
        if (!one) {
#pragma unroll
            for (int c = 1; c < 3; ++c) a[c] = warp_area_average(acc[k][c], n, rcp);
        }
        align_area_finish(r.format, a, px[k]);
    }
}
