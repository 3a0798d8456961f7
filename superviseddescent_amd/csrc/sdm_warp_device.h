// sdm_warp_device.h -- the per-triangle and per-pixel arithmetic of sdm_warp_crops_tensor (include/sdm.h, "Warped faces"): a triangle's
// crop -> source matrix from its three landmarks, and the sibling of align_segment that takes its four positions instead of forming them
// from one matrix.  Everything behind a position is sdm_align_tensor_device.h, unchanged.  Plain C++ behind ALIGN_HD, so the same text is
// the device code of csrc/sdm_warp.hip and -- compiled for the host, tests/cpp/warp_host.cpp -- a program that runs under the host sanitizers.
//
// Every floating-point operation is rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off elsewhere).
#pragma once
#include "sdm_align_tensor_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a triangle of the mesh as the fit reads it: G = [[v.y / D, -v.x / D], [-u.y / D, u.x / D]], the template point q_a, D, and the three
// landmarks' columns in x
struct WarpTri {
    double g[4];                // G00 G01 G10 G11
    double qa[2];
    double D;
    int ia, ib, ic, pad;
};

// A_t of one triangle from its landmarks (pa, pb, pc: x then y): six floats M00 M01 M02 M10 M11 M12; returns whether det(E) is 0 or has
// the sign opposite to D's (SDM_WARP_FOLDED)
ALIGN_HD bool warp_fit_triangle(const WarpTri& t, const float pa[2], const float pb[2], const float pc[2], float m[6])
{
    const double e00 = (double)pb[0] - (double)pa[0], e01 = (double)pc[0] - (double)pa[0];
    const double e10 = (double)pb[1] - (double)pa[1], e11 = (double)pc[1] - (double)pa[1];
    const double l00 = e00 * t.g[0] + e01 * t.g[2], l01 = e00 * t.g[1] + e01 * t.g[3];
    const double l10 = e10 * t.g[0] + e11 * t.g[2], l11 = e10 * t.g[1] + e11 * t.g[3];
    const double t0 = (double)pa[0] - (l00 * t.qa[0] + l01 * t.qa[1]);
    const double t1 = (double)pa[1] - (l10 * t.qa[0] + l11 * t.qa[1]);
    m[0] = (float)l00; m[1] = (float)l01; m[2] = (float)t0;
    m[3] = (float)l10; m[4] = (float)l11; m[5] = (float)t1;
    const double det = e00 * e11 - e01 * e10;
    return !((det > 0.0 && t.D > 0.0) || (det < 0.0 && t.D < 0.0));
}

// the position of crop pixel (column j, row i) through a triangle's matrix: sdm_align_crops' expression
ALIGN_HD void warp_position(const float m[6], int j, int i, float& sx, float& sy)
{
    const float fj = (float)j, fi = (float)i;
    sx = (m[0] * fj + m[1] * fi) + m[2];
    sy = (m[3] * fj + m[4] * fi) + m[5];
}

// align_segment with the positions given: the warped pixel of up to 4 crop pixels at (sx[k], sy[k]) as (B, G, R); a gray source gives
// (g, g, g).  A pixel with on[k] false (beyond the crop row, or no triangle) is (0, 0, 0) and reads no source byte.  r.m is not used.
template <bool WIDE>
ALIGN_HD void warp_segment(const AlignRow& r, const float sx[4], const float sy[4], const bool on[4], uint32_t px[4][3])
{
    AlignPos q[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[k].x0 = q[k].fx = q[k].y0 = q[k].fy = 0;
        ok[k] = on[k] && align_quantise(sx[k], sy[k], q[k]);
        px[k][0] = px[k][1] = px[k][2] = 0u;
    }
    switch (r.format) {
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
    default: {   // SDM_FRAME_NV12
        const int cw = (r.w + 1) >> 1, ch = (r.h + 1) >> 1;
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
    }
    if (r.format == SDM_FRAME_RGB || r.format == SDM_FRAME_RGBA) {          // byte 0 is R: (B, G, R) by byte position
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint32_t t = px[k][0]; px[k][0] = px[k][2]; px[k][2] = t; }
    }
}
