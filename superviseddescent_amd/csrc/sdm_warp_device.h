// sdm_warp_device.h -- the per-triangle and per-pixel arithmetic of sdm_warp_crops_tensor (include/sdm.h, "Warped faces"): a triangle's
// crop -> source matrix from its three landmarks, and a pixel's position through it.  Everything behind a position is
// align_fetch_segment of sdm_align_tensor_device.h, shared with the similarity crops.  Plain C++ behind ALIGN_HD, so the same text is
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
