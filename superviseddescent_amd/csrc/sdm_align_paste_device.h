// sdm_align_paste_device.h -- what the paste-back of crop tensors into frames (include/sdm.h, "Pasting crops back") has of its own: a
// row's inverse map, flags and box (paste_prepare_row), the footprint test (paste_footprint), its shape for the ownership rule
// (PasteRigid) and paste_pixel -- one frame pixel as an entry of its frame's row list sees it.  Everything both pastes share, the
// ownership rule among it, is csrc/sdm_paste_device.h.  Plain C++ behind ALIGN_HD: the device code of csrc/sdm_align_paste.hip and,
// compiled for the host, tests/cpp/align_paste_host.cpp.  No float contraction (the pragma below under clang, -ffp-contract=off elsewhere).
#pragma once
#include "sdm_paste_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// one row, as the prepare stage leaves it
struct PasteRow {
    float w[6];                 // frame -> crop: W00 W01 W02 W10 W11 W12
    int flags;                  // SDM_ALIGN_*
    int frame;
    int x0, y0, x1, y1;         // the footprint's box in the frame, [x0, x1) x [y0, y1); empty for a row that pastes nothing
};

// M00 M01 M02 M10 M11 M12 (float32, crop -> frame) of a row in a frame of fw x fh pixels: W, the flags and the box.  flags_in: the
// fit's flags, or -1 -- then PARTIAL is the fit's rule evaluated here, on the corner pixel centres of the crop.
ALIGN_HD void paste_prepare_row(const float m[6], int flags_in, int frame, int fw, int fh, int cw, int ch, PasteRow& r)
{
    r.frame = frame;
    r.x0 = r.y0 = r.x1 = r.y1 = 0;
    bool finite = true;
    for (int e = 0; e < 6; ++e) finite = finite && isfinite(m[e]);
    int flags = flags_in < 0 ? 0 : flags_in;
    if (flags_in < 0 && finite) {
        const float cj[2] = {0.0f, (float)(cw - 1)}, ci[2] = {0.0f, (float)(ch - 1)};
        for (int u = 0; u < 2; ++u)
            for (int v = 0; v < 2; ++v) {
                const float sx = (m[0] * cj[u] + m[1] * ci[v]) + m[2];
                const float sy = (m[3] * cj[u] + m[4] * ci[v]) + m[5];
                if (!(sx >= 0.0f && sx <= (float)(fw - 1) && sy >= 0.0f && sy <= (float)(fh - 1))) flags = SDM_ALIGN_PARTIAL;
            }
    }
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const double d = paste_inverse(m, r.w);
    bool ok = finite && !(flags & SDM_ALIGN_DEGENERATE) && d != 0.0;
    for (int e = 0; e < 6; ++e) ok = ok && isfinite(r.w[e]);
    if (!ok) {
        r.flags = finite ? flags | SDM_ALIGN_DEGENERATE : SDM_ALIGN_DEGENERATE;       // (as the fit: no other bit beside a non-finite M)
        return;
    }
    r.flags = flags;
    // the box: the crop corners (-1, -1) ... (cw, ch) through M, widened by what the float32 W and positions can move a footprint
    // pixel against the exact inverse.  A position has three rounded products and sums of magnitude <= |W..| fw + |W..| fh + |W.2|,
    // each W entry is rounded once: 2^-21 of that magnitude bounds the error in crop pixels, 1/32 more covers the quantisation; a
    // crop pixel is |M00| + |M01| (|M10| + |M11|) frame pixels wide (high); one frame pixel more for the floor and the ceiling.
    const double eu = (fabs((double)r.w[0]) * fw + fabs((double)r.w[1]) * fh + fabs((double)r.w[2]) + 1.0) * (1.0 / 2097152.0) + 0.03125;
    const double ev = (fabs((double)r.w[3]) * fw + fabs((double)r.w[4]) * fh + fabs((double)r.w[5]) + 1.0) * (1.0 / 2097152.0) + 0.03125;
    const double e = eu > ev ? eu : ev;
    const double mx = (fabs(m00) + fabs(m01)) * e + 1.0, my = (fabs(m10) + fabs(m11)) * e + 1.0;
    double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double u = (k & 1) ? (double)cw : -1.0, v = (k & 2) ? (double)ch : -1.0;
        const double x = (m00 * u + m01 * v) + m02, y = (m10 * u + m11 * v) + m12;
        if (k == 0 || x < xlo) xlo = x;
        if (k == 0 || x > xhi) xhi = x;
        if (k == 0 || y < ylo) ylo = y;
        if (k == 0 || y > yhi) yhi = y;
    }
    xlo = floor(xlo - mx); xhi = ceil(xhi + mx) + 1.0; ylo = floor(ylo - my); yhi = ceil(yhi + my) + 1.0;
    // clipped to the frame while still double: nothing beyond int reaches the conversion
    r.x0 = xlo > 0.0 ? (xlo < (double)fw ? (int)xlo : fw) : 0;
    r.y0 = ylo > 0.0 ? (ylo < (double)fh ? (int)ylo : fh) : 0;
    r.x1 = xhi < (double)fw ? (xhi > 0.0 ? (int)xhi : 0) : fw;
    r.y1 = yhi < (double)fh ? (yhi > 0.0 ? (int)yhi : 0) : fh;
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r.x0 = r.y0 = r.x1 = r.y1 = 0;
}

// frame pixel (X, Y) in the footprint of r: inside its box, and its position accepted
ALIGN_HD bool paste_footprint(const PasteRow& r, int cw, int ch, int X, int Y, AlignPos& q)
{
    if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) return false;
    return paste_position(r.w, cw, ch, X, Y, q);
}

// the rigid paste's shape for paste_owned: all rows' records
struct PasteRigid {
    const PasteRow* rows;
};

ALIGN_HD bool paste_holds(const PasteRigid& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    return paste_footprint(p.rows[n], c.cw, c.ch, X, Y, q);
}

ALIGN_HD void paste_taps(const PasteRigid&, const PasteCropDev& c, int n, int, int, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    paste_sample_taps<false>(c, n, q, nullptr, bgr, a);
}

// Frame pixel (X, Y) as seen by entry k of its frame's row list: in that row's footprint, the ownership rule (paste_owned); else nothing
template <bool PLANAR = true>
ALIGN_HD void paste_pixel(const PasteFrameDev& f, const PasteRow* rows, const int* list, int k, const PasteCropDev& c, int X, int Y)
{
    AlignPos q;
    if (paste_footprint(rows[list[k]], c.cw, c.ch, X, Y, q)) paste_owned<PLANAR>(f, PasteRigid{rows}, list, k, c, X, Y, q);
}
