// sdm_warp_paste_device.h -- the arithmetic of the piecewise-affine paste (include/sdm.h, "Pasting warped faces back"): a row's flags
// and box from its mesh landmarks, a triangle's record -- the inverse W_t of its float32 A_t, its corners in edge-function order, its
// box --, the triangle of a frame pixel, and the paste's shapes for the ownership rule (PasteMesh; PasteMeshOwn for the owner of an
// NV12 block, whose own triangle search is done before the block rule runs).  The fit is warp_fit_triangle
// (sdm_warp_device.h); the inverse, the position, the taps, the decode, the blend, the pixel's load / apply / store and the ownership
// rule (paste_owned) are sdm_paste_device.h's; the quantisation is sdm_align_tensor_device.h's.  Plain C++ behind ALIGN_HD, so
// the same text is the device code of csrc/sdm_warp_paste.hip and -- compiled for the host, tests/cpp/warp_paste_host.cpp -- a program
// that runs under the host sanitizers.
//
// Every floating-point operation is rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off elsewhere).
#pragma once
#include "sdm_paste_device.h"
#include "sdm_warp_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// one row, as the prepare stage leaves it
struct WarpPasteRow {
    int flags;                  // SDM_WARP_*
    int frame;
    int x0, y0, x1, y1;         // the landmarks' box in the frame, [x0, x1) x [y0, y1); empty for a row that pastes nothing
};

// one triangle of one row
struct WarpPasteTri {
    float w[6];                 // frame -> crop: the inverse of the float32 A_t
    float a[2], b[2], c[2];     // the corners as the edge functions read them: b and c exchanged where det E < 0
    int x0, y0, x1, y1;         // the contract's box of the triangle, cut to the row's; empty when it covers nothing
    int covers;                 // 0: det E == 0, d == 0 or an entry of W_t not finite
};

// what the lanes of a wave (the host: one loop) gather over the mesh's landmarks
struct WarpPasteScan {
    bool bad, outside;
    float xlo, xhi, ylo, yhi;
};

ALIGN_HD void warp_paste_scan_init(WarpPasteScan& s)
{
    s.bad = s.outside = false;
    s.xlo = s.ylo = __builtin_inff();
    s.xhi = s.yhi = -__builtin_inff();
}

// landmark (px, py) of a row whose frame has fw x fh pixels: the warp's DEGENERATE and PARTIAL rules, and the extremes
ALIGN_HD void warp_paste_scan_point(float px, float py, int fw, int fh, WarpPasteScan& s)
{
    s.bad = s.bad || !(isfinite(px) && isfinite(py));
    s.outside = s.outside || !(px >= 0.0f && px <= (float)(fw - 1) && py >= 0.0f && py <= (float)(fh - 1));
    s.xlo = fminf(s.xlo, px); s.xhi = fmaxf(s.xhi, px);
    s.ylo = fminf(s.ylo, py); s.yhi = fmaxf(s.yhi, py);
}

// [floor(lo) - margin, ceil(hi) + 1 + margin) clipped to [0, n) while still double: nothing beyond int reaches the conversion
ALIGN_HD void warp_paste_span(float lo, float hi, double margin, int n, int& i0, int& i1)
{
    const double a = floor((double)lo) - margin, b = (ceil((double)hi) + 1.0) + margin;
    i0 = a > 0.0 ? (a < (double)n ? (int)a : n) : 0;
    i1 = b < (double)n ? (b > 0.0 ? (int)b : 0) : n;
}

// the row's record from the gathered scan (all K landmarks); folded: some triangle's FOLDED rule held
ALIGN_HD void warp_paste_row(const WarpPasteScan& s, bool folded, int frame, int fw, int fh, WarpPasteRow& r)
{
    r.frame = frame;
    r.x0 = r.y0 = r.x1 = r.y1 = 0;
    if (s.bad) { r.flags = SDM_WARP_DEGENERATE; return; }
    r.flags = (s.outside ? SDM_WARP_PARTIAL : 0) | (folded ? SDM_WARP_FOLDED : 0);
    warp_paste_span(s.xlo, s.xhi, 0.0, fw, r.x0, r.x1);
    warp_paste_span(s.ylo, s.yhi, 0.0, fh, r.y0, r.y1);
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r.x0 = r.y0 = r.x1 = r.y1 = 0;
}

// det E of a triangle's landmarks: the FOLDED rule's expression (sdm_warp_device.h)
ALIGN_HD double warp_paste_det(const float pa[2], const float pb[2], const float pc[2])
{
    const double e00 = (double)pb[0] - (double)pa[0], e01 = (double)pc[0] - (double)pa[0];
    const double e10 = (double)pb[1] - (double)pa[1], e11 = (double)pc[1] - (double)pa[1];
    return e00 * e11 - e01 * e10;
}

// a triangle's record from its float32 A_t (m) and its landmarks, inside the box of its row (x0 ... y1; empty: the row pastes nothing).
// The triangle's box is the contract's: [floor(min x) - 1, ceil(max x) + 2) of its three corners and the same in y, formed in double
// and cut to the row's box before any conversion to int.  It is part of the rule, not a shortcut: the rounded edge functions of a
// needle triangle with a far corner can be >= 0 many pixels beyond its corners, and every path must then give the same answer.
ALIGN_HD void warp_paste_triangle(const float m[6], const float pa[2], const float pb[2], const float pc[2], int x0, int y0, int x1, int y1,
                                  WarpPasteTri& t)
{
    const double det = warp_paste_det(pa, pb, pc);
    const double d = paste_inverse(m, t.w);
    bool ok = x1 > x0 && y1 > y0 && !(det == 0.0) && !(d == 0.0);
    for (int e = 0; e < 6; ++e) ok = ok && isfinite(t.w[e]);
    const float* qb = det < 0.0 ? pc : pb;
    const float* qc = det < 0.0 ? pb : pc;
    t.a[0] = pa[0]; t.a[1] = pa[1]; t.b[0] = qb[0]; t.b[1] = qb[1]; t.c[0] = qc[0]; t.c[1] = qc[1];
    t.covers = ok ? 1 : 0;
    t.x0 = t.y0 = t.x1 = t.y1 = 0;
    if (!ok) return;
    int bx0, bx1, by0, by1;
    warp_paste_span(fminf(fminf(pa[0], pb[0]), pc[0]), fmaxf(fmaxf(pa[0], pb[0]), pc[0]), 1.0, x1, bx0, bx1);
    warp_paste_span(fminf(fminf(pa[1], pb[1]), pc[1]), fmaxf(fmaxf(pa[1], pb[1]), pc[1]), 1.0, y1, by0, by1);
    bx0 = bx0 < x0 ? x0 : bx0; by0 = by0 < y0 ? y0 : by0;
    if (bx1 <= bx0 || by1 <= by0) return;
    t.x0 = bx0; t.y0 = by0; t.x1 = bx1; t.y1 = by1;
}

// does the triangle's box meet [rx0, rx1) x [ry0, ry1): with one pixel, the contract's box test; with a wave's strip, its cull
ALIGN_HD bool warp_paste_hits(const WarpPasteTri& t, int rx0, int ry0, int rx1, int ry1)
{
    return t.x0 < rx1 && rx0 < t.x1 && t.y0 < ry1 && ry0 < t.y1;
}

// the pixel lies in the triangle's box, and the label map's three edge functions on the row's landmarks are >= 0 at the pixel centre
// (a comparison with a NaN is false)
ALIGN_HD bool warp_paste_inside(const WarpPasteTri& t, int X, int Y)
{
    if (!warp_paste_hits(t, X, Y, X + 1, Y + 1)) return false;
    const double x = (double)X, y = (double)Y;
    const double ax = t.a[0], ay = t.a[1], bx = t.b[0], by = t.b[1], cx = t.c[0], cy = t.c[1];
    const double e0 = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
    if (!(e0 >= 0.0)) return false;
    const double e1 = (cx - bx) * (y - by) - (cy - by) * (x - bx);
    if (!(e1 >= 0.0)) return false;
    const double e2 = (ax - cx) * (y - cy) - (ay - cy) * (x - cx);
    return e2 >= 0.0;
}

// frame pixel (X, Y) in the footprint of row r with the T records tris: inside the row's box, the lowest-numbered covering triangle that
// holds it, and that triangle's position accepted
ALIGN_HD bool warp_paste_footprint(const WarpPasteRow& r, const WarpPasteTri* tris, int T, int cw, int ch, int X, int Y, AlignPos& q)
{
    if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) return false;
    for (int t = 0; t < T; ++t) {
        const WarpPasteTri& tr = tris[t];
        if (!warp_paste_inside(tr, X, Y)) continue;
        return paste_position(tr.w, cw, ch, X, Y, q);
    }
    return false;
}

// the piecewise-affine paste's shape for paste_owned: all rows' records, their triangle records (T per row), the mesh's label map
struct PasteMesh {
    const WarpPasteRow* rows;
    const WarpPasteTri* tris;
    int T;
    const uint8_t* labels;
};

ALIGN_HD bool paste_holds(const PasteMesh& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    return warp_paste_footprint(p.rows[n], p.tris + (long long)n * p.T, p.T, c.cw, c.ch, X, Y, q);
}

ALIGN_HD void paste_taps(const PasteMesh& p, const PasteCropDev& c, int n, int, int, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    paste_sample_taps<true>(c, n, q, p.labels, bgr, a);
}

// The mesh as the owner of an NV12 block sees it (paste_owned_block of sdm_paste_device.h; include/sdm.h, "Pasting warped faces back
// into NV12 frames"): the owner's own triangle search has been done before the block rule runs -- on the device by a walk over the
// row's records staged in LDS, on the host by a plain loop -- and its four answers come packed, pixel i of the block ((X & 1) | (Y & 1)
// << 1) at bits 8 i, 255: no triangle, or the pixel lies outside the row's box.  Every other row answers through warp_paste_footprint.
// own_tris: the owner's T records (its staged copy).  A winner is the lowest-numbered triangle that warp_paste_inside accepts, so that
// this shape and PasteMesh decide every pixel alike: that one triangle's position, and no second triangle tried.
struct PasteMeshOwn {
    PasteMesh mesh;
    int own;                    // the owner's row number
    uint32_t winners;
    const WarpPasteTri* own_tris;
};

#define WPASTE_NO_WINNER 255u

ALIGN_HD bool paste_holds(const PasteMeshOwn& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    if (n != p.own) return paste_holds(p.mesh, n, c, X, Y, q);
    const uint32_t t = p.winners >> (8 * ((X & 1) | (Y & 1) << 1)) & 255u;
    return t != WPASTE_NO_WINNER && paste_position(p.own_tris[t].w, c.cw, c.ch, X, Y, q);
}

ALIGN_HD void paste_taps(const PasteMeshOwn& p, const PasteCropDev& c, int n, int X, int Y, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    paste_taps(p.mesh, c, n, X, Y, q, bgr, a);
}

// the owner's search for the pixels of block (BX, BY) that lie in its box r, triangle after triangle: what the device's LDS walk leaves
ALIGN_HD uint32_t warp_paste_block_winners(const WarpPasteRow& r, const WarpPasteTri* own_tris, int T, int BX, int BY)
{
    uint32_t winners = 0xffffffffu;
    for (int i = 0; i < 4; ++i) {
        const int X = 2 * BX + (i & 1), Y = 2 * BY + (i >> 1);
        if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) continue;
        for (int t = 0; t < T; ++t)
            if (warp_paste_inside(own_tris[t], X, Y)) { winners = (winners & ~(255u << (8 * i))) | (uint32_t)t << (8 * i); break; }
    }
    return winners;
}

// paste_owned for the mesh from its parts, as the host program calls it
ALIGN_HD void warp_paste_owned(const PasteFrameDev& f, const WarpPasteRow* rows, const WarpPasteTri* tris, int T, const int* list, int k,
                               const PasteCropDev& c, const uint8_t* labels, int X, int Y, AlignPos q)
{
    paste_owned(f, PasteMesh{rows, tris, T, labels}, list, k, c, X, Y, q);
}
