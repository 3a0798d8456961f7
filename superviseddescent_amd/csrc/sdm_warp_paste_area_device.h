// sdm_warp_paste_area_device.h -- what the filtered piecewise-affine paste (include/sdm.h, "Pasting warped faces back, filtered") adds to
// csrc/sdm_warp_paste_device.h: (Sx, Sy) of a triangle from its W_t (warp_paste_area_counts: warp_area_samples of
// csrc/sdm_warp_area_device.h on the inverse), the pixel of a triangle above (1, 1) -- the average of the Sx x Sy sub-samples' unrounded
// sums through the pixel's own W_t, an opacity tap on label 255 reading 0 (warp_paste_area_taps) --, and the shapes for the ownership
// rule: PasteMeshArea, and PasteMeshAreaOwn for an owner whose records and counts are staged and whose triangle search is already done.
// The footprint is the unfiltered one (warp_paste_footprint's predicate); the offsets and the exact average are
// csrc/sdm_align_area_device.h's, the blend and the ownership rule csrc/sdm_paste_device.h's.  Plain C++ behind ALIGN_HD: the device code
// of csrc/sdm_warp_paste.hip and, compiled for the host, tests/cpp/warp_paste_area_host.cpp.  No float contraction.
#pragma once
#include "sdm_warp_paste_device.h"
#include "sdm_warp_area_device.h"
#include "sdm_align_paste_area_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a triangle's counts, packed: Sx in bits 0 ... 7, Sy in bits 8 ... 15; kept in an array of its own beside the WarpPasteTri records
typedef uint16_t WarpPasteCounts;
#define WPASTE_COUNTS_ONE ((WarpPasteCounts)0x0101u)

// (Sx, Sy) of a triangle of a row with `flags`: 1 for a triangle that covers nothing; else align_area_samples' rule on
// cx2 = W00 W00 + W10 W10 and on cy2 = W01 W01 + W11 W11
ALIGN_HD WarpPasteCounts warp_paste_area_counts(const WarpPasteTri& t, int flags, int mode, int max_samples, float min2)
{
    if (!t.covers) return WPASTE_COUNTS_ONE;
    int Sx, Sy;
    warp_area_samples(t.w, flags, mode, max_samples, min2, Sx, Sy);
    return (WarpPasteCounts)(Sx | Sy << 8);
}

// paste_area_tap_sums with the mesh's label rule: an opacity tap on a crop pixel with label 255 reads 0
ALIGN_HD void warp_paste_area_tap_sums(const PasteCropDev& c, int n, const AlignPos& q, const uint8_t* labels, uint32_t sum[3], uint32_t& asum)
{
    const uint32_t wt[4] = {(uint32_t)((32 - q.fx) * (32 - q.fy)), (uint32_t)(q.fx * (32 - q.fy)), (uint32_t)((32 - q.fx) * q.fy),
                            (uint32_t)(q.fx * q.fy)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = q.x0 + (k & 1), y = q.y0 + (k >> 1);
        const bool in = x >= 0 && x < c.cw && y >= 0 && y < c.ch;
        const int xc = x < 0 ? 0 : (x > c.cw - 1 ? c.cw - 1 : x), yc = y < 0 ? 0 : (y > c.ch - 1 ? c.ch - 1 : y);
        if (in && labels[(long long)yc * c.cw + xc] != 255u)
            asum += wt[k] * (c.alpha ? (uint32_t)c.alpha[(long long)n * c.an + (long long)yc * c.cw + xc] : 255u);
        const long long e = (long long)n * c.sn + (long long)yc * c.sy + (long long)xc * c.sx;
        if (c.channels == 3) {
#pragma unroll
            for (int t = 0; t < 3; ++t) sum[t] += wt[k] * paste_decode(c, e + (long long)t * c.sc, t);
        } else {
            sum[0] += wt[k] * paste_decode(c, e, 0);
        }
    }
}

// frame pixel (X, Y) under row n through the W_t w of its triangle, whose counts (Sx, Sy) are not (1, 1): the Sx x Sy sub-samples'
// unrounded colour and opacity sums -- all through w, those beyond the triangle's edge too --, averaged; then the channel order as at
// (1, 1).  a = 0 when a sub-sample is refused by the 2^20 rule: the row does not touch the pixel.
ALIGN_HD void warp_paste_area_taps(const PasteCropDev& c, int n, const float w[6], int Sx, int Sy, const uint8_t* labels, int X, int Y,
                                   uint32_t bgr[3], uint32_t& a)
{
    const float* ox = align_area_offsets.o + Sx * (Sx - 1) / 2;
    const float* oy = align_area_offsets.o + Sy * (Sy - 1) / 2;
    uint32_t sum[3] = {0u, 0u, 0u}, asum = 0u;
    bool ok = true;
    for (int v = 0; v < Sy; ++v) {
        const float fy = (float)Y + oy[v];
        const float ax = w[1] * fy, ay = w[4] * fy;
        for (int u = 0; u < Sx; ++u) {
            const float fx = (float)X + ox[u];
            const float pu = (w[0] * fx + ax) + w[2];
            const float pv = (w[3] * fx + ay) + w[5];
            AlignPos q;
            if (!align_quantise(pu, pv, q)) { ok = false; continue; }
            warp_paste_area_tap_sums(c, n, q, labels, sum, asum);
        }
    }
    a = 0u;
    bgr[0] = bgr[1] = bgr[2] = 0u;
    if (!ok) return;
    const uint32_t k = (uint32_t)(Sx * Sy), rcp = align_area_reciprocal(k);           // (k >= 2: not both counts are 1)
    a = align_area_average(asum, k, rcp);
    if (c.channels == 3) {
        const bool rgb = c.t.order == SDM_ALIGN_ORDER_RGB;
        const uint32_t t0 = align_area_average(sum[0], k, rcp), t1 = align_area_average(sum[1], k, rcp), t2 = align_area_average(sum[2], k, rcp);
        bgr[0] = rgb ? t2 : t0; bgr[1] = t1; bgr[2] = rgb ? t0 : t2;
    } else {
        bgr[0] = bgr[1] = bgr[2] = align_area_average(sum[0], k, rcp);
    }
}

// warp_paste_footprint that also says which triangle holds the pixel: its number, or -1 when the footprint does not hold the pixel
ALIGN_HD int warp_paste_footprint_triangle(const WarpPasteRow& r, const WarpPasteTri* tris, int T, int cw, int ch, int X, int Y, AlignPos& q)
{
    if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) return -1;
    for (int t = 0; t < T; ++t) {
        const WarpPasteTri& tr = tris[t];
        if (!warp_paste_inside(tr, X, Y)) continue;
        return paste_position(tr.w, cw, ch, X, Y, q) ? t : -1;
    }
    return -1;
}

// a row's colour and opacity on a pixel that triangle `rec` with the counts `cnt` holds at q: the unfiltered taps at (1, 1)
ALIGN_HD void warp_paste_area_sample(const PasteCropDev& c, int n, const WarpPasteTri& rec, WarpPasteCounts cnt, const uint8_t* labels, int X,
                                     int Y, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    if (cnt == WPASTE_COUNTS_ONE) paste_sample_taps<true>(c, n, q, labels, bgr, a);
    else warp_paste_area_taps(c, n, rec.w, cnt & 255, cnt >> 8, labels, X, Y, bgr, a);
}

// The filtered paste's shape for paste_owned and paste_owned_block: PasteMesh and every triangle's counts (N x T).  paste_taps must know
// which triangle holds the pixel, and the ownership rule hands over only q: the shape carries it.  paste_holds leaves the triangle in
// `tri` whenever it answers true; whoever calls the rule for an entry whose own answer it already has (paste_owned's entry k) sets `tri`
// to that entry's triangle first -- the rule's test against earlier entries leaves on the first true, so it never disturbs it.
struct PasteMeshArea {
    PasteMesh mesh;
    const WarpPasteCounts* counts;
    mutable int tri;
};

ALIGN_HD bool paste_holds(const PasteMeshArea& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    const int t = warp_paste_footprint_triangle(p.mesh.rows[n], p.mesh.tris + (long long)n * p.mesh.T, p.mesh.T, c.cw, c.ch, X, Y, q);
    if (t < 0) return false;
    p.tri = t;
    return true;
}

ALIGN_HD void paste_taps(const PasteMeshArea& p, const PasteCropDev& c, int n, int X, int Y, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    const long long at = (long long)n * p.mesh.T + p.tri;
    warp_paste_area_sample(c, n, p.mesh.tris[at], p.counts[at], p.mesh.labels, X, Y, q, bgr, a);
}

// The shape as an owner sees it whose T records and counts are staged (own_tris, own_counts): its row answers from them.  On a per-pixel
// frame the owner's own test is never asked for (winners is not read; area.tri is the owner's triangle); on an NV12 frame it answers
// from the packed winners of its block, as PasteMeshOwn does.  Every other row answers through PasteMeshArea.
struct PasteMeshAreaOwn {
    PasteMeshArea area;
    int own;                    // the owner's row number
    uint32_t winners;
    const WarpPasteTri* own_tris;
    const WarpPasteCounts* own_counts;
};

ALIGN_HD bool paste_holds(const PasteMeshAreaOwn& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    if (n != p.own) return paste_holds(p.area, n, c, X, Y, q);
    const uint32_t t = p.winners >> (8 * ((X & 1) | (Y & 1) << 1)) & 255u;
    if (t == WPASTE_NO_WINNER || !paste_position(p.own_tris[t].w, c.cw, c.ch, X, Y, q)) return false;
    p.area.tri = (int)t;
    return true;
}

ALIGN_HD void paste_taps(const PasteMeshAreaOwn& p, const PasteCropDev& c, int n, int X, int Y, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    if (n != p.own) { paste_taps(p.area, c, n, X, Y, q, bgr, a); return; }
    warp_paste_area_sample(c, n, p.own_tris[p.area.tri], p.own_counts[p.area.tri], p.area.mesh.labels, X, Y, q, bgr, a);
}

// paste_owned for the filtered mesh from its parts, as the host program calls it: entry k's own triangle is looked up here
ALIGN_HD void warp_paste_area_pixel(const PasteFrameDev& f, const WarpPasteRow* rows, const WarpPasteTri* tris, const WarpPasteCounts* counts,
                                    int T, const int* list, int k, const PasteCropDev& c, const uint8_t* labels, int X, int Y)
{
    const PasteMeshArea shape{PasteMesh{rows, tris, T, labels}, counts, -1};
    AlignPos q;
    if (paste_holds(shape, list[k], c, X, Y, q)) paste_owned(f, shape, list, k, c, X, Y, q);
}
