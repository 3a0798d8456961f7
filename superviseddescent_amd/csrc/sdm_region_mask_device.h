// sdm_region_mask_device.h -- the arithmetic of the landmark region masks (include/sdm.h, "Landmark region masks"): a row's inverse map
// and flags, the vertex transform, the convex hull of a polygon's points (insertion sort, monotone chain), an edge record, a pixel's
// signed distance to a polygon and the byte of the map.  Plain C++ behind ALIGN_HD: the device code of csrc/sdm_region_mask.hip and,
// compiled for the host, tests/cpp/region_mask_host.cpp, which runs it under the host sanitizers on vertex lists, workspaces and maps of
// exactly the bytes they own.
//
// Every float operation is float32 and rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off elsewhere),
// except the hull's turn, whose two products are taken in double, where they are exact.
#pragma once
#include "sdm_paste_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define ALIGN_HD_MEMBER __device__ __forceinline__
#else
#define ALIGN_HD_MEMBER inline
#endif

#define REGION_MAX_POLYGONS 8
#define REGION_MAX_SIZE 128
#define REGION_MAX_POINTS 256
#define REGION_MAX_POS 1048576.0f       // 2^20: a vertex beyond gives SDM_REGION_NONFINITE

// a call's region as the kernels read it: start[g] is polygon g's first point among the P
struct RegionDev {
    int n_polygons, n_holes, P;
    unsigned hull_bits;
    float grow, feather;
    int size[REGION_MAX_POLYGONS], start[REGION_MAX_POLYGONS];
};

// one row, as the prepare stage leaves it.  count[g]: the vertices of polygon g (its size, or what the hull kept); box: the box of the
// vertices of the polygons that are no holes, [x0, x1] x [y0, y1]
struct RegionRow {
    int flags;                  // SDM_ALIGN_* | SDM_REGION_NONFINITE; not 0 & (DEGENERATE | NONFINITE): the map is all zeros
    int count[REGION_MAX_POLYGONS];
    float x0, y0, x1, y1;
};

// one edge a -> b of a polygon, as the pixel code reads it
struct RegionEdge {
    float ax, ay, ex, ey, ee, by;
};

// Host code: start[] and P from the sizes
static inline void region_layout(RegionDev& r)
{
    r.P = 0;
    for (int g = 0; g < r.n_polygons; ++g) { r.start[g] = r.P; r.P += r.size[g]; }
}

// the vertex buffer of a row holds 2 P points: polygon g's vertices begin at 2 * start[g] (the chain of a hull of m points may hold more
// than m entries while it is built, never 2 m)
ALIGN_HD int region_vertex_at(const RegionDev& r, int g) { return 2 * r.start[g]; }

// W of the float32 M and the row's flags without the vertices: flags_in is the fit's flags, or -1 (the _at form: none).  True: W is usable
ALIGN_HD bool region_inverse(const float m[6], int flags_in, float w[6], int& flags)
{
    bool finite = true;
    for (int e = 0; e < 6; ++e) finite = finite && isfinite(m[e]);
    flags = flags_in < 0 ? 0 : flags_in;
    const double d = paste_inverse(m, w);
    bool ok = finite && !(flags & SDM_ALIGN_DEGENERATE) && d != 0.0;
    for (int e = 0; e < 6; ++e) ok = ok && isfinite(w[e]);
    if (!ok) flags = finite ? flags | SDM_ALIGN_DEGENERATE : SDM_ALIGN_DEGENERATE;      // (as the fit: no other bit beside a non-finite M)
    return ok;
}

ALIGN_HD void region_transform(const float w[6], float px, float py, float& qx, float& qy)
{
    qx = (w[0] * px + w[1] * py) + w[2];
    qy = (w[3] * px + w[4] * py) + w[5];
}

ALIGN_HD bool region_vertex_ok(float qx, float qy) { return fabsf(qx) <= REGION_MAX_POS && fabsf(qy) <= REGION_MAX_POS; }       // (false for a NaN)

// the turn of (o, a, b): > 0 left, < 0 right, 0 collinear -- exact
ALIGN_HD int region_turn(float ox, float oy, float ax, float ay, float bx, float by)
{
    const float d0 = ax - ox, d1 = by - oy, d2 = ay - oy, d3 = bx - ox;
    const double l = (double)d0 * (double)d1, r = (double)d2 * (double)d3;
    return l > r ? 1 : (l < r ? -1 : 0);
}

// The convex hull of the m points at v (x, y pairs), which are sorted in place; the hull's vertices go to out (room for 2 m points),
// lower chain then upper chain; returns their number, >= 1
ALIGN_HD int region_hull(float* v, int m, float* out)
{
    for (int i = 1; i < m; ++i) {                                                   // insertion sort by (x, then y)
        const float x = v[2 * i], y = v[2 * i + 1];
        int j = i;
        while (j > 0 && (v[2 * j - 2] > x || (v[2 * j - 2] == x && v[2 * j - 1] > y))) {
            v[2 * j] = v[2 * j - 2]; v[2 * j + 1] = v[2 * j - 1];
            --j;
        }
        v[2 * j] = x; v[2 * j + 1] = y;
    }
    int n = 1;                                                                       // exact duplicates dropped
    for (int i = 1; i < m; ++i)
        if (v[2 * i] != v[2 * n - 2] || v[2 * i + 1] != v[2 * n - 1]) { v[2 * n] = v[2 * i]; v[2 * n + 1] = v[2 * i + 1]; ++n; }
    if (n == 1) { out[0] = v[0]; out[1] = v[1]; return 1; }
    int k = 0;
    for (int i = 0; i < n; ++i) {
        while (k >= 2 && region_turn(out[2 * k - 4], out[2 * k - 3], out[2 * k - 2], out[2 * k - 1], v[2 * i], v[2 * i + 1]) <= 0) --k;
        out[2 * k] = v[2 * i]; out[2 * k + 1] = v[2 * i + 1]; ++k;
    }
    for (int i = n - 2, t = k + 1; i >= 0; --i) {
        while (k >= t && region_turn(out[2 * k - 4], out[2 * k - 3], out[2 * k - 2], out[2 * k - 1], v[2 * i], v[2 * i + 1]) <= 0) --k;
        out[2 * k] = v[2 * i]; out[2 * k + 1] = v[2 * i + 1]; ++k;
    }
    return k - 1;                                                                    // (the last entry is the first again)
}

// a row's P frame points: as (x, y) pairs -- the _at form, the host program -- or gathered from the landmark state
struct RegionPairs {
    const float* p;
    ALIGN_HD_MEMBER void get(int k, float& x, float& y) const { x = p[2 * k]; y = p[2 * k + 1]; }
};
struct RegionState {
    const float* x;             // the row: L x then L y
    const int* idx;             // P landmark indices
    int L;
    ALIGN_HD_MEMBER void get(int k, float& px, float& py) const { px = x[idx[k]]; py = x[L + idx[k]]; }
};

// Polygon g of one row.  pts: the row's P frame points; sorted: the row's P points of room (a hull's sort); verts: the row's vertex
// buffer, 2 P points.  Returns the polygon's vertex count
template <class Points>
ALIGN_HD int region_prepare_polygon(const RegionDev& r, int g, const float w[6], const Points& pts, float* sorted, float* verts)
{
    const int m = r.size[g], s = r.start[g];
    const bool hull = (r.hull_bits >> g & 1u) != 0u;
    float* q = hull ? sorted + 2 * s : verts + 2 * region_vertex_at(r, g);
    for (int k = 0; k < m; ++k) {
        float px, py;
        pts.get(s + k, px, py);
        region_transform(w, px, py, q[2 * k], q[2 * k + 1]);
    }
    return hull ? region_hull(q, m, verts + 2 * region_vertex_at(r, g)) : m;
}

// What every lane of a row's prepare stage works out alike from all P points: NONFINITE, and the box of the polygons that are no holes
template <class Points>
ALIGN_HD void region_prepare_row(const RegionDev& r, const float w[6], const Points& pts, bool usable, int flags, RegionRow& row)
{
    row.x0 = row.y0 = row.x1 = row.y1 = 0.0f;
    row.flags = flags;
    if (!usable) return;
    const int solid = r.n_holes > 0 ? r.start[r.n_polygons - r.n_holes] : r.P;                       // the points ahead of the first hole
    bool ok = true;
    for (int k = 0; k < r.P; ++k) {
        float px, py, qx, qy;
        pts.get(k, px, py);
        region_transform(w, px, py, qx, qy);
        ok = ok && region_vertex_ok(qx, qy);
        if (k < solid) {
            row.x0 = k == 0 ? qx : fminf(row.x0, qx); row.x1 = k == 0 ? qx : fmaxf(row.x1, qx);
            row.y0 = k == 0 ? qy : fminf(row.y0, qy); row.y1 = k == 0 ? qy : fmaxf(row.y1, qy);
        }
    }
    if (!ok) row.flags = flags | SDM_REGION_NONFINITE;
}

ALIGN_HD bool region_row_empty(int flags) { return (flags & (SDM_ALIGN_DEGENERATE | SDM_REGION_NONFINITE)) != 0; }

ALIGN_HD RegionEdge region_edge(float ax, float ay, float bx, float by)
{
    RegionEdge e;
    e.ax = ax; e.ay = ay; e.by = by;
    e.ex = bx - ax; e.ey = by - ay;
    e.ee = (e.ex * e.ex) + (e.ey * e.ey);
    return e;
}

// one edge on one pixel: the squared distance and the winding number carried along
ALIGN_HD void region_edge_pixel(const RegionEdge& e, float px, float py, float& d2, int& wn)
{
    const float wx = px - e.ax, wy = py - e.ay;
    const float t = e.ee > 0.0f ? fminf(fmaxf(((wx * e.ex) + (wy * e.ey)) / e.ee, 0.0f), 1.0f) : 0.0f;
    const float dx = wx - (t * e.ex), dy = wy - (t * e.ey);
    d2 = fminf(d2, (dx * dx) + (dy * dy));
    const float cr = (e.ex * wy) - (e.ey * wx);
    if (e.ay <= py) { if (e.by > py && cr > 0.0f) ++wn; }
    else if (e.by <= py && cr < 0.0f) --wn;
}

// a polygon's signed distance folded into s: a hole takes the larger of s and -sd
ALIGN_HD float region_fold(float s, float d2, int wn, bool hole)
{
    const float d = sqrtf(d2), sd = wn != 0 ? -d : d;
    return hole ? fmaxf(s, -sd) : fminf(s, sd);
}

ALIGN_HD uint32_t region_byte(float s, float grow, float feather)
{
    const float wr = fmaxf(feather, 1.0f);
    const float a = 0.5f + ((grow - s) / wr);
    return (uint32_t)rintf(fminf(fmaxf(a, 0.0f), 1.0f) * 255.0f);
}

// A pixel at least this far outside the row's box has byte 0 whatever the edges say: s is at least the distance to the box (a hole only
// raises it), the ramp ends grow + wr / 2 outside the contour, and two pixels more cover every rounding at |q| <= 2^20
ALIGN_HD float region_reach(float grow, float feather) { return (grow + 0.5f * fmaxf(feather, 1.0f)) + 2.0f; }

ALIGN_HD bool region_pixel_far(const RegionRow& row, float reach, float px, float py)
{
    return px < row.x0 - reach || px > row.x1 + reach || py < row.y0 - reach || py > row.y1 + reach;
}

// The byte of crop pixel (c, r) of one row from its vertex buffer: the formula, edge by edge -- what the host program runs, and what the
// kernel's staged loop must give
ALIGN_HD uint32_t region_pixel(const RegionDev& r, const RegionRow& row, const float* verts, int c, int rr)
{
    if (region_row_empty(row.flags)) return 0u;
    const float px = (float)c, py = (float)rr;
    float s = INFINITY;
    for (int g = 0; g < r.n_polygons; ++g) {
        const float* v = verts + 2 * region_vertex_at(r, g);
        const int m = row.count[g];
        float d2 = INFINITY;
        int wn = 0;
        for (int k = 0; k < m; ++k) {
            const int k1 = k + 1 == m ? 0 : k + 1;
            region_edge_pixel(region_edge(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1]), px, py, d2, wn);
        }
        s = region_fold(s, d2, wn, g >= r.n_polygons - r.n_holes);
    }
    return region_byte(s, r.grow, r.feather);
}
