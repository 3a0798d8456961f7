// sdm_capi_warp.hip -- C-ABI of the piecewise-affine warped faces (include/sdm.h, "Warped faces"): the host side of the mesh -- the
// Delaunay triangulation of a template, the label map and the triangles' constants, all in double with nothing contracted
// (-ffp-contract=off, csrc/Makefile) -- kept in sdm_ctx::warp, and the two calls that fit every row's triangles and warp its image:
// plain bilinear (csrc/sdm_warp.hip) and area-averaged per triangle and axis ("Warped faces, filtered", csrc/sdm_warp_area.hip).  Every argument is checked before anything is launched or changed; the landmark state, the images, the crop
// source and the tracker's slots are only read.
#include "sdm_capi_internal.h"
#include "sdm_warp.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

struct P2 { double x, y; };

// (b - a) x (c - a): positive for a counter-clockwise triple (D of include/sdm.h)
double orient(const P2& a, const P2& b, const P2& c)
{
    const double ux = b.x - a.x, uy = b.y - a.y, vx = c.x - a.x, vy = c.y - a.y;
    return ux * vy - uy * vx;
}

// d strictly inside the circumcircle of the counter-clockwise (a, b, c): the in-circle determinant beyond 1e-12 of its terms' magnitude
bool in_circle(const P2& a, const P2& b, const P2& c, const P2& d)
{
    const double ax = a.x - d.x, ay = a.y - d.y, bx = b.x - d.x, by = b.y - d.y, cx = c.x - d.x, cy = c.y - d.y;
    const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
    const double det = ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx);
    const double mag = std::fabs(ax) * (std::fabs(by) * c2 + b2 * std::fabs(cy)) + std::fabs(ay) * (std::fabs(bx) * c2 + b2 * std::fabs(cx)) +
                       a2 * (std::fabs(bx * cy) + std::fabs(by * cx));
    return det > 1e-12 * mag;
}

// Delaunay triangulation of K distinct points, not all on one line: the points in lexicographic order are added one by one to a
// triangulation of their hull (every hull edge the new point sees strictly from outside gives a triangle), then shared edges are
// flipped until every one is locally Delaunay (Lawson).  Each step is a function of the input alone.
int delaunay(const std::vector<P2>& p, std::vector<int>& tris)
{
    const int K = (int)p.size();
    std::vector<int> order(K);
    for (int k = 0; k < K; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return p[a].x != p[b].x ? p[a].x < p[b].x : p[a].y != p[b].y ? p[a].y < p[b].y : a < b; });
    for (int k = 1; k < K; ++k)
        if (p[order[k]].x == p[order[k - 1]].x && p[order[k]].y == p[order[k - 1]].y) return fail(SDM_ERR_INVALID, "a point is given twice");
    int m = 2;
    while (m < K && orient(p[order[0]], p[order[1]], p[order[m]]) == 0.0) ++m;
    if (m == K) return fail(SDM_ERR_INVALID, "all points lie on one line");
    std::vector<int> tri;                                    // triples, counter-clockwise
    std::vector<int> hull;                                   // counter-clockwise
    const bool left = orient(p[order[0]], p[order[1]], p[order[m]]) > 0.0;
    for (int k = 0; k + 1 < m; ++k) {
        const int a = order[k], b = order[k + 1], c = order[m];
        if (left) { tri.push_back(a); tri.push_back(b); tri.push_back(c); }
        else { tri.push_back(b); tri.push_back(a); tri.push_back(c); }
    }
    if (left) { for (int k = 0; k < m; ++k) hull.push_back(order[k]); hull.push_back(order[m]); }
    else { hull.push_back(order[0]); hull.push_back(order[m]); for (int k = m - 1; k >= 1; --k) hull.push_back(order[k]); }
    for (int k = m + 1; k < K; ++k) {
        const int q = order[k], h = (int)hull.size();
        std::vector<char> sees(h);
        int n_seen = 0;
        for (int e = 0; e < h; ++e) { sees[e] = orient(p[hull[e]], p[hull[(e + 1) % h]], p[q]) < 0.0; n_seen += sees[e]; }
        if (n_seen == 0 || n_seen == h) return fail(SDM_ERR_INVALID, "the points cannot be triangulated");
        int first = 0;                                       // the seen chain's first edge: seen, its predecessor not
        while (!(sees[first] && !sees[(first + h - 1) % h])) ++first;
        int len = 0;
        while (len < h && sees[(first + len) % h]) ++len;
        if (len != n_seen) return fail(SDM_ERR_INVALID, "the points cannot be triangulated");
        for (int e = 0; e < len; ++e) {
            const int u = hull[(first + e) % h], v = hull[(first + e + 1) % h];
            tri.push_back(v); tri.push_back(u); tri.push_back(q);
        }
        std::vector<int> next;                               // hull[first], q, hull[first + len], ... round to hull[first - 1]
        next.push_back(hull[first]); next.push_back(q);
        for (int e = (first + len) % h; e != first; e = (e + 1) % h) next.push_back(hull[e]);
        hull.swap(next);
    }
    // Lawson flips.  owner[u * K + v]: the triangle whose counter-clockwise boundary holds the edge u -> v, or -1
    const int T = (int)tri.size() / 3;
    std::vector<int> owner((size_t)K * K, -1);
    auto claim = [&](int t) { for (int e = 0; e < 3; ++e) owner[(size_t)tri[3 * t + e] * K + tri[3 * t + (e + 1) % 3]] = t; };
    for (int t = 0; t < T; ++t) claim(t);
    long long flips = 0;
    const long long max_flips = 16ll * K * K + 64;
    for (bool changed = true; changed;) {
        changed = false;
        for (int t = 0; t < T; ++t)
            for (int e = 0; e < 3; ++e) {
                const int u = tri[3 * t + e], v = tri[3 * t + (e + 1) % 3], w = tri[3 * t + (e + 2) % 3];
                const int n = owner[(size_t)v * K + u];
                if (n < 0) continue;
                int z = -1;
                for (int g = 0; g < 3; ++g)
                    if (tri[3 * n + g] != u && tri[3 * n + g] != v) z = tri[3 * n + g];
                if (!in_circle(p[u], p[v], p[w], p[z])) continue;
                if (!(orient(p[u], p[z], p[w]) > 0.0 && orient(p[z], p[v], p[w]) > 0.0)) continue;      // (never a triangle without area)
                if (++flips > max_flips) return fail(SDM_ERR_INVALID, "the points cannot be triangulated");
                owner[(size_t)u * K + v] = -1; owner[(size_t)v * K + u] = -1;
                tri[3 * t] = u; tri[3 * t + 1] = z; tri[3 * t + 2] = w;
                tri[3 * n] = z; tri[3 * n + 1] = v; tri[3 * n + 2] = w;
                claim(t); claim(n);
                changed = true;
                e = -1;                                       // triangle t has new edges: look at them from the start
            }
    }
    tris.swap(tri);
    return SDM_OK;
}

// sdm_warp_crops_tensor (filter null) and sdm_warp_crops_tensor_filtered: the same checks, the same fit, one launch behind it.  The
// device buffer holds the records, the matrices and -- filtered -- the triangles' (Sx, Sy) behind them, so one copy brings all home.
int warp_tensor_call(sdm_ctx* c, const sdm_align_tensor* spec, const sdm_align_filter* filter, bool filtered, void* out_dev,
                     float* matrices_host, int* flags_host, int* samples_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    sdm_ctx::Warp& w = c->warp;
    if (w.T < 1 || w.L != c->L) return fail(SDM_ERR_INVALID, "no mesh (sdm_warp_set_mesh first)");
    const int N = c->N, L = c->L, T = w.T;
    if (N < 1) return fail(SDM_ERR_INVALID, "no current rows (sdm_set_x, sdm_detect_batch or sdm_track_step first)");
    int rc;
    if ((rc = align_check_spec(spec)) || (filtered && (rc = align_check_filter(filter))) || (rc = align_check_out(out_dev)) ||
        (rc = align_check_rows(c)))
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t rec = (size_t)N * sizeof(WarpFace), mat = (size_t)N * T * 6 * sizeof(float), smp = (size_t)N * T * 2 * sizeof(int);
    if ((rc = w.rows.ensure(rec + mat + (filtered ? smp : 0)))) return rc;
    WarpFace* faces = (WarpFace*)w.rows.p;
    float* matrices = (float*)(w.rows.p + rec);
    const int* img_idx = c->idx_identity ? nullptr : c->img_idx.p;
    sdm_launch_warp_fit(c->x[c->cur].p, N, L, w.lm.p, w.K, (const WarpTri*)w.tri.p, T, align_source_dev(c), img_idx, faces, matrices,
                        c->stream);
    HIP_TRY(hipGetLastError());
    const AlignTapSource src = align_tap_source(c);
    if (filtered)
        sdm_launch_warp_area(src.base, faces, matrices, T, w.labels.p, src.frames, img_idx, src.stack_format, N, w.out_w, w.out_h,
                             spec->dtype, spec->layout, spec->channels, align_tensor_dev(spec), align_area_dev(filter),
                             (int*)(w.rows.p + rec + mat), out_dev, c->stream);
    else
        sdm_launch_warp_tensor(src.base, faces, matrices, T, w.labels.p, src.frames, img_idx, src.stack_format,
                               N, w.out_w, w.out_h, spec->dtype, spec->layout, spec->channels, align_tensor_dev(spec), out_dev, c->stream);
    HIP_TRY(hipGetLastError());
    // the records, the matrices and the samples in one copy, one synchronise
    std::vector<unsigned char> host;
    if (matrices_host || flags_host || samples_host) {
        host.resize(samples_host ? rec + mat + smp : matrices_host ? rec + mat : rec);
        HIP_TRY(hipMemcpyAsync(host.data(), w.rows.p, host.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags_host)
        for (int r = 0; r < N; ++r) flags_host[r] = ((const WarpFace*)host.data())[r].flags;
    if (matrices_host) memcpy(matrices_host, host.data() + rec, mat);
    if (samples_host) memcpy(samples_host, host.data() + rec + mat, smp);
    return SDM_OK;
}

}  // namespace

extern "C" {

int sdm_warp_delaunay(const float* xy, int K, int* triangles, int capacity, int* n_triangles)
{
    if (!xy || !triangles || !n_triangles) return fail(SDM_ERR_INVALID, "null argument");
    if (K < 3 || K > 255) return fail(SDM_ERR_INVALID, "K must be in [3, 255]");
    std::vector<P2> p((size_t)K);
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(xy[2 * k]) || !std::isfinite(xy[2 * k + 1])) return fail(SDM_ERR_INVALID, "a point is not finite");
        p[k].x = (double)xy[2 * k]; p[k].y = (double)xy[2 * k + 1];
    }
    std::vector<int> tri;
    int rc = delaunay(p, tri);
    if (rc) return rc;
    const int T = (int)tri.size() / 3;
    if (T > capacity) return fail(SDM_ERR_INVALID, "capacity too small: " + std::to_string(T) + " triangles");
    memcpy(triangles, tri.data(), tri.size() * sizeof(int));
    *n_triangles = T;
    return SDM_OK;
}

int sdm_warp_set_mesh(sdm_ctx* c, const int* lm, const float* tmpl, int K, const int* triangles, int T, int out_w, int out_h)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    const int L = c->L;
    if (!lm || !tmpl || !triangles) return fail(SDM_ERR_INVALID, "no landmark indices, template or triangles");
    int rc;
    if ((rc = check_landmark_subset(c, lm, tmpl, K, 3))) return rc;
    if (T < 1 || T > SDM_WARP_MAX_TRIANGLES) return fail(SDM_ERR_INVALID, "T must be in [1, 254]");
    if (out_w < 1 || out_w > 1024 || out_h < 1 || out_h > 1024) return fail(SDM_ERR_INVALID, "crop width and height must be in [1, 1024]");
    std::vector<WarpTri> tab((size_t)T);
    struct Ccw { double ax, ay, bx, by, cx, cy; };
    std::vector<Ccw> ccw((size_t)T);
    for (int t = 0; t < T; ++t) {
        const int a = triangles[3 * t], b = triangles[3 * t + 1], cc = triangles[3 * t + 2];
        if (a < 0 || a >= K || b < 0 || b >= K || cc < 0 || cc >= K)
            return fail(SDM_ERR_INVALID, "triangle " + std::to_string(t) + " names a position outside 0 .. K - 1");
        if (a == b || b == cc || a == cc) return fail(SDM_ERR_INVALID, "triangle " + std::to_string(t) + " names a position twice");
        const double ax = (double)tmpl[2 * a], ay = (double)tmpl[2 * a + 1];
        const double ux = (double)tmpl[2 * b] - ax, uy = (double)tmpl[2 * b + 1] - ay;
        const double vx = (double)tmpl[2 * cc] - ax, vy = (double)tmpl[2 * cc + 1] - ay;
        const double D = ux * vy - uy * vx;
        if (!std::isfinite(D) || D == 0.0) return fail(SDM_ERR_INVALID, "triangle " + std::to_string(t) + " has no area in the template");
        WarpTri& w = tab[t];
        w.g[0] = vy / D; w.g[1] = -vx / D; w.g[2] = -uy / D; w.g[3] = ux / D;
        w.qa[0] = ax; w.qa[1] = ay; w.D = D;
        w.ia = lm[a]; w.ib = lm[b]; w.ic = lm[cc]; w.pad = 0;
        const int b2 = D > 0.0 ? b : cc, c2 = D > 0.0 ? cc : b;       // the labels' counter-clockwise order
        ccw[t] = {ax, ay, (double)tmpl[2 * b2], (double)tmpl[2 * b2 + 1], (double)tmpl[2 * c2], (double)tmpl[2 * c2 + 1]};
    }
    // the label map: the lowest-numbered triangle whose three edge functions are >= 0 at the pixel centre
    std::vector<uint8_t> labels((size_t)out_w * out_h, (uint8_t)SDM_WARP_NO_TRIANGLE);
    for (int i = 0; i < out_h; ++i)
        for (int j = 0; j < out_w; ++j) {
            const double x = (double)j, y = (double)i;
            for (int t = 0; t < T; ++t) {
                const Ccw& q = ccw[t];
                const double e0 = (q.bx - q.ax) * (y - q.ay) - (q.by - q.ay) * (x - q.ax);
                if (!(e0 >= 0.0)) continue;
                const double e1 = (q.cx - q.bx) * (y - q.by) - (q.cy - q.by) * (x - q.bx);
                if (!(e1 >= 0.0)) continue;
                const double e2 = (q.ax - q.cx) * (y - q.cy) - (q.ay - q.cy) * (x - q.cx);
                if (!(e2 >= 0.0)) continue;
                labels[(size_t)i * out_w + j] = (uint8_t)t;
                break;
            }
        }
    // ---- everything is checked: the device copies, then the commit ----
    sdm_ctx::Warp& w = c->warp;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));                  // (a warp in flight still reads the previous tables)
    if ((rc = w.labels.ensure((labels.size() + 3) & ~(size_t)3)) || (rc = w.tri.ensure((size_t)SDM_WARP_MAX_TRIANGLES * sizeof(WarpTri))) ||
        (rc = w.lm.ensure((size_t)L)))
        { w.drop(); return rc; }
    hipError_t e = hipMemcpyAsync(w.labels.p, labels.data(), labels.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w.tri.p, tab.data(), tab.size() * sizeof(WarpTri), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w.lm.p, lm, (size_t)K * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { w.drop(); return fail(SDM_ERR_HIP, std::string("sdm_warp_set_mesh: ") + hipGetErrorString(e)); }
    w.K = K; w.T = T; w.L = L; w.out_w = out_w; w.out_h = out_h;
    w.labels_host.swap(labels);
    w.lm_host.assign(lm, lm + K);
    return SDM_OK;
}

int sdm_warp_get_labels(sdm_ctx* c, uint8_t* labels_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (!labels_host) return fail(SDM_ERR_INVALID, "no output");
    const sdm_ctx::Warp& w = c->warp;
    if (w.T < 1 || w.L != c->L) return fail(SDM_ERR_INVALID, "no mesh (sdm_warp_set_mesh first)");
    memcpy(labels_host, w.labels_host.data(), w.labels_host.size());
    return SDM_OK;
}

int sdm_warp_crops_tensor(sdm_ctx* c, const sdm_align_tensor* spec, void* out_dev, float* matrices_host, int* flags_host)
{
    return warp_tensor_call(c, spec, nullptr, false, out_dev, matrices_host, flags_host, nullptr);
}

int sdm_warp_crops_tensor_filtered(sdm_ctx* c, const sdm_align_tensor* spec, const sdm_align_filter* filter, void* out_dev,
                                   float* matrices_host, int* flags_host, int* samples_host)
{
    return warp_tensor_call(c, spec, filter, true, out_dev, matrices_host, flags_host, samples_host);
}

}  // extern "C"
