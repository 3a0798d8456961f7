// sdm_capi_mask.hip -- C-ABI of the landmark region masks (include/sdm.h, "Landmark region masks"): the entry points check every
// argument before anything is launched or changed and enqueue -- fit form -- one copy in (the K indices, the template and the P vertex
// indices), sdm_align_crops' fit, then the two launches of csrc/sdm_region_mask.hip; the _at form one copy in (the matrices and the
// points) and the two launches.  Nothing waits between them; the one synchronise of a call brings the matrices and flags back.  The
// landmark state, the images and the tracker's slots are only read; the workspace -- the rows' records, the hulls' sort buffer and the
// vertex lists -- is sdm_ctx::align.region.
#include "sdm_capi_internal.h"
#include "sdm_region_mask_device.h"

#include <cmath>

namespace {

// what both forms refuse of the region, and the region as the kernels read it
int region_check(const sdm_region_mask* region, RegionDev& r)
{
    if (!region) return fail(SDM_ERR_INVALID, "no region");
    if (!region->sizes) return fail(SDM_ERR_INVALID, "no polygon sizes");
    if (region->n_polygons < 1 || region->n_polygons > REGION_MAX_POLYGONS) return fail(SDM_ERR_INVALID, "n_polygons must be in [1, 8]");
    if (region->n_holes < 0 || region->n_holes >= region->n_polygons) return fail(SDM_ERR_INVALID, "n_holes must be in [0, n_polygons)");
    if (region->hull_bits >> region->n_polygons) return fail(SDM_ERR_INVALID, "a hull bit at or beyond n_polygons");
    r = RegionDev{};
    r.n_polygons = region->n_polygons; r.n_holes = region->n_holes; r.hull_bits = region->hull_bits;
    for (int g = 0; g < region->n_polygons; ++g) {
        if (region->sizes[g] < 3 || region->sizes[g] > REGION_MAX_SIZE) return fail(SDM_ERR_INVALID, "a polygon must have 3 to 128 vertices");
        r.size[g] = region->sizes[g];
    }
    region_layout(r);
    if (r.P > REGION_MAX_POINTS) return fail(SDM_ERR_INVALID, "more than 256 vertices");
    if (!std::isfinite(region->grow) || std::fabs(region->grow) > 1024.0f) return fail(SDM_ERR_INVALID, "grow must be finite and in [-1024, 1024]");
    if (!std::isfinite(region->feather) || region->feather < 0.0f || region->feather > 1024.0f)
        return fail(SDM_ERR_INVALID, "feather must be finite and in [0, 1024]");
    r.grow = region->grow; r.feather = region->feather;
    return SDM_OK;
}

// a call's workspace in align.region: `head` bytes of the _at form's matrices and points, then the records, the sort buffer, the vertices
struct RegionSpace {
    unsigned char* head;
    RegionRow* rows;
    float* sorted;
    float* verts;
};

int region_space(sdm_ctx* c, int N, int P, size_t head_bytes, RegionSpace& ws)
{
    const size_t rows_bytes = (size_t)N * sizeof(RegionRow), sorted_bytes = (size_t)N * P * 2 * sizeof(float);
    int rc;
    if ((rc = c->align.region.ensure(head_bytes + rows_bytes + 3 * sorted_bytes))) return rc;
    ws.head = c->align.region.p;
    ws.rows = (RegionRow*)(ws.head + head_bytes);
    ws.sorted = (float*)(ws.head + head_bytes + rows_bytes);
    ws.verts = ws.sorted + (size_t)N * P * 2;
    return SDM_OK;
}

}  // namespace

extern "C" {

int sdm_align_region_mask(sdm_ctx* c, const int* lm, const float* tmpl, int K, int cw, int ch, const int* vertex_index,
                          const sdm_region_mask* region, uint8_t* out_dev, float* matrices_host, int* flags_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    RegionDev r;
    if ((rc = align_check_call(c, lm, tmpl, K, cw, ch)) || (rc = region_check(region, r))) return rc;
    if (!vertex_index) return fail(SDM_ERR_INVALID, "no vertex indices");
    for (int k = 0; k < r.P; ++k)
        if (vertex_index[k] < 0 || vertex_index[k] >= c->L) return fail(SDM_ERR_INVALID, "vertex index " + std::to_string(vertex_index[k]) + " out of range");
    if ((rc = align_check_out(out_dev)) || (rc = align_check_rows(c))) return rc;
    const int N = c->N;
    sdm_ctx::Align& a = c->align;
    HIP_TRY(hipSetDevice(c->device));
    RegionSpace ws;
    if ((rc = a.in.ensure((size_t)3 * K + r.P)) || (rc = a.faces.ensure((size_t)N)) || (rc = region_space(c, N, r.P, 0, ws))) return rc;
    // one copy in: the K indices, the template, the P vertex indices
    std::vector<int> in((size_t)3 * K + r.P);
    memcpy(in.data(), lm, (size_t)K * sizeof(int));
    memcpy(in.data() + K, tmpl, (size_t)2 * K * sizeof(float));
    memcpy(in.data() + 3 * K, vertex_index, (size_t)r.P * sizeof(int));
    HIP_TRY(hipMemcpyAsync(a.in.p, in.data(), in.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    sdm_launch_align_fit(c->x[c->cur].p, N, c->L, a.in.p, (const float*)(a.in.p + K), K, align_source_dev(c),
                         c->idx_identity ? nullptr : c->img_idx.p, cw, ch, a.faces.p, c->stream);
    HIP_TRY(hipGetLastError());
    sdm_launch_region_prepare(a.faces.p, c->x[c->cur].p, c->L, a.in.p + 3 * K, nullptr, nullptr, N, r, ws.rows, ws.sorted, ws.verts, c->stream);
    HIP_TRY(hipGetLastError());
    sdm_launch_region_raster(ws.rows, ws.verts, N, cw, ch, r, out_dev, c->stream);
    HIP_TRY(hipGetLastError());
    return align_fetch_rows(c, N, matrices_host, flags_host, nullptr);
}

int sdm_align_region_mask_at(sdm_ctx* c, const float* matrices_host, const float* points_host, int n_rows, int cw, int ch,
                             const sdm_region_mask* region, uint8_t* out_dev, int* flags_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (!matrices_host) return fail(SDM_ERR_INVALID, "no matrices");
    if (!points_host) return fail(SDM_ERR_INVALID, "no points");
    if (n_rows < 1) return fail(SDM_ERR_INVALID, "n_rows must be >= 1");
    if (cw < 1 || cw > 1024 || ch < 1 || ch > 1024) return fail(SDM_ERR_INVALID, "crop width and height must be in [1, 1024]");
    int rc;
    RegionDev r;
    if ((rc = region_check(region, r)) || (rc = align_check_out(out_dev))) return rc;
    const int N = n_rows;
    HIP_TRY(hipSetDevice(c->device));
    const size_t mats_bytes = (size_t)N * 6 * sizeof(float), points_bytes = (size_t)N * r.P * 2 * sizeof(float);
    RegionSpace ws;
    if ((rc = region_space(c, N, r.P, mats_bytes + points_bytes, ws))) return rc;
    // one copy in: the matrices, then the points
    std::vector<unsigned char> in(mats_bytes + points_bytes);
    memcpy(in.data(), matrices_host, mats_bytes);
    memcpy(in.data() + mats_bytes, points_host, points_bytes);
    HIP_TRY(hipMemcpyAsync(ws.head, in.data(), in.size(), hipMemcpyHostToDevice, c->stream));
    sdm_launch_region_prepare(nullptr, nullptr, 0, nullptr, (const float*)ws.head, (const float*)(ws.head + mats_bytes), N, r, ws.rows, ws.sorted,
                              ws.verts, c->stream);
    HIP_TRY(hipGetLastError());
    sdm_launch_region_raster(ws.rows, ws.verts, N, cw, ch, r, out_dev, c->stream);
    HIP_TRY(hipGetLastError());
    std::vector<RegionRow> host;
    if (flags_host) {
        host.resize((size_t)N);
        HIP_TRY(hipMemcpyAsync(host.data(), ws.rows, (size_t)N * sizeof(RegionRow), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t n = 0; n < host.size(); ++n) flags_host[n] = host[n].flags;
    return SDM_OK;
}

}  // extern "C"
