// sdm_region_mask.hip -- landmark region masks on gfx950 (include/sdm.h, "Landmark region masks"), behind the fit of sdm_align_crops or
// a caller's matrices and points.
//
//   region_prepare_kernel   one lane per (row, polygon): the row's W and flags, the polygon's vertices through W into the row's vertex
//                          buffer -- a hull polygon: sorted by insertion, then the monotone chain --, its vertex count; every lane of a
//                          row runs all P points through W for NONFINITE and the box of the polygons that are no holes, the lane of
//                          polygon 0 writes both (and, fit form, the final flags back into the fit's record)
//   region_raster_kernel_t<V>   one workgroup of 256 lanes per (row, band of 256 V map bytes).  The row's edges are staged once in LDS as
//                          (a, e, ee, b.y) records, 24 bytes each, at most 6 KB.  A lane computes the V = 4 or 16 consecutive bytes of
//                          one V-byte aligned piece of the output and stores them with one 4- or 16-byte store; the pieces at a map's
//                          two ends, which it may share with its neighbours' maps, are stored byte by byte.  The edge loop is
//                          wave-uniform: every lane reads the same record (an LDS broadcast) and applies it to its V pixels.  A wave
//                          whose pixels all lie beyond region_reach of the row's box stores zeros without the loop; so does a row that
//                          is DEGENERATE or NONFINITE.  The division stays a division and the square root a square root: both are
//                          correctly rounded as hipcc emits them without fast-math flags.
//
// The arithmetic is csrc/sdm_region_mask_device.h.
#include "sdm_kernels.h"
#include "sdm_region_mask_device.h"

#pragma clang fp contract(off)

namespace {

#define REGION_PREPARE_BLOCK 64
#define REGION_RASTER_BLOCK 256

__global__ __launch_bounds__(REGION_PREPARE_BLOCK) void region_prepare_kernel(AlignFace* __restrict__ faces, const float* __restrict__ x, int L,
                                                                              const int* __restrict__ vidx, const float* __restrict__ mats,
                                                                              const float* __restrict__ points, int N, RegionDev region,
                                                                              RegionRow* __restrict__ rows, float* __restrict__ sorted,
                                                                              float* __restrict__ verts)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= N * region.n_polygons) return;
    const int n = id / region.n_polygons, g = id - n * region.n_polygons;
    float m[6], w[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) m[e] = faces ? faces[n].m[e] : mats[(size_t)6 * n + e];
    int flags;
    const bool usable = region_inverse(m, faces ? faces[n].flags : -1, w, flags);
    float* const row_sorted = sorted + (size_t)2 * region.P * n;
    float* const row_verts = verts + (size_t)4 * region.P * n;
    RegionRow row;
    int count = 0;
    if (faces) {
        const RegionState pts{x + (size_t)2 * L * n, vidx, L};
        region_prepare_row(region, w, pts, usable, flags, row);
        if (!region_row_empty(row.flags)) count = region_prepare_polygon(region, g, w, pts, row_sorted, row_verts);
    } else {
        const RegionPairs pts{points + (size_t)2 * region.P * n};
        region_prepare_row(region, w, pts, usable, flags, row);
        if (!region_row_empty(row.flags)) count = region_prepare_polygon(region, g, w, pts, row_sorted, row_verts);
    }
    rows[n].count[g] = count;
    if (g == 0) {
        rows[n].flags = row.flags;
        rows[n].x0 = row.x0; rows[n].y0 = row.y0; rows[n].x1 = row.x1; rows[n].y1 = row.y1;
        if (faces) faces[n].flags = row.flags;
    }
}

template <int V> struct RegionPiece;
template <> struct RegionPiece<4> { typedef uint32_t type; };
template <> struct RegionPiece<16> { typedef uint4 type; };

template <int V>
__global__ __launch_bounds__(REGION_RASTER_BLOCK) void region_raster_kernel_t(const RegionRow* __restrict__ rows, const float* __restrict__ verts,
                                                                              int cw, int ch, RegionDev region, uint8_t* __restrict__ out)
{
    __shared__ RegionEdge edges[REGION_MAX_POINTS];
    __shared__ RegionRow row_s;
    const int n = blockIdx.x, tid = threadIdx.x;                                     // (rows on x: no 65 535 limit)
    if (tid == 0) row_s = rows[n];
    __syncthreads();
    const RegionRow& row = row_s;                                                    // (read where it lies: the counts are indexed by g)
    const bool empty = region_row_empty(row.flags);
    if (!empty) {
        const float* const row_verts = verts + (size_t)4 * region.P * n;
        for (int g = 0; g < region.n_polygons; ++g) {
            const float* const v = row_verts + 2 * region_vertex_at(region, g);
            const int m = row.count[g];
            for (int k = tid; k < m; k += REGION_RASTER_BLOCK) {
                const int k1 = k + 1 == m ? 0 : k + 1;
                edges[region.start[g] + k] = region_edge(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1]);
            }
        }
    }
    __syncthreads();
    // the map's bytes [0, hw) lie at out + base; piece j holds the map bytes [j V - lead, j V - lead + V), V-byte aligned in out
    const int hw = cw * ch;
    const size_t base = (size_t)n * hw;
    const int lead = (int)(base % V);
    const int j = blockIdx.y * REGION_RASTER_BLOCK + tid;
    const int i0 = j * V - lead;
    if (i0 >= hw) return;
    uint32_t bytes[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bytes[v] = 0u;
    bool need = false;
    float px[V], py[V];
    if (!empty) {
        const float reach = region_reach(region.grow, region.feather);
        const int i = i0 < 0 ? 0 : i0;
        int r = i / cw, c = i - r * cw;
#pragma unroll
        for (int v = 0; v < V; ++v) {                                               // (bytes beyond the map's ends: the end's pixel again, not stored)
            px[v] = (float)c; py[v] = (float)r;
            need = need || !region_pixel_far(row, reach, px[v], py[v]);
            if (i0 + v >= 0 && i0 + v < hw - 1) { if (++c == cw) { c = 0; ++r; } }
        }
    }
    if (__any(need)) {
        float s[V];
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = INFINITY;
        for (int g = 0; g < region.n_polygons; ++g) {
            const RegionEdge* const e = edges + region.start[g];
            const int m = row.count[g];
            float d2[V];
            int wn[V];
#pragma unroll
            for (int v = 0; v < V; ++v) { d2[v] = INFINITY; wn[v] = 0; }
            for (int k = 0; k < m; ++k) {
                const RegionEdge ek = e[k];
#pragma unroll
                for (int v = 0; v < V; ++v) region_edge_pixel(ek, px[v], py[v], d2[v], wn[v]);
            }
            const bool hole = g >= region.n_polygons - region.n_holes;
#pragma unroll
            for (int v = 0; v < V; ++v) s[v] = region_fold(s[v], d2[v], wn[v], hole);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) bytes[v] = region_byte(s[v], region.grow, region.feather);
    }
    uint8_t* const p = out + base + i0;                                             // (i0 < 0: inside the previous map, never below out)
    if (i0 >= 0 && i0 + V <= hw) {
        uint32_t word[V / 4];
#pragma unroll
        for (int v = 0; v < V; v += 4) word[v / 4] = bytes[v] | bytes[v + 1] << 8 | bytes[v + 2] << 16 | bytes[v + 3] << 24;
        typename RegionPiece<V>::type piece;
        memcpy(&piece, word, V);
        *(typename RegionPiece<V>::type*)p = piece;
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (i0 + v >= 0 && i0 + v < hw) p[v] = (uint8_t)bytes[v];
    }
}

}  // namespace

void sdm_launch_region_prepare(AlignFace* faces, const float* x, int L, const int* vidx, const float* mats, const float* points, int N,
                               const RegionDev& region, RegionRow* rows, float* sorted, float* verts, hipStream_t s)
{
    const int lanes = N * region.n_polygons;
    hipLaunchKernelGGL(region_prepare_kernel, dim3((unsigned)((lanes + REGION_PREPARE_BLOCK - 1) / REGION_PREPARE_BLOCK)), dim3(REGION_PREPARE_BLOCK),
                       0, s, faces, x, L, vidx, mats, points, N, region, rows, sorted, verts);
}

// 16 bytes per lane from 64 x 64 on (a band is then a whole 64 x 64 map); 4 below, where a map is a few bands at the most
void sdm_launch_region_raster(const RegionRow* rows, const float* verts, int N, int cw, int ch, const RegionDev& region, uint8_t* out,
                              hipStream_t s)
{
    const int hw = cw * ch;
    if (hw >= 4096) {
        const int pieces = (hw + 15) / 16 + 1;                                       // (+ 1: a map that begins inside a piece)
        hipLaunchKernelGGL(region_raster_kernel_t<16>, dim3((unsigned)N, (unsigned)((pieces + REGION_RASTER_BLOCK - 1) / REGION_RASTER_BLOCK)),
                           dim3(REGION_RASTER_BLOCK), 0, s, rows, verts, cw, ch, region, out);
    } else {
        const int pieces = (hw + 3) / 4 + 1;
        hipLaunchKernelGGL(region_raster_kernel_t<4>, dim3((unsigned)N, (unsigned)((pieces + REGION_RASTER_BLOCK - 1) / REGION_RASTER_BLOCK)),
                           dim3(REGION_RASTER_BLOCK), 0, s, rows, verts, cw, ch, region, out);
    }
}
