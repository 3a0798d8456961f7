// Host build of the arithmetic of sdm_align_region_mask (superviseddescent_amd/csrc/sdm_region_mask_device.h), run by
// tests/test_region_mask_host.py under -fsanitize=address,undefined: a row's points, the hulls' sort buffer, the vertex buffer and the
// map each live in a heap block of exactly the bytes they own, so a load or store that leaves them is reported.  A row is drawn as the
// kernels do it: the row's record, every polygon's vertices -- in DESCENDING polygon order, since the result must not depend on it --,
// then every pixel of the crop through region_pixel.  No device, no HIP.
//   usage: region_mask_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 w, h, n_polygons, n_holes, hull_bits; float32 grow, feather; n_polygons int32 sizes;
//               int32 n_rows; per row: 6 float32 M, int32 bytes + the P x 2 float32 frame points
//   out.bin     per row: int32 flags, n_polygons int32 counts, per polygon its count x 2 float32 vertices, then the w * h bytes of the map
#include "../../superviseddescent_amd/csrc/sdm_region_mask_device.h"

#include "host_case.hpp"

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: region_mask_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n = get<int>(in);
    int rows_seen = 0;
    for (int k = 0; k < n; ++k) {
        RegionDev r{};
        const int w = get<int>(in), h = get<int>(in);
        r.n_polygons = get<int>(in); r.n_holes = get<int>(in); r.hull_bits = (unsigned)get<int>(in);
        r.grow = get<float>(in); r.feather = get<float>(in);
        if (r.n_polygons < 1 || r.n_polygons > REGION_MAX_POLYGONS) { std::fprintf(stderr, "bad case\n"); return 2; }
        for (int g = 0; g < r.n_polygons; ++g) r.size[g] = get<int>(in);
        region_layout(r);
        const int n_rows = get<int>(in);
        for (int row_i = 0; row_i < n_rows; ++row_i, ++rows_seen) {
            float m[6], wm[6];
            for (float& v : m) v = get<float>(in);
            int pb;
            const std::unique_ptr<uint8_t[]> points = block(in, pb);
            if (pb != r.P * 2 * (int)sizeof(float)) { std::fprintf(stderr, "bad points\n"); return 2; }
            const std::unique_ptr<float[]> sorted(new float[2 * r.P]), verts(new float[4 * r.P]);
            const std::unique_ptr<uint8_t[]> map(new uint8_t[(size_t)w * h]);
            const RegionPairs pts{(const float*)points.get()};
            int flags;
            const bool usable = region_inverse(m, -1, wm, flags);
            RegionRow row{};
            region_prepare_row(r, wm, pts, usable, flags, row);
            for (int g = r.n_polygons - 1; g >= 0; --g)
                row.count[g] = region_row_empty(row.flags) ? 0 : region_prepare_polygon(r, g, wm, pts, sorted.get(), verts.get());
            const float reach = region_reach(r.grow, r.feather);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const uint32_t b = region_pixel(r, row, verts.get(), x, y);
                    // the kernel's cull must agree with the formula wherever it would be taken
                    if (!region_row_empty(row.flags) && region_pixel_far(row, reach, (float)x, (float)y) && b != 0u) {
                        std::fprintf(stderr, "case %d row %d pixel (%d, %d): culled, but the formula gives %u\n", k, row_i, x, y, b);
                        return 1;
                    }
                    map[(size_t)y * w + x] = (uint8_t)b;
                }
            out.write((const char*)&row.flags, sizeof(int));
            out.write((const char*)row.count, r.n_polygons * sizeof(int));
            for (int g = 0; g < r.n_polygons; ++g)
                out.write((const char*)(verts.get() + 2 * region_vertex_at(r, g)), (std::streamsize)row.count[g] * 2 * sizeof(float));
            out.write((const char*)map.get(), (std::streamsize)w * h);
        }
    }
    std::printf("%d cases, %d rows\n", n, rows_seen);
    return 0;
}
