// Host build of the arithmetic of sdm_warp_paste_tensor_filtered (superviseddescent_amd/csrc/sdm_warp_paste_area_device.h on top of
// sdm_warp_paste_device.h, sdm_warp_area_device.h and sdm_align_paste_area_device.h), run by tests/test_warp_paste_area_host.py under
// -fsanitize=address,undefined: the frame (an NV12 frame: each plane), the tensor, the label map and the opacity maps of a case each live
// in a heap block of exactly the bytes they own, so a load or store that leaves them is reported.  A case is ONE frame with its rows:
// per row the scan, every triangle's fit, record and counts as the kernels make them, then the ownership rule for every pixel (NV12: 2 x 2
// block) of every row's box -- once with the rows in DESCENDING order through the shape PasteMeshArea, once in ascending order through
// PasteMeshAreaOwn with the owner's triangle (NV12: its block's winners) found by a plain loop, each pass on the frame as the case gives it.
// The kernel's wave-wide strip cull, its ballots and its LDS staging are not here: only the GPU tests run them.  No device, no HIP.
//   usage: warp_paste_area_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 format, w, h, stride, cw, ch, dtype, layout, channels, order, gray_shift, n_rows, alpha_mode
//               (0: none, 1: one map, 2: one per row), K, T, filter mode, max_samples; float32 min_scale, scale[3], bias[3]; T x 3 int32
//               triangle positions; T x 7 float64 (G00 G01 G10 G11 qa.x qa.y D); n_rows x K x 2 float32 points; int32 bytes + the label map;
//               int32 bytes + the tensor; int32 bytes + the opacity maps; int32 bytes + the frame (NV12: the Y plane); int32 bytes + the UV
//               plane (0 bytes unless NV12)
//   out.bin     per case: n_rows int32 flags, n_rows x T x 6 float32 A_t, n_rows x T x 6 float32 W_t, n_rows x T x 2 int32 (Sx, Sy); then
//               per pass: the frame's bytes, the UV plane's bytes
#include "../../superviseddescent_amd/csrc/sdm_warp_paste_area_device.h"

#include "host_case.hpp"

#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: warp_paste_area_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n = get<int>(in);
    for (int k = 0; k < n; ++k) {
        PasteFrameDev f{};
        f.format = get<int>(in); f.w = get<int>(in); f.h = get<int>(in); f.stride = get<int>(in);
        PasteCropDev c{};
        c.cw = get<int>(in); c.ch = get<int>(in); c.dtype = get<int>(in);
        const int layout = get<int>(in);
        c.channels = get<int>(in); c.t.order = get<int>(in);
        align_gray_weights(get<int>(in), c.t);
        const int rows_n = get<int>(in), alpha_mode = get<int>(in), K = get<int>(in), T = get<int>(in);
        const int mode = get<int>(in), max_samples = get<int>(in);
        const float min_scale = get<float>(in);
        const float min2 = min_scale * min_scale;
        for (int e = 0; e < 3; ++e) c.t.scale[e] = get<float>(in);
        for (int e = 0; e < 3; ++e) c.t.bias[e] = get<float>(in);
        std::vector<WarpTri> tri((size_t)T);
        for (WarpTri& t : tri) { t.ia = get<int>(in); t.ib = get<int>(in); t.ic = get<int>(in); t.pad = 0; }
        for (WarpTri& t : tri) {
            for (int e = 0; e < 4; ++e) t.g[e] = get<double>(in);
            t.qa[0] = get<double>(in); t.qa[1] = get<double>(in); t.D = get<double>(in);
        }
        std::vector<float> pts((size_t)rows_n * K * 2);
        for (float& v : pts) v = get<float>(in);
        int lb, tb, ab, fb, ub;
        const std::unique_ptr<uint8_t[]> labels = block(in, lb), tensor = block(in, tb), alpha = block(in, ab), frame = block(in, fb),
                                         chroma = block(in, ub);
        c.in = tensor.get(); c.alpha = alpha_mode ? alpha.get() : nullptr;
        paste_crop_layout(c, layout, alpha_mode == 2);
        f.row_begin = 0; f.row_end = rows_n;
        std::vector<WarpPasteRow> rows((size_t)rows_n);
        std::vector<WarpPasteTri> recs((size_t)rows_n * T);
        std::vector<WarpPasteCounts> counts((size_t)rows_n * T);
        std::vector<float> mats((size_t)rows_n * T * 6);
        std::vector<int> list((size_t)rows_n);
        for (int r = 0; r < rows_n; ++r) {
            list[r] = r;
            const float* p = &pts[(size_t)r * K * 2];
            WarpPasteScan s;
            warp_paste_scan_init(s);
            for (int j = 0; j < K; ++j) warp_paste_scan_point(p[2 * j], p[2 * j + 1], f.w, f.h, s);
            warp_paste_row(s, false, 0, f.w, f.h, rows[r]);
            bool folded = false;
            for (int t = 0; t < T; ++t) {
                const float* pa = p + 2 * tri[t].ia; const float* pb = p + 2 * tri[t].ib; const float* pc = p + 2 * tri[t].ic;
                float* m = &mats[((size_t)r * T + t) * 6];
                if (s.bad) for (int e = 0; e < 6; ++e) m[e] = __builtin_nanf("");
                else folded = warp_fit_triangle(tri[t], pa, pb, pc, m) || folded;
                warp_paste_triangle(m, pa, pb, pc, rows[r].x0, rows[r].y0, rows[r].x1, rows[r].y1, recs[(size_t)r * T + t]);
            }
            if (!s.bad && folded) rows[r].flags |= SDM_WARP_FOLDED;
            for (int t = 0; t < T; ++t)                                        // (the counts stage runs behind the prepare stage: final flags)
                counts[(size_t)r * T + t] = warp_paste_area_counts(recs[(size_t)r * T + t], rows[r].flags, mode, max_samples, min2);
        }
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&rows[r].flags, sizeof(int));
        out.write((const char*)mats.data(), (std::streamsize)(mats.size() * sizeof(float)));
        for (const WarpPasteTri& t : recs) out.write((const char*)t.w, 6 * sizeof(float));
        for (const WarpPasteCounts cnt : counts) {
            const int s2[2] = {cnt & 255, cnt >> 8};
            out.write((const char*)s2, sizeof(s2));
        }
        const PasteMeshArea shape{PasteMesh{rows.data(), recs.data(), T, labels.get()}, counts.data(), -1};
        for (int pass = 0; pass < 2; ++pass) {
            // each pass on planes of its own, exactly their bytes
            std::unique_ptr<uint8_t[]> y(new uint8_t[fb > 0 ? fb : 1]), uv(new uint8_t[ub > 0 ? ub : 1]);
            std::memcpy(y.get(), frame.get(), (size_t)fb);
            std::memcpy(uv.get(), chroma.get(), (size_t)ub);
            f.p = y.get();
            for (int i = 0; i < rows_n; ++i) {
                const int r = pass ? i : rows_n - 1 - i;
                const WarpPasteRow& b = rows[r];
                const WarpPasteTri* own = &recs[(size_t)r * T];
                const WarpPasteCounts* own_counts = &counts[(size_t)r * T];
                if (b.x1 <= b.x0 || b.y1 <= b.y0) continue;
                if (f.format != SDM_FRAME_NV12) {
                    for (int Y = b.y0; Y < b.y1; ++Y)
                        for (int X = b.x0; X < b.x1; ++X) {
                            if (pass == 0) { warp_paste_area_pixel(f, rows.data(), recs.data(), counts.data(), T, list.data(), r, c, labels.get(), X, Y); continue; }
                            AlignPos q;
                            const int mine = warp_paste_footprint_triangle(b, own, T, c.cw, c.ch, X, Y, q);
                            if (mine < 0) continue;
                            PasteMeshAreaOwn shape_own{shape, r, 0xffffffffu, own, own_counts};
                            shape_own.area.tri = mine;
                            paste_owned(f, shape_own, list.data(), r, c, X, Y, q);
                        }
                    continue;
                }
                for (int by = b.y0 >> 1; by < (b.y1 + 1) >> 1; ++by)
                    for (int bx = b.x0 >> 1; bx < (b.x1 + 1) >> 1; ++bx) {
                        if (pass == 0) { paste_owned_block(f, uv.get(), shape, list.data(), r, c, bx, by); continue; }
                        const uint32_t winners = warp_paste_block_winners(b, own, T, bx, by);
                        if (winners != 0xffffffffu)
                            paste_owned_block(f, uv.get(), PasteMeshAreaOwn{shape, r, winners, own, own_counts}, list.data(), r, c, bx, by);
                    }
            }
            out.write((const char*)y.get(), fb);
            out.write((const char*)uv.get(), ub);
        }
    }
    std::printf("%d cases\n", n);
    return 0;
}
