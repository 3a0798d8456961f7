// Host build of the arithmetic of sdm_warp_paste_tensor_nv12 (superviseddescent_amd/csrc/sdm_paste_device.h: paste_owned_block on the
// shapes PasteMesh and PasteMeshOwn of sdm_warp_paste_device.h), run by tests/test_warp_paste_nv12_host.py under
// -fsanitize=address,undefined: the Y plane, the UV plane, the tensor, the label map and the opacity maps of a case each live in a heap
// block of exactly the bytes they own (a plane: up to the last byte of its last row), so a load or store that leaves them is reported.
// A case is ONE NV12 frame with its rows; every row's scan, fit and records as tests/cpp/warp_paste_host.cpp makes them, then the block
// ownership rule for every (row, block of the row's box widened to even coordinates) in a SHUFFLED order -- twice, each on the planes as
// the case gives them: through PasteMesh, where every row answers through warp_paste_footprint, and through the adaptor PasteMeshOwn with
// the owner's winners filled by a plain loop over warp_paste_inside (warp_paste_block_winners).  What a block's owner is about to store is
// read from its state before the store.  The kernel's wave-wide strip cull, its ballots and its LDS staging are not here: only the GPU
// tests run them.  No device, no HIP.
//   usage: warp_paste_nv12_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 w, h, stride, cw, ch, dtype, layout, channels, order, gray_shift, n_rows, alpha_mode (0: none,
//               1: one map, 2: one per row), K, T, shuffle seed; float32 scale[3], bias[3]; T x 3 int32 triangle positions; T x 7 float64
//               (G00 G01 G10 G11 qa.x qa.y D); n_rows x K x 2 float32 points; int32 bytes + the label map; int32 bytes + the tensor; int32
//               bytes + the opacity maps; int32 bytes + the Y plane; int32 bytes + the UV plane
//   out.bin     per case: n_rows int32 flags; then per pass (PasteMesh, PasteMeshOwn): h x w bytes -- 1 where the luma byte was stored --,
//               ceil(h/2) x ceil(w/2) bytes -- 1 where the UV pair was stored --, int32 the blocks that were owned twice, the Y plane's
//               bytes, the UV plane's
#include "../../superviseddescent_amd/csrc/sdm_warp_paste_device.h"

#include "host_case.hpp"

#include <algorithm>
#include <cstring>
#include <random>
#include <vector>

struct Unit { int r, bx, by; };

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: warp_paste_nv12_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n = get<int>(in);
    for (int k = 0; k < n; ++k) {
        PasteFrameDev f{};
        f.format = SDM_FRAME_NV12;
        f.w = get<int>(in); f.h = get<int>(in); f.stride = get<int>(in);
        PasteCropDev c{};
        c.cw = get<int>(in); c.ch = get<int>(in); c.dtype = get<int>(in);
        const int layout = get<int>(in);
        c.channels = get<int>(in); c.t.order = get<int>(in);
        align_gray_weights(get<int>(in), c.t);
        const int rows_n = get<int>(in), alpha_mode = get<int>(in), K = get<int>(in), T = get<int>(in), seed = get<int>(in);
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
        int lb, tb, ab, yb, ub;
        const std::unique_ptr<uint8_t[]> labels = block(in, lb), tensor = block(in, tb), alpha = block(in, ab), luma = block(in, yb),
                                         chroma = block(in, ub);
        c.in = tensor.get(); c.alpha = alpha_mode ? alpha.get() : nullptr;
        paste_crop_layout(c, layout, alpha_mode == 2);
        f.row_begin = 0; f.row_end = rows_n;
        std::vector<WarpPasteRow> rows((size_t)rows_n);
        std::vector<WarpPasteTri> recs((size_t)rows_n * T);
        std::vector<int> list((size_t)rows_n);
        std::vector<Unit> units;
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
                float m[6];
                if (s.bad) for (int e = 0; e < 6; ++e) m[e] = __builtin_nanf("");
                else folded = warp_fit_triangle(tri[t], pa, pb, pc, m) || folded;
                warp_paste_triangle(m, pa, pb, pc, rows[r].x0, rows[r].y0, rows[r].x1, rows[r].y1, recs[(size_t)r * T + t]);
            }
            if (!s.bad && folded) rows[r].flags |= SDM_WARP_FOLDED;
            if (rows[r].x1 <= rows[r].x0 || rows[r].y1 <= rows[r].y0) continue;
            for (int by = rows[r].y0 >> 1; by < (rows[r].y1 + 1) >> 1; ++by)
                for (int bx = rows[r].x0 >> 1; bx < (rows[r].x1 + 1) >> 1; ++bx) units.push_back(Unit{r, bx, by});
        }
        std::mt19937 rng((unsigned)seed);
        std::shuffle(units.begin(), units.end(), rng);
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&rows[r].flags, sizeof(int));
        const int bw = (f.w + 1) / 2, bh = (f.h + 1) / 2;
        const PasteMesh mesh{rows.data(), recs.data(), T, labels.get()};
        for (int pass = 0; pass < 2; ++pass) {
            // each pass on planes of its own, exactly their bytes
            std::unique_ptr<uint8_t[]> y(new uint8_t[yb > 0 ? yb : 1]), uv(new uint8_t[ub > 0 ? ub : 1]);
            std::memcpy(y.get(), luma.get(), (size_t)yb);
            std::memcpy(uv.get(), chroma.get(), (size_t)ub);
            f.p = y.get();
            std::vector<char> stored_y((size_t)f.w * f.h, 0), stored_uv((size_t)bw * bh, 0), owners((size_t)bw * bh, 0);
            int twice = 0;
            for (const Unit& u : units) {
                PasteBlock s;
                bool owned;
                if (pass == 0) owned = paste_owned_block_state(f, uv.get(), mesh, list.data(), u.r, c, u.bx, u.by, s);
                else {
                    const WarpPasteTri* own = &recs[(size_t)u.r * T];
                    const uint32_t winners = warp_paste_block_winners(rows[u.r], own, T, u.bx, u.by);
                    owned = winners != 0xffffffffu &&
                            paste_owned_block_state(f, uv.get(), PasteMeshOwn{mesh, u.r, winners, own}, list.data(), u.r, c, u.bx, u.by, s);
                }
                if (!owned) continue;
                twice += owners[(size_t)u.by * bw + u.bx]++ ? 1 : 0;
                for (int i = 0; i < 4; ++i)
                    if (s.wrote >> i & 1) stored_y[(size_t)(2 * u.by + (i >> 1)) * f.w + 2 * u.bx + (i & 1)] = 1;
                if (s.wrote & 16) stored_uv[(size_t)u.by * bw + u.bx] = 1;
                paste_block_store(s);
            }
            out.write(stored_y.data(), (std::streamsize)stored_y.size());
            out.write(stored_uv.data(), (std::streamsize)stored_uv.size());
            out.write((const char*)&twice, sizeof(int));
            out.write((const char*)y.get(), yb);
            out.write((const char*)uv.get(), ub);
        }
    }
    std::printf("%d cases\n", n);
    return 0;
}
