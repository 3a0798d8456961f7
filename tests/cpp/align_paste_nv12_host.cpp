// Host build of the arithmetic of sdm_align_paste_tensor_nv12 (superviseddescent_amd/csrc/sdm_paste_device.h: paste_owned_block on the
// shapes of sdm_align_paste_device.h and sdm_align_paste_area_device.h), run by tests/test_align_paste_nv12_host.py under
// -fsanitize=address,undefined: the Y plane, the UV plane, the tensor and the opacity maps of a case each live in a heap block of exactly
// the bytes they own (a plane: up to the last byte of its last row), so a load or store that leaves them is reported.  A case is ONE
// NV12 frame with its rows; they are pasted as the kernel does it: every row's prepare, then the block ownership rule for every
// (row, block of the row's box widened to even coordinates) -- in a SHUFFLED order, since the result must not depend on it.  What a block's
// owner is about to store is read from its state (PasteBlock::wrote) before the store.  No device, no HIP.
//   usage: align_paste_nv12_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 w, h, stride, cw, ch, dtype, layout, channels, order, gray_shift, n_rows, alpha_mode (0: none,
//               1: one map, 2: one per row), filtered (0: plain bilinear), filter mode, max_samples, shuffle seed; float32 min_scale;
//               float32 scale[3], bias[3]; n_rows x 6 float32 M; int32 bytes + the tensor; int32 bytes + the opacity maps; int32 bytes +
//               the Y plane; int32 bytes + the UV plane
//   out.bin     per case: n_rows int32 flags, n_rows int32 S, h x w bytes -- 1 where the luma byte was stored --, ceil(h/2) x ceil(w/2)
//               bytes -- 1 where the UV pair was stored --, int32 the blocks that were owned twice, the Y plane's bytes, the UV plane's
#include "../../superviseddescent_amd/csrc/sdm_align_paste_area_device.h"

#include "host_case.hpp"

#include <algorithm>
#include <random>
#include <vector>

struct Unit { int r, bx, by; };

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: align_paste_nv12_host <cases.bin> <out.bin>\n"); return 2; }
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
        const int rows_n = get<int>(in), alpha_mode = get<int>(in), filtered = get<int>(in), mode = get<int>(in), max_samples = get<int>(in);
        const int seed = get<int>(in);
        const float min_scale = get<float>(in);
        const float min2 = min_scale * min_scale;
        for (int e = 0; e < 3; ++e) c.t.scale[e] = get<float>(in);
        for (int e = 0; e < 3; ++e) c.t.bias[e] = get<float>(in);
        std::vector<float> m((size_t)6 * rows_n);
        for (float& v : m) v = get<float>(in);
        int tb, ab, yb, ub;
        const std::unique_ptr<uint8_t[]> tensor = block(in, tb), alpha = block(in, ab), luma = block(in, yb), chroma = block(in, ub);
        c.in = tensor.get(); c.alpha = alpha_mode ? alpha.get() : nullptr;
        paste_crop_layout(c, layout, alpha_mode == 2);
        f.p = luma.get(); f.row_begin = 0; f.row_end = rows_n;
        std::vector<PasteRow> rows((size_t)rows_n);
        std::vector<PasteAreaRow> area((size_t)rows_n);
        std::vector<int> list((size_t)rows_n);
        std::vector<Unit> units;
        for (int r = 0; r < rows_n; ++r) {
            list[r] = r;
            if (filtered) paste_area_prepare_row(&m[(size_t)6 * r], -1, 0, f.w, f.h, c.cw, c.ch, mode, max_samples, min2, rows[r], area[r]);
            else { paste_prepare_row(&m[(size_t)6 * r], -1, 0, f.w, f.h, c.cw, c.ch, rows[r]); area[r].S = 1; }
            if (rows[r].x1 <= rows[r].x0 || rows[r].y1 <= rows[r].y0) continue;
            for (int by = rows[r].y0 >> 1; by < (rows[r].y1 + 1) >> 1; ++by)
                for (int bx = rows[r].x0 >> 1; bx < (rows[r].x1 + 1) >> 1; ++bx) units.push_back(Unit{r, bx, by});
        }
        std::mt19937 rng((unsigned)seed);
        std::shuffle(units.begin(), units.end(), rng);
        const int bw = (f.w + 1) / 2, bh = (f.h + 1) / 2;
        std::vector<char> stored_y((size_t)f.w * f.h, 0), stored_uv((size_t)bw * bh, 0), owners((size_t)bw * bh, 0);
        int twice = 0;
        for (const Unit& u : units) {
            PasteBlock s;
            const bool owned = filtered ? paste_owned_block_state(f, chroma.get(), PasteRigidArea{rows.data(), area.data()}, list.data(), u.r, c,
                                                                  u.bx, u.by, s)
                                        : paste_owned_block_state(f, chroma.get(), PasteRigid{rows.data()}, list.data(), u.r, c, u.bx, u.by, s);
            if (!owned) continue;
            twice += owners[(size_t)u.by * bw + u.bx]++ ? 1 : 0;
            for (int i = 0; i < 4; ++i)
                if (s.wrote >> i & 1) stored_y[(size_t)(2 * u.by + (i >> 1)) * f.w + 2 * u.bx + (i & 1)] = 1;
            if (s.wrote & 16) stored_uv[(size_t)u.by * bw + u.bx] = 1;
            paste_block_store(s);
        }
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&rows[r].flags, sizeof(int));
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&area[r].S, sizeof(int));
        out.write(stored_y.data(), (std::streamsize)stored_y.size());
        out.write(stored_uv.data(), (std::streamsize)stored_uv.size());
        out.write((const char*)&twice, sizeof(int));
        out.write((const char*)luma.get(), yb);
        out.write((const char*)chroma.get(), ub);
    }
    std::printf("%d cases\n", n);
    return 0;
}
