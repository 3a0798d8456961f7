// Host build of the arithmetic of sdm_align_paste_tensor_filtered (superviseddescent_amd/csrc/sdm_align_paste_area_device.h), run by
// tests/test_align_paste_area_host.py under -fsanitize=address,undefined: the frame, the tensor and the opacity maps of a case each live
// in a heap block of exactly the bytes they own (a frame: up to the last pixel of the last row), so a load or store that leaves them is
// reported.  A case is ONE frame with its rows; they are pasted as the kernel does it: every row's prepare, then for every row every
// pixel of its box through paste_area_pixel -- in DESCENDING row order, since the result must not depend on it.  No device, no HIP.
//   usage: align_paste_area_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 format, w, h, stride, cw, ch, dtype, layout, channels, order, gray_shift, n_rows,
//               alpha_mode (0: none, 1: one map, 2: one per row), filter mode, max_samples; float32 min_scale; float32 scale[3], bias[3];
//               n_rows x 6 float32 M; int32 bytes + the tensor; int32 bytes + the opacity maps; int32 bytes + the frame
//   out.bin     per case: n_rows int32 flags, n_rows x 6 float32 W, n_rows x 4 int32 box, n_rows int32 S, n_rows x h x w bytes -- the
//               working footprint (paste_area_holds) over the whole frame --, the frame's bytes
#include "../../superviseddescent_amd/csrc/sdm_align_paste_area_device.h"

#include "host_case.hpp"

#include <vector>

// the unfiltered kernel reads PasteRow as it did before the filtered paste: S and the footprint's reach live beside it
static_assert(sizeof(PasteRow) == 48 && sizeof(PasteAreaRow) == 16, "record sizes");

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: align_paste_area_host <cases.bin> <out.bin>\n"); return 2; }
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
        const int rows_n = get<int>(in), alpha_mode = get<int>(in), mode = get<int>(in), max_samples = get<int>(in);
        const float min_scale = get<float>(in);
        const float min2 = min_scale * min_scale;
        for (int e = 0; e < 3; ++e) c.t.scale[e] = get<float>(in);
        for (int e = 0; e < 3; ++e) c.t.bias[e] = get<float>(in);
        std::vector<float> m((size_t)6 * rows_n);
        for (float& v : m) v = get<float>(in);
        int tb, ab, fb;
        const std::unique_ptr<uint8_t[]> tensor = block(in, tb), alpha = block(in, ab), frame = block(in, fb);
        c.in = tensor.get(); c.alpha = alpha_mode ? alpha.get() : nullptr;
        paste_crop_layout(c, layout, alpha_mode == 2);
        f.p = frame.get(); f.row_begin = 0; f.row_end = rows_n;
        std::vector<PasteRow> rows((size_t)rows_n);
        std::vector<PasteAreaRow> area((size_t)rows_n);
        std::vector<int> list((size_t)rows_n);
        for (int r = 0; r < rows_n; ++r) {
            list[r] = r;
            paste_area_prepare_row(&m[(size_t)6 * r], -1, 0, f.w, f.h, c.cw, c.ch, mode, max_samples, min2, rows[r], area[r]);
        }
        for (int r = rows_n - 1; r >= 0; --r)
            for (int Y = rows[r].y0; Y < rows[r].y1; ++Y)
                for (int X = rows[r].x0; X < rows[r].x1; ++X) paste_area_pixel(f, rows.data(), area.data(), list.data(), r, c, X, Y);
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&rows[r].flags, sizeof(int));
        for (int r = 0; r < rows_n; ++r) out.write((const char*)rows[r].w, 6 * sizeof(float));
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&rows[r].x0, 4 * sizeof(int));
        for (int r = 0; r < rows_n; ++r) out.write((const char*)&area[r].S, sizeof(int));
        std::vector<char> holds((size_t)f.w * f.h);
        for (int r = 0; r < rows_n; ++r) {
            for (int Y = 0; Y < f.h; ++Y)
                for (int X = 0; X < f.w; ++X) {
                    AlignPos q;
                    holds[(size_t)Y * f.w + X] = paste_area_holds(rows[r], area[r], c.cw, c.ch, X, Y, q) ? 1 : 0;
                }
            out.write(holds.data(), (std::streamsize)holds.size());
        }
        out.write((const char*)frame.get(), fb);
    }
    std::printf("%d cases\n", n);
    return 0;
}
