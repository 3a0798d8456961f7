// Host build of the planar-frame paths of the shared device headers (include/sdm.h, "Planar colour frames"): the pixel fetch of the crop
// tensors (superviseddescent_amd/csrc/sdm_align_tensor_device.h, align_fetch_segment), the area sums of the rigid crop and of the warp
// (sdm_align_area_device.h, sdm_warp_area_device.h) and the pastes' load / apply / store (sdm_paste_device.h through paste_pixel of
// sdm_align_paste_device.h), run by tests/test_planar_host.py under -fsanitize=address,undefined.  A planar frame lives in ONE heap block
// of exactly the bytes it owns -- from the first byte of its lowest plane to the last pixel of the last row of its highest --, so a load
// or store that leaves it is reported.  Every result is compared with that of the SAME functions on the interleaved frame of the same
// pixels, which lives in a block of its own; after a paste every byte between the planes and in the pitch padding must still hold the
// sentinel.  Planes at the default distance, at a padded odd one and at a negative one; faces that cross all four borders; frames 2 pixels
// wide and 1 x 1.  No device, no HIP, no case file: the program draws its own cases and returns 1 at the first difference.
//   usage: planar_host
#include "../../superviseddescent_amd/csrc/sdm_align_area_device.h"
#include "../../superviseddescent_amd/csrc/sdm_warp_area_device.h"
#include "../../superviseddescent_amd/csrc/sdm_align_paste_device.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

const uint8_t SENTINEL = 0xA5;

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint8_t byte() { return (uint8_t)(next() >> 7); }
};

// a planar frame of w x h pixels in a block of exactly its bytes; kind 0: D = h * stride, 1: D = h * stride + 7 (odd: planes misaligned
// against each other), 2: D = -(h * stride + 5) (data is the HIGHEST plane)
struct Planar {
    std::unique_ptr<uint8_t[]> mem;
    uint8_t* p0;
    long long D, bytes;
    int w, h, stride;
    uint8_t* at(int c, int y, int x) const { return p0 + c * D + (long long)y * stride + x; }
};

Planar make_planar(int w, int h, int stride, int kind)
{
    Planar f;
    f.w = w; f.h = h; f.stride = stride;
    const long long plane = (long long)(h - 1) * stride + w, gap = (long long)h * stride + (kind == 1 ? 7 : kind == 2 ? 5 : 0);
    f.D = kind == 2 ? -gap : gap;
    f.bytes = 2 * gap + plane;
    f.mem.reset(new uint8_t[f.bytes]);
    for (long long i = 0; i < f.bytes; ++i) f.mem[i] = SENTINEL;
    f.p0 = f.mem.get() + (kind == 2 ? 2 * gap : 0);
    return f;
}

// the interleaved frame of the same pixels, rows of 3 w + pad bytes, in a block of exactly its bytes
struct Packed {
    std::unique_ptr<uint8_t[]> mem;
    long long bytes;
    int stride;
};

Packed make_packed(const Planar& f, int pad)
{
    Packed q;
    q.stride = 3 * f.w + pad;
    q.bytes = (long long)(f.h - 1) * q.stride + 3 * f.w;
    q.mem.reset(new uint8_t[q.bytes]);
    for (long long i = 0; i < q.bytes; ++i) q.mem[i] = SENTINEL;
    for (int y = 0; y < f.h; ++y)
        for (int x = 0; x < f.w; ++x)
            for (int c = 0; c < 3; ++c) q.mem[(long long)y * q.stride + 3 * x + c] = *f.at(c, y, x);
    return q;
}

void fill(Planar& f, Rng& rng)
{
    for (int c = 0; c < 3; ++c)
        for (int y = 0; y < f.h; ++y)
            for (int x = 0; x < f.w; ++x) *f.at(c, y, x) = rng.byte();
}

int failures = 0;
void expect(bool ok, const char* what, int a, int b, int c)
{
    if (ok) return;
    if (failures++ < 10) std::fprintf(stderr, "MISMATCH %s (%d, %d, %d)\n", what, a, b, c);
}

bool same(const uint32_t a[4][3], const uint32_t b[4][3], int npx)
{
    for (int k = 0; k < npx; ++k)
        for (int c = 0; c < 3; ++c)
            if (a[k][c] != b[k][c]) return false;
    return true;
}

// crop -> frame matrices whose crops of cw x ch reach over every border of a w x h frame: scale, rotation, a centre near each border
std::vector<std::vector<float>> matrices(int w, int h, int cw, int ch)
{
    std::vector<std::vector<float>> out;
    const float centres[5][2] = {{0.5f * w, 0.5f * h}, {-0.7f, 0.4f * h}, {w - 0.3f, 0.6f * h}, {0.45f * w, -0.6f}, {0.55f * w, h - 0.4f}};
    const float forms[4][2] = {{1.0f, 0.0f}, {0.61f, 0.35f}, {2.3f, -0.8f}, {-3.1f, 3.4f}};          // (a, b): [a -b; b a]
    for (const auto& ctr : centres)
        for (const auto& fm : forms) {
            const float a = fm[0], b = fm[1];
            out.push_back({a, -b, ctr[0] - (a * 0.5f * cw - b * 0.5f * ch), b, a, ctr[1] - (b * 0.5f * cw + a * 0.5f * ch)});
        }
    out.push_back({0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f});                                      // degenerate: every pixel the same position
    out.push_back({1.0f, 0.0f, 3.0e6f, 0.0f, 1.0f, 0.0f});                                    // beyond the 2^20 rule: nothing is read
    return out;
}

template <bool WIDE>
void fetch_case(const Planar& f, const Packed& q, int fmt_planar, int fmt_packed, int id)
{
    const int cw = 11, ch = 7;
    AlignRow rp{}, ri{};
    rp.w = ri.w = f.w; rp.h = ri.h = f.h;
    rp.stride = f.stride; rp.format = fmt_planar; rp.p0 = f.p0; rp.pd = f.D;
    ri.stride = q.stride; ri.format = fmt_packed; ri.p0 = q.mem.get();
    WarpAreaRec rec[2];
    int mi = 0;
    for (const auto& m : matrices(f.w, f.h, cw, ch)) {
        for (int e = 0; e < 6; ++e) rp.m[e] = ri.m[e] = rec[0].m[e] = rec[1].m[e] = m[e];
        rec[0].Sx = 1 + mi % 3; rec[0].Sy = 1 + (mi / 3) % 4; rec[1].Sx = 4; rec[1].Sy = 2;
        for (int i = 0; i < ch; ++i)
            for (int j0 = 0; j0 < cw; j0 += 4) {
                const int npx = cw - j0 < 4 ? cw - j0 : 4;
                uint32_t a[4][3], b[4][3];
                align_segment<WIDE>(rp, i, j0, npx, a);
                align_segment<WIDE>(ri, i, j0, npx, b);
                expect(same(a, b, npx), "bilinear fetch", id, mi, i * 100 + j0);
                for (int S = 2; S <= 3; ++S) {
                    align_area_segment<WIDE>(rp, i, j0, npx, S, a);
                    align_area_segment<WIDE>(ri, i, j0, npx, S, b);
                    expect(same(a, b, npx), "area fetch", id, mi, i * 100 + j0);
                }
                const int lab[4] = {0, npx > 1 ? 1 : -1, npx > 2 ? 0 : -1, npx > 3 ? 1 : -1};
                warp_area_segment<WIDE>(rp, rec, lab, i, j0, a);
                warp_area_segment<WIDE>(ri, rec, lab, i, j0, b);
                expect(same(a, b, npx), "warp area fetch", id, mi, i * 100 + j0);
            }
        ++mi;
    }
}

// two overlapping rows (and a third that lies outside) pasted into the planar frame and into its interleaved copy, in descending row
// order as align_paste_host does it; channels 1 | 3, one opacity map per row
void paste_case(Planar& f, int fmt_planar, int fmt_packed, int channels, Rng& rng, int id)
{
    Packed q = make_packed(f, 4);
    const int cw = 6, ch = 5, rows_n = 3;
    PasteCropDev c{};
    c.cw = cw; c.ch = ch; c.dtype = SDM_ALIGN_U8; c.channels = channels; c.t.order = id & 1 ? SDM_ALIGN_ORDER_RGB : SDM_ALIGN_ORDER_BGR;
    align_gray_weights(14 + (id & 1), c.t);
    for (int e = 0; e < 3; ++e) { c.t.scale[e] = 1.0f; c.t.bias[e] = 0.0f; }
    const int tb = rows_n * channels * cw * ch, ab = rows_n * cw * ch;
    std::unique_ptr<uint8_t[]> tensor(new uint8_t[tb]), alpha(new uint8_t[ab]);
    for (int i = 0; i < tb; ++i) tensor[i] = rng.byte();
    for (int i = 0; i < ab; ++i) alpha[i] = (i % 7 == 0) ? 0 : (i % 5 == 0) ? 255 : rng.byte();
    c.in = tensor.get(); c.alpha = alpha.get();
    paste_crop_layout(c, id & 2 ? SDM_ALIGN_NHWC : SDM_ALIGN_NCHW, true);
    // crop -> frame: the crop blown up over the frame's borders; the same shifted by a fraction (overlapping); one far outside
    const float sx = (f.w + 3.0f) / cw, sy = (f.h + 3.0f) / ch;
    const float m[rows_n][6] = {{sx, 0.0f, -1.5f, 0.0f, sy, -1.5f}, {0.8f * sx, 0.2f, 0.4f, -0.2f, 0.8f * sy, 0.3f}, {1.0f, 0.0f, 5000.0f, 0.0f, 1.0f, 5000.0f}};
    PasteFrameDev fp{}, fi{};
    fp.p = f.p0; fp.stride = f.stride; fp.plane = f.D; fp.format = fmt_planar;
    fi.p = q.mem.get(); fi.stride = q.stride; fi.format = fmt_packed;
    fp.w = fi.w = f.w; fp.h = fi.h = f.h; fp.row_end = fi.row_end = rows_n;
    std::vector<PasteRow> rows((size_t)rows_n);
    int list[rows_n];
    for (int r = 0; r < rows_n; ++r) {
        list[r] = r;
        paste_prepare_row(m[r], -1, 0, f.w, f.h, cw, ch, rows[r]);
    }
    for (int r = rows_n - 1; r >= 0; --r)
        for (int Y = rows[r].y0; Y < rows[r].y1; ++Y)
            for (int X = rows[r].x0; X < rows[r].x1; ++X) {
                paste_pixel(fp, rows.data(), list, r, c, X, Y);
                paste_pixel(fi, rows.data(), list, r, c, X, Y);
            }
    // the pixels: plane c of the planar frame is byte c of the interleaved one; everything else in the block is still the sentinel
    std::vector<char> pixel((size_t)f.bytes, 0);
    for (int cc = 0; cc < 3; ++cc)
        for (int y = 0; y < f.h; ++y)
            for (int x = 0; x < f.w; ++x) {
                expect(*f.at(cc, y, x) == q.mem[(long long)y * q.stride + 3 * x + cc], "pasted byte", id, y * 1000 + x, cc);
                pixel[(size_t)(f.at(cc, y, x) - f.mem.get())] = 1;
            }
    for (long long i = 0; i < f.bytes; ++i)
        if (!pixel[(size_t)i]) expect(f.mem[i] == SENTINEL, "byte outside the planes", id, (int)i, 0);
}

}  // namespace

int main()
{
    Rng rng{20240611u};
    const int sizes[4][3] = {{23, 17, 23}, {23, 17, 29}, {2, 9, 2}, {1, 1, 1}};          // w, h, stride
    int id = 0, pasted_any = 0;
    for (const auto& s : sizes)
        for (int kind = 0; kind < 3; ++kind)
            for (int rgb = 0; rgb < 2; ++rgb, ++id) {
                Planar f = make_planar(s[0], s[1], s[2], kind);
                fill(f, rng);
                const Packed q = make_packed(f, 5);
                const int fp = rgb ? SDM_FRAME_RGB_PLANAR : SDM_FRAME_BGR_PLANAR, fi = rgb ? SDM_FRAME_RGB : SDM_FRAME_BGR;
                fetch_case<false>(f, q, fp, fi, id);
                fetch_case<true>(f, q, fp, fi, id);
                for (int channels = 1; channels <= 3; channels += 2) {
                    Planar g = make_planar(s[0], s[1], s[2], kind);
                    fill(g, rng);
                    const std::vector<uint8_t> before(g.mem.get(), g.mem.get() + g.bytes);
                    paste_case(g, fp, fi, channels, rng, id);
                    for (long long i = 0; i < g.bytes; ++i) pasted_any += before[(size_t)i] != g.mem[i];
                }
            }
    if (!pasted_any) { std::fprintf(stderr, "no paste changed a byte\n"); return 1; }
    if (failures) { std::fprintf(stderr, "%d mismatches\n", failures); return 1; }
    std::printf("%d cases, %d bytes pasted\n", id, pasted_any);
    return 0;
}
