// Host build of the arithmetic of sdm_warp_crops_tensor (superviseddescent_amd/csrc/sdm_warp_device.h), run by tests/test_warp_host.py
// under -fsanitize=address,undefined: every plane lives in a heap block of exactly the bytes the frame owns (up to the last pixel of the
// last row), so a tap that leaves the frame is reported.  No device, no HIP.
//   usage: warp_host <cases.bin> <out.bin>
//   cases.bin   int32 n_fits, then per fit: float64 G[4], q_a[2], D; float32 p_a[2], p_b[2], p_c[2]
//               int32 n, then per case: int32 format, w, h, stride, cstride, out_w, out_h, T; float32 matrices[T][6]; out_h x out_w label
//               bytes; float32 scale[3], bias[3]; int32 bytes0, bytes0 bytes of plane 0; int32 bytes1, bytes1 bytes of the UV plane
//   out.bin     per fit: float32 A_t[6], int32 folded
//               per case: out_h x out_w x 3 bytes (B, G, R), out_h x out_w bytes (1 channel, gray_shift 14), out_h x out_w bytes
//               (gray_shift 15), 3 x out_h x out_w float32 (RGB planes, v * scale + bias)
// A lane's work is a segment of 4 pixels, as in the warp's kernel (WarpMesh, csrc/sdm_warp.hip): labels, positions through each pixel's own
// matrix, align_fetch_segment.
// exits 1 when the 32-bit and the 64-bit offset paths disagree
#include "../../superviseddescent_amd/csrc/sdm_warp_device.h"

#include "host_case.hpp"

#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: warp_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n_fits = get<int>(in);
    for (int k = 0; k < n_fits; ++k) {
        WarpTri t{};
        for (int e = 0; e < 4; ++e) t.g[e] = get<double>(in);
        for (int e = 0; e < 2; ++e) t.qa[e] = get<double>(in);
        t.D = get<double>(in);
        float p[3][2], m[6];
        for (int v = 0; v < 3; ++v)
            for (int e = 0; e < 2; ++e) p[v][e] = get<float>(in);
        const int folded = warp_fit_triangle(t, p[0], p[1], p[2], m) ? 1 : 0;
        out.write((const char*)m, sizeof(m));
        out.write((const char*)&folded, sizeof(int));
    }
    const int n = get<int>(in);
    AlignTensorDev w14{}, w15{};
    align_gray_weights(14, w14);
    align_gray_weights(15, w15);
    bool same = true;
    for (int k = 0; k < n; ++k) {
        AlignRow r{};
        r.format = get<int>(in); r.w = get<int>(in); r.h = get<int>(in); r.stride = get<int>(in); r.cstride = get<int>(in);
        const int ow = get<int>(in), oh = get<int>(in), T = get<int>(in);
        std::vector<float> mats((size_t)T * 6);
        in.read((char*)mats.data(), (std::streamsize)(mats.size() * sizeof(float)));
        std::unique_ptr<uint8_t[]> lab(new uint8_t[(size_t)ow * oh]);           // (exactly the map's bytes)
        in.read((char*)lab.get(), (std::streamsize)ow * oh);
        float scale[3], bias[3];
        for (int e = 0; e < 3; ++e) scale[e] = get<float>(in);
        for (int e = 0; e < 3; ++e) bias[e] = get<float>(in);
        int b0, b1;
        const std::unique_ptr<uint8_t[]> p0 = block(in, b0), p1 = block(in, b1);
        r.p0 = p0.get(); r.p1 = b1 > 0 ? p1.get() : nullptr;
        AlignRow luma = r;                                   // one output channel: an NV12 row is its Y plane
        if (luma.format == SDM_FRAME_NV12) luma.format = SDM_FRAME_GRAY;
        const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
        std::vector<uint8_t> bgr((size_t)oh * ow * 3), g14((size_t)oh * ow), g15((size_t)oh * ow);
        std::vector<float> planes((size_t)3 * oh * ow);
        for (int i = 0; i < oh; ++i)
            for (int j0 = 0; j0 < ow; j0 += 4) {
                const int npx = ow - j0 < 4 ? ow - j0 : 4;
                float sx[4], sy[4];
                bool on[4];
                for (int q = 0; q < 4; ++q) {
                    const int l = q < npx ? lab[(size_t)i * ow + j0 + q] : SDM_WARP_NO_TRIANGLE;
                    on[q] = l != SDM_WARP_NO_TRIANGLE;
                    sx[q] = sy[q] = 0.0f;
                    if (on[q]) {
                        if (l >= T) { std::fprintf(stderr, "label %d beyond the %d triangles\n", l, T); return 2; }
                        warp_position(&mats[(size_t)l * 6], j0 + q, i, sx[q], sy[q]);
                    }
                }
                uint32_t px[4][3], wide[4][3], one[4][3], one_wide[4][3];
                align_fetch_segment<false>(r, sx, sy, on, px);
                align_fetch_segment<true>(r, sx, sy, on, wide);
                align_fetch_segment<false>(luma, sx, sy, on, one);
                align_fetch_segment<true>(luma, sx, sy, on, one_wide);
                for (int q = 0; q < npx; ++q) {
                    const size_t at = (size_t)i * ow + j0 + q;
                    for (int c = 0; c < 3; ++c) {
                        same = same && px[q][c] == wide[q][c] && one[q][c] == one_wide[q][c];
                        bgr[at * 3 + c] = (uint8_t)px[q][c];
                        planes[(size_t)c * oh * ow + at] = align_element(align_channel<3>(px[q], c, weigh, SDM_ALIGN_ORDER_RGB, 0, 0, 0, 14), scale[c], bias[c]);
                    }
                    g14[at] = (uint8_t)align_channel<1>(one[q], 0, weigh, 0, w14.wb, w14.wg, w14.wr, w14.gray_shift);
                    g15[at] = (uint8_t)align_channel<1>(one[q], 0, weigh, 0, w15.wb, w15.wg, w15.wr, w15.gray_shift);
                }
            }
        out.write((const char*)bgr.data(), (std::streamsize)bgr.size());
        out.write((const char*)g14.data(), (std::streamsize)g14.size());
        out.write((const char*)g15.data(), (std::streamsize)g15.size());
        out.write((const char*)planes.data(), (std::streamsize)(planes.size() * sizeof(float)));
    }
    std::printf("%d fits, %d cases, 32-bit and 64-bit offsets %s\n", n_fits, n, same ? "agree" : "DIFFER");
    return same ? 0 : 1;
}
