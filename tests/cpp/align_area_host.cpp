// Host build of the per-pixel arithmetic of sdm_align_crops_tensor_filtered (superviseddescent_amd/csrc/sdm_align_area_device.h), run by
// tests/test_align_area_host.py under -fsanitize=address,undefined: every plane lives in a heap block of exactly the bytes the frame
// owns (up to the last pixel of the last row), so a sub-sample's tap that leaves the frame is reported.  No device, no HIP.
//   usage: align_area_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 format, w, h, stride, cstride, out_w, out_h; float32 M[6]; float32 scale[3], bias[3];
//               int32 mode, max_samples; float32 min_scale; int32 bytes0, bytes0 bytes of plane 0; int32 bytes1, bytes1 bytes of the UV plane
//   out.bin     per case: int32 S, out_h x out_w x 3 bytes (B, G, R), out_h x out_w bytes (1 channel, gray_shift 14), out_h x out_w bytes
//               (gray_shift 15), 3 x out_h x out_w float32 (RGB planes, v * scale + bias)
// S == 1 runs align_segment, S > 1 align_area_segment, as the kernel does; so does the switch of a one-channel NV12 row to its Y plane.
// exits 1 when the 32-bit and the 64-bit offset paths disagree, or the reciprocal division is not the division
#include "../../superviseddescent_amd/csrc/sdm_align_area_device.h"

#include "host_case.hpp"

#include <vector>

template <bool WIDE>
static void segment(const AlignRow& r, int i, int j0, int npx, int S, uint32_t px[4][3])
{
    if (S == 1) align_segment<WIDE>(r, i, j0, npx, px);
    else align_area_segment<WIDE>(r, i, j0, npx, S, px);
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: align_area_host <cases.bin> <out.bin>\n"); return 2; }
    // every shifted sum the average can meet, for every S > 1
    for (uint32_t S = 2; S <= ALIGN_AREA_MAX_S; ++S) {
        const uint32_t n = S * S, rcp = align_area_reciprocal(n);
        for (uint32_t x = 0; x <= (255u * 1024u * n + 512u * n) >> 10; ++x)
            if (align_area_divide(x, rcp) != x / n) { std::printf("reciprocal division fails at %u / %u\n", x, n); return 1; }
    }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n = get<int>(in);
    AlignTensorDev w14{}, w15{};
    align_gray_weights(14, w14);
    align_gray_weights(15, w15);
    bool same = true;
    for (int k = 0; k < n; ++k) {
        AlignRow r;
        r.format = get<int>(in); r.w = get<int>(in); r.h = get<int>(in); r.stride = get<int>(in); r.cstride = get<int>(in);
        const int ow = get<int>(in), oh = get<int>(in);
        for (int e = 0; e < 6; ++e) r.m[e] = get<float>(in);
        float scale[3], bias[3];
        for (int e = 0; e < 3; ++e) scale[e] = get<float>(in);
        for (int e = 0; e < 3; ++e) bias[e] = get<float>(in);
        const int mode = get<int>(in), max_samples = get<int>(in);
        const float min_scale = get<float>(in);
        int b0, b1;
        const std::unique_ptr<uint8_t[]> p0 = block(in, b0), p1 = block(in, b1);
        r.p0 = p0.get(); r.p1 = b1 > 0 ? p1.get() : nullptr;
        const int S = align_area_samples(r.m, 0, mode, max_samples, min_scale * min_scale);
        AlignRow luma = r;                                   // one output channel: an NV12 row is its Y plane
        if (luma.format == SDM_FRAME_NV12) luma.format = SDM_FRAME_GRAY;
        const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
        std::vector<uint8_t> bgr((size_t)oh * ow * 3), g14((size_t)oh * ow), g15((size_t)oh * ow);
        std::vector<float> planes((size_t)3 * oh * ow);
        for (int i = 0; i < oh; ++i)
            for (int j0 = 0; j0 < ow; j0 += 4) {
                const int npx = ow - j0 < 4 ? ow - j0 : 4;
                uint32_t px[4][3], wide[4][3], one[4][3], one_wide[4][3];
                segment<false>(r, i, j0, npx, S, px);
                segment<true>(r, i, j0, npx, S, wide);
                segment<false>(luma, i, j0, npx, S, one);
                segment<true>(luma, i, j0, npx, S, one_wide);
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
        out.write((const char*)&S, sizeof(int));
        out.write((const char*)bgr.data(), (std::streamsize)bgr.size());
        out.write((const char*)g14.data(), (std::streamsize)g14.size());
        out.write((const char*)g15.data(), (std::streamsize)g15.size());
        out.write((const char*)planes.data(), (std::streamsize)(planes.size() * sizeof(float)));
    }
    std::printf("%d cases, 32-bit and 64-bit offsets %s\n", n, same ? "agree" : "DIFFER");
    return same ? 0 : 1;
}
