// Host build of the per-pixel arithmetic of sdm_align_crops_tensor (superviseddescent_amd/csrc/sdm_align_tensor_device.h), run by
// tests/test_align_tensor_host.py under -fsanitize=address,undefined: every plane lives in a heap block of exactly the bytes the
// frame owns (up to the last pixel of the last row), so a tap that leaves the frame is reported.  No device, no HIP.
//   usage: align_tensor_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 format, w, h, stride, cstride, out_w, out_h; float32 M[6]; float32 scale[3], bias[3];
//               int32 bytes0, bytes0 bytes of plane 0; int32 bytes1, bytes1 bytes of the UV plane
//   out.bin     per case: out_h x out_w x 3 bytes (B, G, R), out_h x out_w bytes (1 channel, gray_shift 14), out_h x out_w bytes
//               (gray_shift 15), 3 x out_h x out_w float32 (RGB planes, v * scale + bias)
// exits 1 when the 32-bit and the 64-bit offset paths disagree
#include "../../superviseddescent_amd/csrc/sdm_align_tensor_device.h"

#include "host_case.hpp"

#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: align_tensor_host <cases.bin> <out.bin>\n"); return 2; }
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
        int b0, b1;
        const std::unique_ptr<uint8_t[]> p0 = block(in, b0), p1 = block(in, b1);
        r.p0 = p0.get(); r.p1 = b1 > 0 ? p1.get() : nullptr;
        const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
        std::vector<uint8_t> bgr((size_t)oh * ow * 3), g14((size_t)oh * ow), g15((size_t)oh * ow);
        std::vector<float> planes((size_t)3 * oh * ow);
        for (int i = 0; i < oh; ++i)
            for (int j0 = 0; j0 < ow; j0 += 4) {
                const int npx = ow - j0 < 4 ? ow - j0 : 4;
                uint32_t px[4][3], wide[4][3];
                align_segment<false>(r, i, j0, npx, px);
                align_segment<true>(r, i, j0, npx, wide);
                for (int q = 0; q < npx; ++q) {
                    const size_t at = (size_t)i * ow + j0 + q;
                    for (int c = 0; c < 3; ++c) {
                        same = same && px[q][c] == wide[q][c];
                        bgr[at * 3 + c] = (uint8_t)px[q][c];
                        planes[(size_t)c * oh * ow + at] = align_element(align_channel<3>(px[q], c, weigh, SDM_ALIGN_ORDER_RGB, 0, 0, 0, 14), scale[c], bias[c]);
                    }
                    // (an NV12 source with one channel is read as GRAY by the kernel: Y as it is; here the converted B stands in)
                    g14[at] = (uint8_t)align_channel<1>(px[q], 0, weigh, 0, w14.wb, w14.wg, w14.wr, w14.gray_shift);
                    g15[at] = (uint8_t)align_channel<1>(px[q], 0, weigh, 0, w15.wb, w15.wg, w15.wr, w15.gray_shift);
                }
            }
        out.write((const char*)bgr.data(), (std::streamsize)bgr.size());
        out.write((const char*)g14.data(), (std::streamsize)g14.size());
        out.write((const char*)g15.data(), (std::streamsize)g15.size());
        out.write((const char*)planes.data(), (std::streamsize)(planes.size() * sizeof(float)));
    }
    std::printf("%d cases, 32-bit and 64-bit offsets %s\n", n, same ? "agree" : "DIFFER");
    return same ? 0 : 1;
}
