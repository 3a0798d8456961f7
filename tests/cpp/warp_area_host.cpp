// Host build of the arithmetic of sdm_warp_crops_tensor_filtered (superviseddescent_amd/csrc/sdm_warp_area_device.h), run by
// tests/test_warp_area_host.py under -fsanitize=address,undefined: every plane lives in a heap block of exactly the bytes the frame owns
// (up to the last pixel of the last row), so a tap that leaves the frame is reported.  No device, no HIP.
//   usage: warp_area_host <cases.bin> <out.bin>
//   cases.bin   int32 n_rules, then per rule: float32 A[6]; int32 flags, mode, max_samples; float32 min_scale
//               int32 n, then per case: int32 format, w, h, stride, cstride, out_w, out_h, T; float32 matrices[T][6]; out_h x out_w label
//               bytes; float32 scale[3], bias[3]; int32 flags, mode, max_samples; float32 min_scale; int32 bytes0, bytes0 bytes of plane 0;
//               int32 bytes1, bytes1 bytes of the UV plane
//   out.bin     per rule: int32 Sx, Sy
//               per case: int32 samples[T][2]; out_h x out_w x 3 bytes (B, G, R), out_h x out_w bytes (1 channel, gray_shift 14),
//               out_h x out_w bytes (gray_shift 15), 3 x out_h x out_w float32 (RGB planes, v * scale + bias); uint32: the largest
//               sum + 512 n any pixel of a GRAY case reached before the division (0 for the other formats)
// A lane's work is a segment of 4 pixels, as in the kernel (WarpMeshArea, csrc/sdm_warp_area.hip): the labels, the counts of each pixel's
// triangle, the unfiltered path when every live pixel has Sx = Sy = 1, warp_area_segment otherwise.
// exits 1 when the 32-bit and the 64-bit offset paths disagree
#include "../../superviseddescent_amd/csrc/sdm_warp_area_device.h"

#include "host_case.hpp"

#include <vector>

template <bool WIDE>
static void segment(const AlignRow& r, const std::vector<WarpAreaRec>& rec, const uint8_t* labels, int ow, int i, int j0, int npx, uint32_t px[4][3])
{
    int lab[4];
    bool plain = true;
    for (int q = 0; q < 4; ++q) {
        const int l = q < npx ? labels[(size_t)i * ow + j0 + q] : SDM_WARP_NO_TRIANGLE;
        lab[q] = l == SDM_WARP_NO_TRIANGLE ? -1 : l;
        if (lab[q] >= 0) plain = plain && rec[(size_t)l].Sx == 1 && rec[(size_t)l].Sy == 1;
    }
    if (plain) {
        float sx[4], sy[4];
        bool on[4];
        for (int q = 0; q < 4; ++q) {
            on[q] = lab[q] >= 0;
            sx[q] = sy[q] = 0.0f;
            if (on[q]) warp_position(rec[(size_t)lab[q]].m, j0 + q, i, sx[q], sy[q]);
        }
        align_fetch_segment<WIDE>(r, sx, sy, on, px);
    } else {
        warp_area_segment<WIDE>(r, rec.data(), lab, i, j0, px);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: warp_area_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int n_rules = get<int>(in);
    for (int k = 0; k < n_rules; ++k) {
        float m[6];
        for (int e = 0; e < 6; ++e) m[e] = get<float>(in);
        const int flags = get<int>(in), mode = get<int>(in), max_samples = get<int>(in);
        const float min_scale = get<float>(in);
        int S[2];
        warp_area_samples(m, flags, mode, max_samples, min_scale * min_scale, S[0], S[1]);
        out.write((const char*)S, sizeof(S));
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
        const int flags = get<int>(in), mode = get<int>(in), max_samples = get<int>(in);
        const float min_scale = get<float>(in);
        int b0, b1;
        const std::unique_ptr<uint8_t[]> p0 = block(in, b0), p1 = block(in, b1);
        r.p0 = p0.get(); r.p1 = b1 > 0 ? p1.get() : nullptr;
        std::vector<int> smp((size_t)T * 2);
        std::vector<WarpAreaRec> rec((size_t)T);                 // (exactly T records: a label beyond them is reported)
        for (int t = 0; t < T; ++t) {
            for (int e = 0; e < 6; ++e) rec[(size_t)t].m[e] = mats[(size_t)t * 6 + e];
            warp_area_samples(rec[(size_t)t].m, flags, mode, max_samples, min_scale * min_scale, rec[(size_t)t].Sx, rec[(size_t)t].Sy);
            smp[(size_t)2 * t] = rec[(size_t)t].Sx; smp[(size_t)2 * t + 1] = rec[(size_t)t].Sy;
        }
        out.write((const char*)smp.data(), (std::streamsize)(smp.size() * sizeof(int)));
        AlignRow luma = r;                                   // one output channel: an NV12 row is its Y plane
        if (luma.format == SDM_FRAME_NV12) luma.format = SDM_FRAME_GRAY;
        const bool weigh = r.format >= SDM_FRAME_BGR && r.format <= SDM_FRAME_RGBA;
        std::vector<uint8_t> bgr((size_t)oh * ow * 3), g14((size_t)oh * ow), g15((size_t)oh * ow);
        std::vector<float> planes((size_t)3 * oh * ow);
        uint32_t top = 0u;
        for (int i = 0; i < oh; ++i)
            for (int j0 = 0; j0 < ow; j0 += 4) {
                const int npx = ow - j0 < 4 ? ow - j0 : 4;
                for (int q = 0; q < npx; ++q)
                    if (lab[(size_t)i * ow + j0 + q] != SDM_WARP_NO_TRIANGLE && lab[(size_t)i * ow + j0 + q] >= T) {
                        std::fprintf(stderr, "label %d beyond the %d triangles\n", lab[(size_t)i * ow + j0 + q], T);
                        return 2;
                    }
                uint32_t px[4][3], wide[4][3], one[4][3], one_wide[4][3];
                segment<false>(r, rec, lab.get(), ow, i, j0, npx, px);
                segment<true>(r, rec, lab.get(), ow, i, j0, npx, wide);
                segment<false>(luma, rec, lab.get(), ow, i, j0, npx, one);
                segment<true>(luma, rec, lab.get(), ow, i, j0, npx, one_wide);
                if (r.format == SDM_FRAME_GRAY) {            // the accumulator of every pixel, as warp_area_segment forms it
                    int l4[4];
                    for (int q = 0; q < 4; ++q) {
                        const int l = q < npx ? lab[(size_t)i * ow + j0 + q] : SDM_WARP_NO_TRIANGLE;
                        l4[q] = l == SDM_WARP_NO_TRIANGLE ? -1 : l;
                    }
                    uint32_t acc[4][3] = {}, cnt[4];
                    bool ok[4];
                    for (int q = 0; q < 4; ++q) ok[q] = l4[q] >= 0;
                    warp_area_sums<ALIGN_AREA_GRAY, false>(r, rec.data(), l4, i, j0, acc, cnt, ok);
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t s = acc[q][0] + 512u * cnt[q];
                        top = l4[q] >= 0 && s > top ? s : top;
                    }
                }
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
        out.write((const char*)&top, sizeof(top));
    }
    std::printf("%d rules, %d cases, 32-bit and 64-bit offsets %s\n", n_rules, n, same ? "agree" : "DIFFER");
    return same ? 0 : 1;
}
