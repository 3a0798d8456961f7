// Host build of the YUV colour description of the shared device headers (include/sdm.h, "YUV colour description and 10-bit surfaces";
// superviseddescent_amd/csrc/sdm_yuv_device.h and the P010 taps of sdm_align_tensor_device.h, sdm_align_area_device.h and
// sdm_warp_area_device.h), run by tests/test_yuv_host.py under -fsanitize=address,undefined.  No device, no HIP.
//   yuv_host decode8            the six 8-bit tables over the whole 256^3 cube of (Y, U, V) against the real value computed in double
//                               from Kr and Kb; value 5's row against align_nv12_to_bgr on the same cube
//   yuv_host decode10           the six 10-bit tables on 2^20 random triples and the 8 corner triples
//   yuv_host encode             the six encodes over the 256^3 cube of (R, G, B) against the real value; encode(decode(Y, U, V)) within
//                               +-1 wherever the decode did not clamp, over the 256^3 cube of (Y, U, V); value 5's row against
//                               paste_nv12_luma / paste_nv12_chroma over the cube
//   yuv_host dump <in> <out>    every table row on the triples of a file, for the bit-for-bit comparison with tests/yuv_ref.py
//   yuv_host taps <in> <out>    the rigid, area, warp and area-warp fetches of a P010 frame whose planes each live in a heap block of
//                               EXACTLY the bytes the frame owns (host_case.hpp), with 32-bit and with 64-bit offsets
// The bound 0.501: half a unit of the final rounding, plus at most three coefficient roundings of 2^-21 each times an operand below
// 2^10 -- under 10^-3.
#include "../../superviseddescent_amd/csrc/sdm_align_area_device.h"
#include "../../superviseddescent_amd/csrc/sdm_warp_area_device.h"
#include "../../superviseddescent_amd/csrc/sdm_paste_device.h"
#include "host_case.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

const double KR[3] = {0.299, 0.2126, 0.2627}, KB[3] = {0.114, 0.0722, 0.0593};
const double BOUND = 0.501;

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

double clamp255(double v) { return v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v); }

// the real (B, G, R) of (Y, U, V) at d bits
void real_decode(int m, int full, int d, int Y, int U, int V, double bgr[3])
{
    const double Kr = KR[m], Kb = KB[m], Kg = 1.0 - Kr - Kb, one = (double)(1 << (d - 8));
    const double ys = full ? 255.0 / (double)((1 << d) - 1) : 255.0 / (219.0 * one), cs = full ? ys : 255.0 / (224.0 * one);
    const int y0 = full ? 0 : 16 << (d - 8);
    const double y = (double)(Y > y0 ? Y - y0 : 0) * ys, u = (double)(U - (1 << (d - 1))), v = (double)(V - (1 << (d - 1)));
    bgr[2] = y + 2.0 * (1.0 - Kr) * cs * v;
    bgr[0] = y + 2.0 * (1.0 - Kb) * cs * u;
    bgr[1] = y - 2.0 * Kr * (1.0 - Kr) / Kg * cs * v - 2.0 * Kb * (1.0 - Kb) / Kg * cs * u;
}

// worst |integer - clamp255(real)| of a table on one triple; clamped: a real component left [0, 255] (or Y lay below y0)
double decode_error(const YuvDecode& t, int m, int full, int d, int Y, int U, int V, bool* clamped = nullptr)
{
    uint32_t got[3];
    double want[3], worst = 0.0;
    yuv_to_bgr(t, (uint32_t)Y, (uint32_t)U, (uint32_t)V, got);
    real_decode(m, full, d, Y, U, V, want);
    bool cl = Y < t.y0;
    for (int c = 0; c < 3; ++c) {
        cl = cl || want[c] < 0.0 || want[c] > 255.0;
        worst = std::fmax(worst, std::fabs((double)got[c] - clamp255(want[c])));
    }
    if (clamped) *clamped = cl;
    return worst;
}

int decode8()
{
    int bad = 0;
    for (int m = 0; m < 3; ++m)
        for (int full = 0; full < 2; ++full) {
            const YuvDecode& t = yuv_tables.dec[m * 2 + full];
            double worst = 0.0;
            for (int Y = 0; Y < 256; ++Y)
                for (int U = 0; U < 256; ++U)
                    for (int V = 0; V < 256; ++V) worst = std::fmax(worst, decode_error(t, m, full, 8, Y, U, V));
            std::printf("decode 8 bits, matrix %d, full %d: worst error %.6f\n", m, full, worst);
            bad += !(worst <= BOUND);
        }
    // BT.709 limited, the header's check values
    const YuvDecode& c = yuv_tables.dec[2];
    bad += !(c.cy == 1220945 && c.cvr == 1879825 && c.cub == 2215014 && c.cvg == 558796 && c.cug == 223607);
    // value 5: the bits it always had
    long long differ = 0;
    for (int Y = 0; Y < 256; ++Y)
        for (int U = 0; U < 256; ++U)
            for (int V = 0; V < 256; ++V) {
                uint32_t a[3], b[3];
                yuv_to_bgr(yuv_tables.dec[yuv_decode_row(SDM_FRAME_NV12)], (uint32_t)Y, (uint32_t)U, (uint32_t)V, a);
                align_nv12_to_bgr((uint32_t)Y, (uint32_t)U, (uint32_t)V, b);
                differ += a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
            }
    std::printf("value 5 against align_nv12_to_bgr: %lld triples differ\n", differ);
    return bad || differ;
}

int decode10()
{
    int bad = 0;
    Rng rng{77u};
    std::vector<int> triples;
    for (int k = 0; k < 8; ++k) { triples.push_back(k & 1 ? 1023 : 0); triples.push_back(k & 2 ? 1023 : 0); triples.push_back(k & 4 ? 1023 : 0); }
    for (int k = 0; k < (1 << 20); ++k)
        for (int c = 0; c < 3; ++c) triples.push_back((int)(rng.next() & 1023u));
    for (int m = 0; m < 3; ++m)
        for (int full = 0; full < 2; ++full) {
            const YuvDecode& t = yuv_tables.dec[6 + m * 2 + full];
            double worst = 0.0;
            for (size_t k = 0; k + 2 < triples.size(); k += 3)
                worst = std::fmax(worst, decode_error(t, m, full, 10, triples[k], triples[k + 1], triples[k + 2]));
            std::printf("decode 10 bits, matrix %d, full %d: worst error %.6f\n", m, full, worst);
            bad += !(worst <= BOUND);
        }
    const YuvDecode& c = yuv_tables.dec[6 + 2];
    bad += !(c.cy == 305236 && c.cvr == 469956 && c.cub == 553753 && c.cvg == 139699 && c.cug == 55902);
    return bad;
}

int encode()
{
    int bad = 0;
    for (int m = 0; m < 3; ++m)
        for (int full = 0; full < 2; ++full) {
            const YuvEncode& e = yuv_tables.enc[m * 2 + full];
            const double Kr = KR[m], Kb = KB[m], Kg = 1.0 - Kr - Kb, sy = full ? 1.0 : 219.0 / 255.0, sc = full ? 1.0 : 224.0 / 255.0;
            double worst = 0.0;
            for (int R = 0; R < 256; ++R)
                for (int G = 0; G < 256; ++G)
                    for (int B = 0; B < 256; ++B) {
                        const uint32_t bgr[3] = {(uint32_t)B, (uint32_t)G, (uint32_t)R};
                        uint32_t u, v;
                        const uint32_t y = yuv_luma(e, bgr);
                        yuv_chroma(e, bgr, u, v);
                        const double ry = (Kr * R + Kg * G + Kb * B) * sy + (full ? 0.0 : 16.0);
                        const double ru = (0.5 * B - 0.5 * Kg / (1.0 - Kb) * G - 0.5 * Kr / (1.0 - Kb) * R) * sc + 128.0;
                        const double rv = (0.5 * R - 0.5 * Kg / (1.0 - Kr) * G - 0.5 * Kb / (1.0 - Kr) * B) * sc + 128.0;
                        worst = std::fmax(worst, std::fabs((double)y - ry));
                        worst = std::fmax(worst, std::fabs((double)u - clamp255(ru)));
                        worst = std::fmax(worst, std::fabs((double)v - clamp255(rv)));
                    }
            // the round trip over every (Y, U, V) whose decode did not clamp
            const YuvDecode& t = yuv_tables.dec[m * 2 + full];
            int trip = 0;
            long long kept = 0;
            for (int Y = 0; Y < 256; ++Y)
                for (int U = 0; U < 256; ++U)
                    for (int V = 0; V < 256; ++V) {
                        bool clamped;
                        decode_error(t, m, full, 8, Y, U, V, &clamped);
                        if (clamped) continue;
                        ++kept;
                        uint32_t bgr[3], u, v;
                        yuv_to_bgr(t, (uint32_t)Y, (uint32_t)U, (uint32_t)V, bgr);
                        const int y = (int)yuv_luma(e, bgr);
                        yuv_chroma(e, bgr, u, v);
                        const int dy = std::abs(y - Y), du = std::abs((int)u - U), dv = std::abs((int)v - V);
                        trip = dy > trip ? dy : trip; trip = du > trip ? du : trip; trip = dv > trip ? dv : trip;
                    }
            std::printf("encode, matrix %d, full %d: worst error %.6f, round trip within %d on %lld triples\n", m, full, worst, trip, kept);
            bad += !(worst <= BOUND) || trip > 1 || kept == 0;
        }
    const YuvEncode& c = yuv_tables.enc[3];          // BT.709 full, the header's check values
    bad += !(c.yr == 222927 && c.yg == 749942 && c.yb == 75707 && c.ub == 524288 && c.ug == 404150 && c.ur == 120138 && c.vr == 524288 &&
             c.vg == 476214 && c.vb == 48074);
    // value 5's row is paste_nv12_luma / paste_nv12_chroma
    long long differ = 0;
    for (int R = 0; R < 256; ++R)
        for (int G = 0; G < 256; ++G)
            for (int B = 0; B < 256; ++B) {
                const uint32_t bgr[3] = {(uint32_t)B, (uint32_t)G, (uint32_t)R};
                uint32_t u0, v0, u1, v1;
                yuv_chroma(yuv_tables.enc[yuv_encode_row(SDM_FRAME_NV12)], bgr, u0, v0);
                paste_nv12_chroma(bgr, u1, v1);
                differ += u0 != u1 || v0 != v1 || yuv_luma(yuv_tables.enc[YUV_ENCODE_PLAIN], bgr) != paste_nv12_luma(bgr);
            }
    std::printf("value 5 against paste_nv12_luma / paste_nv12_chroma: %lld triples differ\n", differ);
    return bad || differ;
}

// in: int32 n, n x 3 uint16 (0 ... 1023).  out: per decode row (13) n x 3 bytes (B, G, R) of the triple (& 255 for an 8-bit row), then per
// encode row (7) n x 3 bytes (Y, U, V) of (B, G, R) = the triple & 255
int dump(const char* in, const char* out)
{
    std::ifstream f(in, std::ios::binary);
    const int n = get<int>(f);
    std::vector<uint16_t> tr((size_t)3 * n);
    f.read((char*)tr.data(), (std::streamsize)(tr.size() * 2));
    if (!f) return 2;
    std::vector<uint8_t> res;
    for (int row = 0; row < YUV_DECODE_ROWS; ++row) {
        const uint32_t mask = (row >= 6 && row < 12) ? 1023u : 255u;
        for (int k = 0; k < n; ++k) {
            uint32_t bgr[3];
            yuv_to_bgr(yuv_tables.dec[row], tr[3 * k] & mask, tr[3 * k + 1] & mask, tr[3 * k + 2] & mask, bgr);
            for (int c = 0; c < 3; ++c) res.push_back((uint8_t)bgr[c]);
        }
    }
    for (int row = 0; row < YUV_ENCODE_ROWS; ++row)
        for (int k = 0; k < n; ++k) {
            const uint32_t bgr[3] = {tr[3 * k] & 255u, tr[3 * k + 1] & 255u, tr[3 * k + 2] & 255u};
            uint32_t u, v;
            yuv_chroma(yuv_tables.enc[row], bgr, u, v);
            res.push_back((uint8_t)yuv_luma(yuv_tables.enc[row], bgr)); res.push_back((uint8_t)u); res.push_back((uint8_t)v);
        }
    std::ofstream o(out, std::ios::binary);
    o.write((const char*)res.data(), (std::streamsize)res.size());
    return o ? 0 : 2;
}

// in: format, w, h, stride, the Y block, the UV block, cw, ch, m[6], S, T, T x (m[6], Sx, Sy), the label map (ch x cw bytes, 255: none).
// out: per fetch (rigid, area, warp, area warp) ch x cw x 3 bytes of the colour fetch, then ch x cw bytes of the luma-only fetch
template <bool WIDE>
void taps_run(AlignRow r, int cw, int ch, int S, const std::vector<WarpAreaRec>& rec, const uint8_t* lab, std::vector<uint8_t>& res)
{
    for (int fetch = 0; fetch < 4; ++fetch)
        for (int luma = 0; luma < 2; ++luma) {
            AlignRow q = r;
            if (luma) q.format |= YUV_LUMA_ONLY;
            for (int i = 0; i < ch; ++i)
                for (int j0 = 0; j0 < cw; j0 += 4) {
                    const int npx = cw - j0 < 4 ? cw - j0 : 4;
                    uint32_t px[4][3];
                    int labs[4];
                    float sx[4], sy[4];
                    bool on[4];
                    for (int k = 0; k < 4; ++k) {
                        const int l = k < npx ? lab[i * cw + j0 + k] : 255;
                        labs[k] = l == 255 ? -1 : l;
                        on[k] = labs[k] >= 0;
                        sx[k] = sy[k] = 0.0f;
                        if (on[k]) warp_position(rec[(size_t)labs[k]].m, j0 + k, i, sx[k], sy[k]);
                    }
                    if (fetch == 0) align_segment<WIDE>(q, i, j0, npx, px);
                    else if (fetch == 1) align_area_segment<WIDE>(q, i, j0, npx, S, px);
                    else if (fetch == 2) align_fetch_segment<WIDE>(q, sx, sy, on, px);
                    else warp_area_segment<WIDE>(q, rec.data(), labs, i, j0, px);
                    for (int k = 0; k < npx; ++k)
                        for (int c = 0; c < (luma ? 1 : 3); ++c) res.push_back((uint8_t)px[k][c]);
                }
        }
}

int taps(const char* in, const char* out)
{
    std::ifstream f(in, std::ios::binary);
    AlignRow r{};
    r.format = get<int>(f); r.w = get<int>(f); r.h = get<int>(f); r.stride = r.cstride = get<int>(f);
    int yb, uvb, lb;
    const std::unique_ptr<uint8_t[]> y = block(f, yb), uv = block(f, uvb);
    // the blocks are exactly the bytes the frame owns
    if (yb != (r.h - 1) * r.stride + 2 * r.w || uvb != ((r.h + 1) / 2 - 1) * r.stride + 4 * ((r.w + 1) / 2)) return 2;
    r.p0 = y.get(); r.p1 = uv.get();
    const int cw = get<int>(f), ch = get<int>(f);
    for (int e = 0; e < 6; ++e) r.m[e] = get<float>(f);
    const int S = get<int>(f), T = get<int>(f);
    std::vector<WarpAreaRec> rec((size_t)T);
    for (auto& t : rec) {
        for (int e = 0; e < 6; ++e) t.m[e] = get<float>(f);
        t.Sx = get<int>(f); t.Sy = get<int>(f);
    }
    const std::unique_ptr<uint8_t[]> lab = block(f, lb);
    if (lb != cw * ch) return 2;
    std::vector<uint8_t> narrow, wide;
    taps_run<false>(r, cw, ch, S, rec, lab.get(), narrow);
    taps_run<true>(r, cw, ch, S, rec, lab.get(), wide);
    if (narrow != wide) { std::fprintf(stderr, "32-bit and 64-bit offsets differ\n"); return 1; }
    std::ofstream o(out, std::ios::binary);
    o.write((const char*)narrow.data(), (std::streamsize)narrow.size());
    return o ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "decode8") return decode8();
    if (mode == "decode10") return decode10();
    if (mode == "encode") return encode();
    if (mode == "dump" && argc == 4) return dump(argv[2], argv[3]);
    if (mode == "taps" && argc == 4) return taps(argv[2], argv[3]);
    std::fprintf(stderr, "usage: yuv_host decode8 | decode10 | encode | dump <in> <out> | taps <in> <out>\n");
    return 2;
}
