// Host build of the arithmetic of the tracker's motion-compensated initialisation (superviseddescent_amd/csrc/sdm_track_motion_device.h),
// run by tests/test_track_motion_host.py under -fsanitize=address,undefined: every frame lives in a heap block of exactly
// (h - 1) * stride + w bytes, the column sums in one of exactly n k ints, the window in one of exactly its rows times its pitch, so a tap
// or a word that leaves its buffer is reported.  The work is done as the kernels of csrc/sdm_track_motion.hip do it -- 256 lanes, the
// pixel columns and the offsets strided over them -- with the lanes one after the other, in DESCENDING order, since the result must
// not depend on it.  No device, no HIP.
//   usage: track_motion_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 w, h, stride and the frame the chip is stored from (int32 bytes, the bytes); the same of
//               the frame that is searched; float32 x0, x1, y0, y1, scale; int32 S, min_gain.  Then int32 m and m x {best, zero, min_gain}.
//   out.bin     per case int32 k, ox, oy; the 32 x 32 chip; (2S + 1)^2 int32 SADs [dy + S][dx + S]; int32 best dx, dy (cells), best SAD,
//               SAD(0, 0), shift x, y (pixels).  Then m int32 of the acceptance rule.
#include "../../superviseddescent_amd/csrc/sdm_track_motion_device.h"

#include "host_case.hpp"

#include <cstring>
#include <vector>

static const int LANES = 256;

// n x n cells from (X0, Y0) into out (pitch bytes per row), the two phases of a cell row as the kernels run them
static void build_cells(const TrackMotionImage& im, int X0, int Y0, int k, int n, uint8_t* out, int pitch)
{
    std::unique_ptr<int[]> colsum(new int[(size_t)n * k]);
    for (int r = 0; r < n; ++r) {
        for (int lane = LANES - 1; lane >= 0; --lane) track_motion_columns(im, X0, Y0 + r * k, k, n * k, lane, LANES, colsum.get());
        for (int c = n - 1; c >= 0; --c) {
            int s = 0;
            for (int q = TRACK_MOTION_PARTS - 1; q >= 0; --q) s += track_motion_cell_part(colsum.get(), c, q, k);
            out[r * pitch + c] = track_motion_mean(s, k);
        }
    }
}

static TrackMotionImage frame(std::ifstream& in, std::unique_ptr<uint8_t[]>& hold)
{
    TrackMotionImage im;
    im.w = get<int>(in); im.h = get<int>(in); im.stride = get<int>(in);
    int bytes = 0;
    hold = block(in, bytes);
    if (bytes != (im.h - 1) * im.stride + im.w) { std::fprintf(stderr, "a frame block of the wrong size\n"); std::exit(2); }
    im.p = hold.get();
    return im;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: track_motion_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](int v) { out.write((const char*)&v, 4); };
    const int n_cases = get<int>(in);
    for (int t = 0; t < n_cases; ++t) {
        std::unique_ptr<uint8_t[]> hold_a, hold_b;
        const TrackMotionImage a = frame(in, hold_a), b = frame(in, hold_b);
        const float x0 = get<float>(in), x1 = get<float>(in), y0 = get<float>(in), y1 = get<float>(in), scale = get<float>(in);
        const int S = get<int>(in), min_gain = get<int>(in);
        const TrackMotionGrid g = track_motion_grid(x0, x1, y0, y1, scale);
        put(g.k); put(g.ox); put(g.oy);
        std::unique_ptr<uint32_t[]> chip(new uint32_t[TRACK_MOTION_C * TRACK_MOTION_C / 4]);
        build_cells(a, g.ox, g.oy, g.k, TRACK_MOTION_C, (uint8_t*)chip.get(), TRACK_MOTION_C);
        out.write((const char*)chip.get(), TRACK_MOTION_C * TRACK_MOTION_C);
        const int W = track_motion_window(S), pitch = track_motion_pitch(S);
        std::unique_ptr<uint32_t[]> cur(new uint32_t[(size_t)W * pitch / 4]);
        std::memset(cur.get(), 0, (size_t)W * pitch);
        build_cells(b, g.ox - S * g.k, g.oy - S * g.k, g.k, W, (uint8_t*)cur.get(), pitch);
        for (int dy = -S; dy <= S; ++dy)
            for (int dx = -S; dx <= S; ++dx) put(track_motion_sad(cur.get(), chip.get(), S, dx, dy));
        unsigned long long best = ~0ull;
        int zero = -1;
        for (int lane = LANES - 1; lane >= 0; --lane) {
            const unsigned long long key = track_motion_search(cur.get(), chip.get(), S, lane, LANES, &zero);
            best = key < best ? key : best;
        }
        const int sad = track_motion_key_sad(best), dx = track_motion_key_dx(best), dy = track_motion_key_dy(best);
        const bool take = track_motion_accept(sad, zero, min_gain);
        put(dx); put(dy); put(sad); put(zero); put(take ? dx * g.k : 0); put(take ? dy * g.k : 0);
    }
    const int m = get<int>(in);
    for (int t = 0; t < m; ++t) {
        const int best = get<int>(in), zero = get<int>(in), gain = get<int>(in);
        put(track_motion_accept(best, zero, gain) ? 1 : 0);
    }
    std::printf("%d cases, %d acceptance triples\n", n_cases, m);
    return 0;
}
