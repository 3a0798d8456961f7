// Host build of the arithmetic of the tracker's temporal landmark filter (superviseddescent_amd/csrc/sdm_track_filter_device.h), run by
// tests/test_track_filter_host.py under -fsanitize=address,undefined: every slot's r, d and f row and every row of a step live in a
// heap block of exactly 2L floats, so a load or store that leaves a row is reported.  A row is worked on as track_filter_kernel does
// it -- 64 lanes with the coordinates strided over them, the lanes' bounds reduced, then every lane's share of the row -- with the
// lanes one after the other, in DESCENDING order, since the result must not depend on it.  No device, no HIP.
//   usage: track_filter_host <cases.bin> <out.bin>
//   cases.bin   int32 n, then per case: int32 L, S, n_ops; float32 min_cutoff, beta, d_cutoff; per op: int32 kind (0 step, 1 un-prime), n,
//               n int32 ids; a step goes on with n int32 masks, n float32 dt, n x 2L float32 x
//   out.bin     per step n x 2L float32 out; per case, at its end: S x 2L r, S x 2L d, S x 2L f (float32), S int32 primed
#include "../../superviseddescent_amd/csrc/sdm_track_filter_device.h"

#include "host_case.hpp"

#include <algorithm>
#include <vector>

using Row = std::unique_ptr<float[]>;

static std::vector<Row> rows(int n, int M)
{
    std::vector<Row> v((size_t)n);
    for (Row& r : v) { r.reset(new float[M]); std::fill(r.get(), r.get() + M, 0.0f); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: track_filter_host <cases.bin> <out.bin>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int lanes = 64;
    const int n_cases = get<int>(in);
    int steps = 0;
    for (int k = 0; k < n_cases; ++k) {
        const int L = get<int>(in), S = get<int>(in), n_ops = get<int>(in), M = 2 * L;
        TrackFilterParams p{};
        p.min_cutoff = get<float>(in); p.beta = get<float>(in); p.d_cutoff = get<float>(in);
        std::vector<Row> r = rows(S, M), d = rows(S, M), f = rows(S, M);
        std::vector<int> primed((size_t)S, 0);
        for (int o = 0; o < n_ops; ++o) {
            const int kind = get<int>(in), n = get<int>(in);
            std::vector<int> ids((size_t)n), masks((size_t)n);
            for (int& v : ids) v = get<int>(in);
            if (kind == 1) {
                for (int id : ids) primed[id] = 0;
                continue;
            }
            for (int& v : masks) v = get<int>(in);
            std::vector<float> dt((size_t)n);
            for (float& v : dt) v = get<float>(in);
            std::vector<Row> x = rows(n, M);
            for (Row& row : x)
                for (int j = 0; j < M; ++j) row[j] = get<float>(in);
            for (int i = n - 1; i >= 0; --i) {
                const int id = ids[i];
                const int action = track_filter_action(masks[i], primed[id]);
                float w = 0.0f;
                if (action == TRACK_FILTER_RUN) {
                    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
                    for (int lane = lanes - 1; lane >= 0; --lane) {
                        float a, b, c, e;
                        track_filter_bounds(x[i].get(), L, lane, lanes, a, b, c, e);
                        x0 = fminf(x0, a); x1 = fmaxf(x1, b); y0 = fminf(y0, c); y1 = fmaxf(y1, e);
                    }
                    w = track_filter_weight(p.beta, x0, x1, y0, y1);
                }
                for (int lane = lanes - 1; lane >= 0; --lane)
                    track_filter_row(x[i].get(), r[id].get(), d[id].get(), f[id].get(), M, lane, lanes, action, dt[i], w, p);
                primed[id] = action != TRACK_FILTER_PASS;
            }
            for (const Row& row : x) out.write((const char*)row.get(), (std::streamsize)M * 4);
            ++steps;
        }
        for (const std::vector<Row>* st : {&r, &d, &f})
            for (const Row& row : *st) out.write((const char*)row.get(), (std::streamsize)M * 4);
        out.write((const char*)primed.data(), (std::streamsize)S * 4);
    }
    std::printf("%d cases, %d steps\n", n_cases, steps);
    return 0;
}
