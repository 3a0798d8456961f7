// Conversion rate of sdm_set_frames_device's kernel (csrc/sdm_frames.hip) on 64 dense BGR frames of 1920 x 1080, beside the host
// upload's bgr2gray_kernel (csrc/sdm_apply.hip) on the same bytes and a device-to-device hipMemcpyAsync of the same bytes (read +
// write of the colour bytes: the memory ceiling).  Calls the library's launchers directly, times with events, alternates the three
// variants, three runs each, and checks that the two kernels wrote the same gray bytes.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I superviseddescent_amd/csrc scripts/ubench/frames_ingest.hip \
//         -L superviseddescent_amd/lib -lsdm_hip -Wl,-rpath,$PWD/superviseddescent_amd/lib -o frames_ingest
#include "sdm_kernels.h"

#include <cstdio>
#include <cstring>
#include <vector>

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main()
{
    const int n = 64, W = 1920, H = 1080, iters = 20, runs = 3;
    const size_t px = (size_t)n * W * H, in_bytes = px * 3;
    std::vector<uint8_t> host(in_bytes);
    unsigned long long s = 88172645463325252ull;
    for (size_t i = 0; i < in_bytes; i += 8) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; std::memcpy(&host[i], &s, 8); }
    uint8_t *src, *gray_new, *gray_old, *copy;
    FrameConvDev* desc;
    CK(hipMalloc(&src, in_bytes + 16)); CK(hipMalloc(&copy, in_bytes)); CK(hipMalloc(&gray_new, px)); CK(hipMalloc(&gray_old, px + 16));
    CK(hipMalloc(&desc, n * sizeof(FrameConvDev)));
    CK(hipMemcpy(src, host.data(), in_bytes, hipMemcpyHostToDevice));
    std::vector<FrameConvDev> d(n);
    unsigned blocks = 0;
    for (int i = 0; i < n; ++i) {
        d[i] = FrameConvDev{src + (size_t)i * W * H * 3, (long long)i * sdm_frames_gray_stride(W) * H, W, H, W * 3, sdm_frames_gray_stride(W), 3, 0, blocks, 0};
        blocks += (unsigned)sdm_frames_blocks(W, H);
    }
    CK(hipMemcpy(desc, d.data(), n * sizeof(FrameConvDev), hipMemcpyHostToDevice));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto run = [&](int v) {
        if (v == 0) sdm_launch_frames_to_gray(desc, n, blocks, gray_new, 14, st);
        else if (v == 1) sdm_launch_bgr2gray(src, gray_old, (long long)px, 14, st);
        else (void)hipMemcpyAsync(copy, src, in_bytes, hipMemcpyDeviceToDevice, st);
    };
    const char* names[3] = {"frames_to_gray_kernel (new)", "bgr2gray_kernel (host upload's)", "hipMemcpyAsync D2D, same colour bytes"};
    for (int v = 0; v < 3; ++v) { run(v); run(v); }      // warm-up
    CK(hipStreamSynchronize(st));
    float us[3][3];
    for (int r = 0; r < runs; ++r)
        for (int v = 0; v < 3; ++v) {
            CK(hipEventRecord(a, st));
            for (int i = 0; i < iters; ++i) run(v);
            CK(hipEventRecord(b, st));
            CK(hipEventSynchronize(b));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, a, b));
            us[v][r] = ms * 1000.0f / iters;
        }
    CK(hipGetLastError());
    std::vector<uint8_t> g0(px), g1(px);
    CK(hipMemcpy(g0.data(), gray_new, px, hipMemcpyDeviceToHost)); CK(hipMemcpy(g1.data(), gray_old, px, hipMemcpyDeviceToHost));
    std::printf("64 dense BGR frames 1920 x 1080: %.1f MB colour in, %.1f MB gray out; %d launches per run, %d runs, variants alternated\n",
                in_bytes / 1e6, px / 1e6, iters, runs);
    std::printf("gray bytes of the two kernels: %s\n", std::memcmp(g0.data(), g1.data(), px) == 0 ? "identical" : "DIFFERENT");
    for (int v = 0; v < 3; ++v) {
        float lo = us[v][0], hi = us[v][0], sum = 0;
        for (int r = 0; r < runs; ++r) { lo = us[v][r] < lo ? us[v][r] : lo; hi = us[v][r] > hi ? us[v][r] : hi; sum += us[v][r]; }
        const double mean = sum / runs, moved = v == 2 ? 2.0 * in_bytes : (double)in_bytes + px;      // bytes read + written
        std::printf("%-40s %8.1f us/launch (runs %.1f %.1f %.1f, spread %.1f %%)  %6.2f TB/s moved, %6.2f TB/s of colour bytes in\n", names[v], mean,
                    us[v][0], us[v][1], us[v][2], 100.0 * (hi - lo) / mean, moved / mean * 1e-6, in_bytes / mean * 1e-6);
    }
    return 0;
}
