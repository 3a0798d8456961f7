// GPU test driver of rcr::warped_crops_tensor (superviseddescent_amd/include/rcr/warp.hpp; run by tests/test_cpp_warp.py on the MI355X
// box): landmark rows on rcr::DeviceFrame s of several formats, warped piecewise-affinely onto the default mesh of the model's mean
// (rcr::WarpMesh::of_mean: alignment_template + Delaunay) and written as a float16 NCHW RGB tensor with mean / std and as a u8 NHWC BGR tensor.
//   usage: warp_gpu <dir>
//   <dir>/meta.txt      S out_w out_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes uv_offset (-1: behind the Y plane)
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another (`bytes` each)
//   <dir>/rows.f32      S x 2L landmark rows
// writes f16.bin, u8.bin, mats.f32, flags.i32, labels.u8, tmpl.f32, tri.i32
#include "rcr/warp.hpp"

#include <cstdio>
#include <dlfcn.h>
#include <fstream>

// the runtime calls the driver needs, taken from the HIP runtime that libsdm_hip.so has already brought into the process
struct Hip {
    int (*malloc_)(void**, size_t) = nullptr;
    int (*free_)(void*) = nullptr;
    int (*memcpy_)(void*, const void*, size_t, int) = nullptr;
    Hip()
    {
        malloc_ = (int (*)(void**, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
        free_ = (int (*)(void*))dlsym(RTLD_DEFAULT, "hipFree");
        memcpy_ = (int (*)(void*, const void*, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
        if (!malloc_ || !free_ || !memcpy_) throw std::runtime_error("the HIP runtime is not loaded");
    }
};

template <class T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const size_t n = (size_t)f.tellg();
    f.seekg(0);
    std::vector<T> v(n / sizeof(T));
    f.read((char*)v.data(), (std::streamsize)n);
    return v;
}

static void write_bytes(const std::string& path, const void* p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)p, (std::streamsize)n);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: warp_gpu <dir>\n"); return 2; }
    const std::string dir = argv[1];
    try {
        std::ifstream meta(dir + "/meta.txt");
        int S, ow, oh, K;
        meta >> S >> ow >> oh >> K;
        std::vector<int> lm(K);
        for (int& v : lm) meta >> v;
        std::vector<int> fmt(S), W(S), H(S), stride(S), bytes(S), uv(S);
        for (int s = 0; s < S; ++s) meta >> fmt[s] >> W[s] >> H[s] >> stride[s] >> bytes[s] >> uv[s];
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L) throw std::runtime_error("scenario size mismatch");
        superviseddescent::hip::Handle first(superviseddescent::hip::device());     // (the device is up from here on)
        Hip hip;
        std::vector<rcr::DeviceFrame> frames;
        std::vector<const void*> chroma;
        std::vector<void*> allocations;
        size_t at = 0;
        for (int s = 0; s < S; ++s) {
            void* d = nullptr;
            if (hip.malloc_(&d, (size_t)bytes[s] + 3) != 0) throw std::runtime_error("hipMalloc failed");
            allocations.push_back(d);
            uint8_t* p = (uint8_t*)d + s % 4;                                       // source misalignment 0 ... 3
            if (hip.memcpy_(p, pixels.data() + at, (size_t)bytes[s], 1 /* host to device */) != 0) throw std::runtime_error("hipMemcpy failed");
            at += (size_t)bytes[s];
            frames.push_back(rcr::DeviceFrame{p, W[s], H[s], stride[s], fmt[s]});
            chroma.push_back(uv[s] >= 0 ? p + uv[s] : nullptr);
        }
        cv::Mat x(S, 2 * L, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        const size_t n = (size_t)S * 3 * ow * oh;
        void* out = nullptr;
        if (hip.malloc_(&out, n * 2) != 0) throw std::runtime_error("hipMalloc failed");
        allocations.push_back(out);

        const rcr::WarpMesh mesh = rcr::WarpMesh::of_mean(model.get_mean(), lm, ow, oh);
        const int T = mesh.n_triangles();
        write_bytes(dir + "/tmpl.f32", mesh.tmpl.ptr<float>(0), (size_t)K * 2 * 4);
        write_bytes(dir + "/tri.i32", mesh.triangles.data(), (size_t)T * 3 * 4);
        rcr::TensorSpec f16;                                                        // float16, NCHW, RGB
        const double mean[3] = {123.675, 116.28, 103.53}, sd[3] = {58.395, 57.12, 57.375};
        f16.normalise(mean, sd);
        auto a = rcr::warped_crops_tensor(model, frames, x, {}, mesh, f16, out, chroma);
        std::vector<uint8_t> host(n * 2);
        if (hip.memcpy_(host.data(), out, n * 2, 2 /* device to host */) != 0) throw std::runtime_error("hipMemcpy failed");
        write_bytes(dir + "/f16.bin", host.data(), n * 2);
        write_bytes(dir + "/mats.f32", a.matrices.ptr<float>(0), (size_t)S * T * 6 * 4);
        write_bytes(dir + "/flags.i32", a.flags.data(), (size_t)S * 4);
        write_bytes(dir + "/labels.u8", a.labels.ptr<uint8_t>(0), (size_t)ow * oh);

        rcr::TensorSpec u8;
        u8.dtype = SDM_ALIGN_U8; u8.layout = SDM_ALIGN_NHWC; u8.order = SDM_ALIGN_ORDER_BGR;
        rcr::warped_crops_tensor(model, frames, x, {}, mesh, u8, out, chroma);
        if (hip.memcpy_(host.data(), out, n, 2) != 0) throw std::runtime_error("hipMemcpy failed");
        write_bytes(dir + "/u8.bin", host.data(), n);
        for (void* d : allocations) hip.free_(d);
        std::printf("%d rows, %d triangles, %d x %d crops written\n", S, T, ow, oh);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
