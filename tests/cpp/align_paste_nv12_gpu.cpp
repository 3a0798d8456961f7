// GPU test driver of the rcr::paste_crops_tensor overloads that take the frames' UV planes (superviseddescent_amd/include/rcr/alignment.hpp;
// run by tests/test_cpp_align_paste_nv12.py on the MI355X box): a float16 NCHW RGB tensor with mean / std and a per-row opacity map pasted
// into rcr::DeviceFrame s of format NV12 -- the UV plane directly behind Y (chroma nullptr) or in an allocation of its own -- and BGR, each
// pass into a fresh copy of the frames: through the fit of landmark rows with area-averaged sampling (the detection_model overload),
// through the matrices that call returned (the explicit overload, filtered), and through them plain bilinear.
//   usage: align_paste_nv12_gpu <dir>
//   <dir>/meta.txt      S crop_w crop_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes_plane0 bytes_uv separate
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another: plane 0, then the UV plane
//   <dir>/rows.f32      S x 2L landmark rows          <dir>/tmpl.f32    K x 2 template points
//   <dir>/tensor.f16    S x 3 x crop_h x crop_w       <dir>/alpha.u8    S x crop_h x crop_w
// writes fit.u8, at.u8 and plain.u8 (the frames' bytes after each paste), mats.f32, flags.i32, flags_at.i32, samples.i32, samples_at.i32
#include "rcr/alignment.hpp"

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
    if (argc < 2) { std::fprintf(stderr, "usage: align_paste_nv12_gpu <dir>\n"); return 2; }
    const std::string dir = argv[1];
    try {
        std::ifstream meta(dir + "/meta.txt");
        int S, cw, ch, K;
        meta >> S >> cw >> ch >> K;
        std::vector<int> lm(K);
        for (int& v : lm) meta >> v;
        std::vector<int> fmt(S), W(S), H(S), stride(S), bytes(S), uv_bytes(S), separate(S);
        for (int s = 0; s < S; ++s) meta >> fmt[s] >> W[s] >> H[s] >> stride[s] >> bytes[s] >> uv_bytes[s] >> separate[s];
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        auto tm = read_all<float>(dir + "/tmpl.f32");
        auto tensor = read_all<uint8_t>(dir + "/tensor.f16");
        auto alpha = read_all<uint8_t>(dir + "/alpha.u8");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L || (int)tm.size() != 2 * K || tensor.size() != (size_t)S * 3 * cw * ch * 2 || alpha.size() != (size_t)S * cw * ch)
            throw std::runtime_error("scenario size mismatch");
        superviseddescent::hip::Handle first(superviseddescent::hip::device());     // (the device is up from here on)
        Hip hip;
        std::vector<void*> allocations;
        auto upload = [&](const void* src, size_t n, size_t shift) {
            void* d = nullptr;
            if (hip.malloc_(&d, n + shift) != 0) throw std::runtime_error("hipMalloc failed");
            allocations.push_back(d);
            if (hip.memcpy_((uint8_t*)d + shift, src, n, 1 /* host to device */) != 0) throw std::runtime_error("hipMemcpy failed");
            return (uint8_t*)d + shift;
        };
        const uint8_t* in_dev = upload(tensor.data(), tensor.size(), 0);
        const rcr::PasteMask mask{upload(alpha.data(), alpha.size(), 0), true};
        cv::Mat x(S, 2 * L, CV_32FC1), tmpl(K, 2, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        std::memcpy(tmpl.ptr<float>(0), tm.data(), tm.size() * 4);
        rcr::TensorSpec spec;                                                       // float16, NCHW, RGB
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
        for (int c = 0; c < 3; ++c) { spec.scale[c] = sd[c]; spec.bias[c] = mean[c]; }
        const rcr::AlignFilter filter;                                              // area, up to 16 x 16 sub-samples, every minifying row
        rcr::paste_result fit;
        const char* names[3] = {"/fit.u8", "/at.u8", "/plain.u8"};
        for (int pass = 0; pass < 3; ++pass) {
            std::vector<rcr::DeviceFrame> frames;
            std::vector<void*> chroma;
            size_t at = 0;
            for (int s = 0; s < S; ++s) {
                // planes that lie together: one allocation, misaligned by 0 ... 3; a separate UV plane: its own, misaligned by 1 ... 4 mod 4
                uint8_t* p = upload(pixels.data() + at, (size_t)bytes[s] + (separate[s] ? 0 : (size_t)uv_bytes[s]), (size_t)(s % 4));
                uint8_t* uv = separate[s] ? upload(pixels.data() + at + bytes[s], (size_t)uv_bytes[s], (size_t)((s + 1) % 4)) : nullptr;
                at += (size_t)bytes[s] + (size_t)uv_bytes[s];
                frames.push_back(rcr::DeviceFrame{p, W[s], H[s], stride[s], fmt[s]});
                chroma.push_back(uv);
            }
            rcr::paste_result res;
            if (pass == 0) res = fit = rcr::paste_crops_tensor(model, frames, chroma, x, {}, lm, tmpl, cw, ch, spec, filter, in_dev, mask);
            else if (pass == 1) res = rcr::paste_crops_tensor(fit.matrices, {}, cw, ch, spec, filter, in_dev, frames, chroma, mask);
            else res = rcr::paste_crops_tensor(fit.matrices, {}, cw, ch, spec, in_dev, frames, chroma, mask);
            std::vector<uint8_t> host(pixels.size());
            at = 0;
            for (int s = 0; s < S; ++s) {
                const size_t n0 = (size_t)bytes[s] + (separate[s] ? 0 : (size_t)uv_bytes[s]);
                if (hip.memcpy_(host.data() + at, frames[s].data, n0, 2 /* device to host */) != 0) throw std::runtime_error("hipMemcpy failed");
                if (separate[s] && hip.memcpy_(host.data() + at + n0, chroma[s], (size_t)uv_bytes[s], 2) != 0) throw std::runtime_error("hipMemcpy failed");
                at += (size_t)bytes[s] + (size_t)uv_bytes[s];
            }
            write_bytes(dir + names[pass], host.data(), host.size());
            if (pass == 2) {
                if (!res.samples.empty()) throw std::runtime_error("samples without a filter");
                continue;
            }
            write_bytes(dir + (pass == 0 ? "/flags.i32" : "/flags_at.i32"), res.flags.data(), (size_t)S * 4);
            if ((int)res.samples.size() != S) throw std::runtime_error("no samples came back");
            write_bytes(dir + (pass == 0 ? "/samples.i32" : "/samples_at.i32"), res.samples.data(), (size_t)S * 4);
        }
        write_bytes(dir + "/mats.f32", fit.matrices.ptr<float>(0), (size_t)S * 6 * 4);
        for (void* d : allocations) hip.free_(d);
        std::printf("%d rows of %d x %d pasted three times\n", S, cw, ch);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
