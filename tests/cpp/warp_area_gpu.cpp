// GPU test driver of the rcr::warped_crops_tensor overloads that take an rcr::AlignFilter (superviseddescent_amd/include/rcr/warp.hpp; run
// by tests/test_cpp_warp_area.py on the MI355X box): landmark rows on rcr::DeviceFrame s of several formats, warped piecewise-affinely
// onto the default mesh of the model's mean with area-averaged sampling, written as a float16 NCHW RGB tensor with mean / std (the
// default filter) and as a u8 NHWC BGR tensor (at most 3 sub-samples per axis, min_scale 2).
//   usage: warp_area_gpu <dir>
//   <dir>/meta.txt      S out_w out_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes uv_offset (-1: behind the Y plane)
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another (`bytes` each)
//   <dir>/rows.f32      S x 2L landmark rows
// writes f16.bin, u8.bin, mats.f32, flags.i32, labels.u8, samples.i32 (the float16 call's), samples_u8.i32
#include "rcr/warp.hpp"

#include "gpu_driver.hpp"

// the tracker form: the same detail call on the tracker's handle (instantiated here, run by the Python layer's tracker test)
static rcr::warped_tensor_result (*const tracker_form)(rcr::tracker&, const rcr::WarpMesh&, const rcr::TensorSpec&, const rcr::AlignFilter&, void*,
                                                       const std::vector<rcr::DeviceFrame>&, const std::vector<const void*>&) = &rcr::warped_crops_tensor;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "warp_area_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt", 1);                                    // tail: uv_offset
        const int S = sc.S, ow = sc.w, oh = sc.h;
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L) throw std::runtime_error("scenario size mismatch");
        if (!tracker_form) throw std::runtime_error("no tracker form");
        DeviceMemory mem;
        std::vector<rcr::DeviceFrame> frames;
        std::vector<const void*> chroma;
        size_t at = 0;
        for (int s = 0; s < S; ++s) {
            uint8_t* p = mem.upload(pixels.data() + at, (size_t)sc.bytes[s], (size_t)(s % 4));      // source misalignment 0 ... 3
            at += (size_t)sc.bytes[s];
            frames.push_back(rcr::DeviceFrame{p, sc.W[s], sc.H[s], sc.stride[s], sc.fmt[s]});
            const int uv = sc.tail[s][0];
            chroma.push_back(uv >= 0 ? p + uv : nullptr);
        }
        cv::Mat x(S, 2 * L, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        const size_t n = (size_t)S * 3 * ow * oh;
        void* out = mem.alloc(n * 2);

        const rcr::WarpMesh mesh = rcr::WarpMesh::of_mean(model.get_mean(), sc.lm, ow, oh);
        const int T = mesh.n_triangles();
        rcr::TensorSpec f16;                                                        // float16, NCHW, RGB
        const double mean[3] = {123.675, 116.28, 103.53}, sd[3] = {58.395, 57.12, 57.375};
        f16.normalise(mean, sd);
        auto a = rcr::warped_crops_tensor(model, frames, x, {}, mesh, f16, rcr::AlignFilter(), out, chroma);
        if (a.samples.size() != (size_t)S * T * 2) throw std::runtime_error("samples: rows x T x 2 expected");
        std::vector<uint8_t> host(n * 2);
        mem.download(host.data(), out, n * 2);
        write_bytes(dir + "/f16.bin", host.data(), n * 2);
        write_bytes(dir + "/mats.f32", a.matrices.ptr<float>(0), (size_t)S * T * 6 * 4);
        write_bytes(dir + "/flags.i32", a.flags.data(), (size_t)S * 4);
        write_bytes(dir + "/labels.u8", a.labels.ptr<uint8_t>(0), (size_t)ow * oh);
        write_bytes(dir + "/samples.i32", a.samples.data(), a.samples.size() * 4);

        rcr::TensorSpec u8;
        u8.dtype = SDM_ALIGN_U8; u8.layout = SDM_ALIGN_NHWC; u8.order = SDM_ALIGN_ORDER_BGR;
        rcr::AlignFilter capped;
        capped.max_samples = 3; capped.min_scale = 2.0f;
        auto b = rcr::warped_crops_tensor(model, frames, x, {}, mesh, u8, capped, out, chroma);
        mem.download(host.data(), out, n);
        write_bytes(dir + "/u8.bin", host.data(), n);
        write_bytes(dir + "/samples_u8.i32", b.samples.data(), b.samples.size() * 4);
        // the unfiltered overload reports no samples
        if (!rcr::warped_crops_tensor(model, frames, x, {}, mesh, u8, out, chroma).samples.empty()) throw std::runtime_error("samples of an unfiltered call");
        std::printf("%d rows, %d triangles, %d x %d crops written\n", S, T, ow, oh);
        return 0;
    });
}
