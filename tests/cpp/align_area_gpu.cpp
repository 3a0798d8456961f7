// GPU test driver of the rcr::aligned_crops_tensor overload that takes an rcr::AlignFilter (run by tests/test_cpp_align_area.py on the
// MI355X box): landmark rows of several scales on two ragged BGR rcr::DeviceFrame s and one NV12 frame, area-averaged, written as a float16
// NCHW RGB tensor with mean / std and -- capped at 2 sub-samples per axis -- as a u8 NHWC BGR tensor.
//   usage: align_area_gpu <dir>
//   <dir>/meta.txt      S out_w out_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another (`bytes` each: plane 0, and behind it the UV plane of an NV12 frame)
//   <dir>/rows.f32      S x 2L landmark rows;  <dir>/tmpl.f32  K x 2 template points
// writes f16.bin, u8.bin, mats.f32, flags.i32, samples.i32, samples_u8.i32
#include "rcr/alignment.hpp"

#include "gpu_driver.hpp"

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "align_area_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt");
        const int S = sc.S, ow = sc.w, oh = sc.h, K = (int)sc.lm.size();
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        auto tmpl = read_all<float>(dir + "/tmpl.f32");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L || (int)tmpl.size() != 2 * K) throw std::runtime_error("scenario size mismatch");
        DeviceMemory mem;
        std::vector<rcr::DeviceFrame> frames;
        size_t at = 0;
        for (int s = 0; s < S; ++s) {
            uint8_t* p = mem.upload(pixels.data() + at, (size_t)sc.bytes[s], (size_t)(s % 4));      // source misalignment 0 ... 3
            at += (size_t)sc.bytes[s];
            frames.push_back(rcr::DeviceFrame{p, sc.W[s], sc.H[s], sc.stride[s], sc.fmt[s]});
        }
        cv::Mat x(S, 2 * L, CV_32FC1), t(K, 2, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        std::memcpy(t.ptr<float>(0), tmpl.data(), tmpl.size() * 4);
        const size_t n = (size_t)S * 3 * ow * oh;
        void* out = mem.alloc(n * 2);

        rcr::TensorSpec f16;                                                        // float16, NCHW, RGB
        const double mean[3] = {123.675, 116.28, 103.53}, sd[3] = {58.395, 57.12, 57.375};
        f16.normalise(mean, sd);
        rcr::AlignFilter area;                                                      // area, up to 16 sub-samples per axis
        auto a = rcr::aligned_crops_tensor(model, frames, x, {}, sc.lm, t, ow, oh, f16, area, out);
        std::vector<uint8_t> host(n * 2);
        mem.download(host.data(), out, n * 2);
        write_bytes(dir + "/f16.bin", host.data(), n * 2);
        write_bytes(dir + "/mats.f32", a.matrices.ptr<float>(0), (size_t)S * 6 * 4);
        write_bytes(dir + "/flags.i32", a.flags.data(), (size_t)S * 4);
        write_bytes(dir + "/samples.i32", a.samples.data(), (size_t)S * 4);

        rcr::TensorSpec u8;
        u8.dtype = SDM_ALIGN_U8; u8.layout = SDM_ALIGN_NHWC; u8.order = SDM_ALIGN_ORDER_BGR;
        area.max_samples = 2;
        auto b = rcr::aligned_crops_tensor(model, frames, x, {}, sc.lm, t, ow, oh, u8, area, out);
        write_bytes(dir + "/samples_u8.i32", b.samples.data(), (size_t)S * 4);
        mem.download(host.data(), out, n);
        write_bytes(dir + "/u8.bin", host.data(), n);
        std::printf("%d rows, %d x %d crops written\n", S, ow, oh);
        return 0;
    });
}
