// GPU test driver of rcr::paste_warped_tensor (superviseddescent_amd/include/rcr/warp.hpp; run by tests/test_cpp_warp_paste.py on the
// MI355X box): a float16 NCHW RGB tensor with mean / std and a per-row opacity map pasted into rcr::DeviceFrame s of several formats --
// once through the fit of landmark rows (the detection_model overload), once through those rows' mesh landmarks (the explicit
// overload), each into a fresh copy of the frames.
//   usage: warp_paste_gpu <dir>
//   <dir>/meta.txt      S crop_w crop_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another (`bytes` each)
//   <dir>/rows.f32      S x 2L landmark rows          <dir>/tmpl.f32    K x 2 template points (triangles: their Delaunay triangulation)
//   <dir>/tensor.f16    S x 3 x crop_h x crop_w       <dir>/alpha.u8    S x crop_h x crop_w
// writes fit.u8 and at.u8 (the frames' bytes after each paste), mats.f32, flags.i32, flags_at.i32
#include "rcr/warp.hpp"

#include "gpu_driver.hpp"

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "warp_paste_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt");
        const int S = sc.S, cw = sc.w, ch = sc.h, K = (int)sc.lm.size();
        const std::vector<int>& lm = sc.lm;
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        auto tm = read_all<float>(dir + "/tmpl.f32");
        auto tensor = read_all<uint8_t>(dir + "/tensor.f16");
        auto alpha = read_all<uint8_t>(dir + "/alpha.u8");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L || (int)tm.size() != 2 * K || tensor.size() != (size_t)S * 3 * cw * ch * 2 || alpha.size() != (size_t)S * cw * ch)
            throw std::runtime_error("scenario size mismatch");
        DeviceMemory mem;
        const uint8_t* in_dev = mem.upload(tensor.data(), tensor.size());
        const rcr::PasteMask mask{mem.upload(alpha.data(), alpha.size()), true};
        cv::Mat x(S, 2 * L, CV_32FC1), tmpl(K, 2, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        std::memcpy(tmpl.ptr<float>(0), tm.data(), tm.size() * 4);
        rcr::TensorSpec spec;                                                       // float16, NCHW, RGB
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
        for (int c = 0; c < 3; ++c) { spec.scale[c] = sd[c]; spec.bias[c] = mean[c]; }
        const rcr::WarpMesh mesh = rcr::WarpMesh::of_template(lm, tmpl, cw, ch);
        cv::Mat points(S, 2 * K, CV_32FC1);
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < K; ++k) {
                points.at<float>(s, 2 * k) = x.at<float>(s, lm[k]);
                points.at<float>(s, 2 * k + 1) = x.at<float>(s, L + lm[k]);
            }
        rcr::warp_paste_result fit;
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<rcr::DeviceFrame> frames;
            size_t at = 0;
            for (int s = 0; s < S; ++s) {
                uint8_t* p = mem.upload(pixels.data() + at, (size_t)sc.bytes[s], (size_t)(s % 4));     // misalignment 0 ... 3
                at += (size_t)sc.bytes[s];
                frames.push_back(rcr::DeviceFrame{p, sc.W[s], sc.H[s], sc.stride[s], sc.fmt[s]});
            }
            rcr::warp_paste_result res;
            if (pass == 0) res = fit = rcr::paste_warped_tensor(model, frames, x, {}, mesh, spec, in_dev, mask);
            else res = rcr::paste_warped_tensor(model, points, {}, mesh, spec, in_dev, frames, mask);
            std::vector<uint8_t> host(pixels.size());
            at = 0;
            for (int s = 0; s < S; ++s) {
                mem.download(host.data() + at, frames[s].data, (size_t)sc.bytes[s]);
                at += (size_t)sc.bytes[s];
            }
            write_bytes(dir + (pass == 0 ? "/fit.u8" : "/at.u8"), host.data(), host.size());
            write_bytes(dir + (pass == 0 ? "/flags.i32" : "/flags_at.i32"), res.flags.data(), (size_t)S * 4);
        }
        write_bytes(dir + "/mats.f32", fit.matrices.ptr<float>(0), (size_t)S * 6 * mesh.n_triangles() * 4);
        std::printf("%d rows of %d x %d pasted twice\n", S, cw, ch);
        return 0;
    });
}
