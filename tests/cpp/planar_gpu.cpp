// GPU test driver of rcr::DeviceFrame's second plane (superviseddescent_amd/include/rcr/adaptive_vlhog.hpp; include/sdm.h, "Planar colour
// frames"; run by tests/test_cpp_planar.py on the MI355X box): the same pixels as interleaved BGR frames and as planar frames --
// SDM_FRAME_BGR_PLANAR, every even frame with its planes a padded distance apart (second_plane set), every odd one a contiguous
// 3 x H x W block (second_plane left at its default) -- go through detection_model::detect_batch, one uint8 NHWC crop tensor of the
// detected rows and one paste of a float16 NCHW tensor with a per-row opacity map.  The caller compares the two passes bit for bit.
//   usage: planar_gpu <dir>
//   <dir>/meta.txt      S crop_w crop_h K idx_0 ... idx_{K-1}, then per frame: format (BGR) W H stride bytes
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the interleaved frames' bytes, one after another
//   <dir>/boxes.i32     S x 4 face boxes              <dir>/tmpl.f32    K x 2 template points
//   <dir>/tensor.f16    S x 3 x crop_h x crop_w       <dir>/alpha.u8    S x crop_h x crop_w
// writes per pass p in {packed, planar}: rows_p.f32 (S x 2L), crops_p.u8 (S x crop_h x crop_w x 3), mats_p.f32, flags_p.i32 and
// paste_p.u8 -- the frames' bytes after the paste; planar: per frame the whole allocation, plane c at c * D with D = H * W + (s even ? 67
// : 0) and a row stride of W, the bytes between the planes 0xA5 before the paste
#include "rcr/alignment.hpp"

#include "gpu_driver.hpp"

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "planar_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt");
        const int S = sc.S, cw = sc.w, ch = sc.h, K = (int)sc.lm.size();
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        auto tm = read_all<float>(dir + "/tmpl.f32");
        auto tensor = read_all<uint8_t>(dir + "/tensor.f16");
        auto alpha = read_all<uint8_t>(dir + "/alpha.u8");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)boxes.size() != 4 * S || (int)tm.size() != 2 * K || tensor.size() != (size_t)S * 3 * cw * ch * 2 || alpha.size() != (size_t)S * cw * ch)
            throw std::runtime_error("scenario size mismatch");
        DeviceMemory mem;
        const uint8_t* in_dev = mem.upload(tensor.data(), tensor.size());
        const rcr::PasteMask mask{mem.upload(alpha.data(), alpha.size()), true};
        uint8_t* crops_dev = mem.alloc((size_t)S * cw * ch * 3);
        cv::Mat tmpl(K, 2, CV_32FC1);
        std::memcpy(tmpl.ptr<float>(0), tm.data(), tm.size() * 4);
        std::vector<cv::Rect> rects;
        for (int s = 0; s < S; ++s) rects.push_back(cv::Rect(boxes[4 * s], boxes[4 * s + 1], boxes[4 * s + 2], boxes[4 * s + 3]));
        rcr::TensorSpec crop_spec;
        crop_spec.dtype = SDM_ALIGN_U8; crop_spec.layout = SDM_ALIGN_NHWC; crop_spec.order = SDM_ALIGN_ORDER_BGR;
        rcr::TensorSpec paste_spec;                                                 // float16, NCHW, RGB
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
        for (int c = 0; c < 3; ++c) { paste_spec.scale[c] = sd[c]; paste_spec.bias[c] = mean[c]; }
        for (int pass = 0; pass < 2; ++pass) {
            const std::string p = pass ? "planar" : "packed";
            std::vector<rcr::DeviceFrame> frames;
            std::vector<size_t> sizes;
            size_t at = 0;
            for (int s = 0; s < S; ++s) {
                const int W = sc.W[s], H = sc.H[s];
                if (!pass) {
                    frames.push_back(rcr::DeviceFrame{mem.upload(pixels.data() + at, (size_t)sc.bytes[s], (size_t)(s % 4)), W, H, sc.stride[s], SDM_FRAME_BGR});
                    sizes.push_back((size_t)sc.bytes[s]);
                } else {
                    const size_t D = (size_t)H * W + (s % 2 == 0 ? 67 : 0);
                    std::vector<uint8_t> planes(2 * D + (size_t)H * W, 0xA5);
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x)
                            for (int c = 0; c < 3; ++c) planes[c * D + (size_t)y * W + x] = pixels[at + (size_t)y * sc.stride[s] + 3 * x + c];
                    const uint8_t* d = mem.upload(planes.data(), planes.size(), (size_t)(s % 4));
                    rcr::DeviceFrame f{d, W, H, W, SDM_FRAME_BGR_PLANAR};           // (the aggregate form of old: second_plane stays nullptr)
                    if (s % 2 == 0) f.second_plane = d + D;
                    frames.push_back(f);
                    sizes.push_back(planes.size());
                }
                at += (size_t)sc.bytes[s];
            }
            const cv::Mat x = model.detect_batch(frames, rects);
            if (x.rows != S || x.cols != 2 * L) throw std::runtime_error("detect_batch: unexpected shape");
            write_mat(dir + "/rows_" + p + ".f32", x);
            const rcr::aligned_tensor_result cut = rcr::aligned_crops_tensor(model, frames, x, {}, sc.lm, tmpl, cw, ch, crop_spec, crops_dev);
            std::vector<uint8_t> crops((size_t)S * cw * ch * 3);
            mem.download(crops.data(), crops_dev, crops.size());
            write_bytes(dir + "/crops_" + p + ".u8", crops.data(), crops.size());
            const rcr::paste_result res = rcr::paste_crops_tensor(model, frames, x, {}, sc.lm, tmpl, cw, ch, paste_spec, in_dev, mask);
            write_mat(dir + "/mats_" + p + ".f32", res.matrices);
            write_bytes(dir + "/flags_" + p + ".i32", res.flags.data(), (size_t)S * 4);
            std::vector<uint8_t> host;
            for (int s = 0; s < S; ++s) {
                const size_t n = host.size();
                host.resize(n + sizes[s]);
                mem.download(host.data() + n, frames[s].data, sizes[s]);
            }
            write_bytes(dir + "/paste_" + p + ".u8", host.data(), host.size());
        }
        std::printf("%d frames: detect, crop %d x %d and paste on interleaved and on planar frames\n", S, cw, ch);
        return 0;
    });
}
