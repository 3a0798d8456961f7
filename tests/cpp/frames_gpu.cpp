// GPU test driver of the rcr::DeviceFrame overloads (run by tests/test_cpp_frames.py on the MI355X box): detection_model::detect_batch
// and tracker::step on colour frames that are already on the device against the cv::Mat overloads on the same pixels.
//   usage: frames_gpu <dir>
//   <dir>/meta.txt      S T, then per stream: H W
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T frames of S images each, image s dense H_s x W_s x 3 (BGR)
//   <dir>/boxes.i32     S x 4
// writes detect_mat.f32, detect_dev.f32, track_mat.f32, track_dev.f32 (the rows after frame T - 1) and exits 1 when they differ
#include "rcr/tracker.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

static bool same_bits(const Mat& a, const Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int r = 0; r < a.rows; ++r)
        if (std::memcmp(a.ptr<float>(r), b.ptr<float>(r), (size_t)a.cols * 4) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "frames_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int S, T;
        meta >> S >> T;
        std::vector<int> H(S), W(S);
        size_t per_frame = 0;
        for (int s = 0; s < S; ++s) { meta >> H[s] >> W[s]; per_frame += (size_t)H[s] * W[s] * 3; }
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        if (pixels.size() != per_frame * T || boxes.size() != (size_t)S * 4 || T < 2) throw std::runtime_error("scenario size mismatch");
        std::vector<cv::Rect> b0;
        for (int s = 0; s < S; ++s) b0.push_back(cv::Rect(boxes[4 * s], boxes[4 * s + 1], boxes[4 * s + 2], boxes[4 * s + 3]));
        std::vector<int> ids(S);
        for (int s = 0; s < S; ++s) ids[s] = s;

        DeviceMemory mem;
        rcr::tracker tr_mat(model, S), tr_dev(model, S);
        // every frame on the host as cv::Mat views, and on the device with a pitch of its own (row + 5 + s bytes: odd row starts)
        std::vector<std::vector<Mat>> mats(T);
        std::vector<std::vector<rcr::DeviceFrame>> devs(T);
        size_t at = 0;
        for (int t = 0; t < T; ++t)
            for (int s = 0; s < S; ++s) {
                uint8_t* p = pixels.data() + at;
                at += (size_t)H[s] * W[s] * 3;
                mats[t].push_back(Mat(H[s], W[s], CV_8UC3, p));
                const size_t row = (size_t)W[s] * 3, pitch = row + 5 + s;
                std::vector<uint8_t> pitched(pitch * H[s], 0);
                for (int y = 0; y < H[s]; ++y) std::memcpy(pitched.data() + y * pitch, p + y * row, row);
                devs[t].push_back(rcr::DeviceFrame{mem.upload(pitched.data(), pitched.size()), W[s], H[s], (int)pitch, SDM_FRAME_BGR});
            }

        const Mat rows_mat = model.detect_batch(mats[0], b0);
        const Mat rows_dev = model.detect_batch(devs[0], b0);
        write_mat(dir + "/detect_mat.f32", rows_mat);
        write_mat(dir + "/detect_dev.f32", rows_dev);
        bool ok = same_bits(rows_mat, rows_dev);

        tr_mat.start(ids, b0);
        tr_dev.start(ids, b0);
        for (int t = 0; t < T; ++t) {
            tr_mat.step(ids, mats[t]);
            tr_dev.step(ids, devs[t]);
            ok = ok && same_bits(tr_mat.rows(), tr_dev.rows()) && tr_mat.lost() == tr_dev.lost();
        }
        write_mat(dir + "/track_mat.f32", tr_mat.rows());
        write_mat(dir + "/track_dev.f32", tr_dev.rows());
        std::printf("streams %d, frames %d: DeviceFrame overloads %s the cv::Mat overloads\n", S, T, ok ? "equal" : "DIFFER from");
        return ok ? 0 : 1;
    });
}
