// GPU test driver of rcr::tracker's motion-compensated initialisation (run by tests/test_cpp_track_motion.py on the MI355X box): the
// loop of track_gpu.cpp through tracker::motion, with tracker::last_motion behind every step.
//   usage: track_motion_gpu <dir>
//   <dir>/meta.txt      S T H W capacity search scale min_gain
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T x S x H x W (stream s of frame t is image s)
//   <dir>/boxes.i32     T x S x 4
// writes <dir>/cpp_landmarks.f32 (T x S x 2L), cpp_lost.i32 (T x S masks), cpp_motion.i32 (T x S x 6: last_motion behind every step)
// and, of the slots after the run, cpp_grids.i32 (S x 3) and cpp_chips.u8 (S x 32 x 32)
#include "rcr/tracker.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "track_motion_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int S, T, H, W, capacity, search, min_gain;
        float scale;
        meta >> S >> T >> H >> W >> capacity >> search >> scale >> min_gain;
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto frames = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        if (!meta || frames.size() != (size_t)T * S * H * W || boxes.size() != (size_t)T * S * 4) throw std::runtime_error("scenario size mismatch");
        auto box = [&](int t, int s) { const int* b = &boxes[((size_t)t * S + s) * 4]; return cv::Rect(b[0], b[1], b[2], b[3]); };

        rcr::tracker tr(model, capacity);
        tr.motion(search, scale, min_gain);
        std::vector<int> ids(S);
        std::vector<bool> have_face(S, false);
        for (int s = 0; s < S; ++s) ids[s] = s;
        std::ofstream out_l(dir + "/cpp_landmarks.f32", std::ios::binary), out_m(dir + "/cpp_lost.i32", std::ios::binary),
            out_s(dir + "/cpp_motion.i32", std::ios::binary);
        int shifted = 0;
        for (int t = 0; t < T; ++t) {
            std::vector<int> restart;
            std::vector<cv::Rect> restart_boxes;
            for (int s = 0; s < S; ++s)
                if (!have_face[s]) { restart.push_back(s); restart_boxes.push_back(box(t, s)); }
            if (!restart.empty()) tr.start(restart, restart_boxes);
            std::vector<Mat> images;
            for (int s = 0; s < S; ++s) images.push_back(Mat(H, W, CV_8UC1, frames.data() + ((size_t)t * S + s) * H * W));
            auto lms = tr.step(ids, images);
            if ((int)lms.size() != S) throw std::runtime_error("step returned the wrong number of rows");
            for (int s = 0; s < S; ++s) have_face[s] = tr.lost()[s] == 0;
            const Mat& rows = tr.rows();
            for (int r = 0; r < rows.rows; ++r) out_l.write((const char*)rows.ptr<float>(r), (std::streamsize)rows.cols * 4);
            out_m.write((const char*)tr.lost().data(), (std::streamsize)S * 4);
            for (const auto& m : tr.last_motion(ids)) {
                const int v[6] = {m.dx, m.dy, m.sad_best, m.sad_zero, m.k, m.searched};
                out_s.write((const char*)v, sizeof(v));
                shifted += m.dx != 0 || m.dy != 0;
            }
        }
        std::vector<int> grids;
        std::vector<uint8_t> chips;
        tr.last_motion(ids, &grids, &chips);
        write_bytes(dir + "/cpp_grids.i32", grids.data(), grids.size() * sizeof(int));
        write_bytes(dir + "/cpp_chips.u8", chips.data(), chips.size());
        std::printf("frames %d streams %d rows shifted %d\n", T, S, shifted);
        return 0;
    });
}
