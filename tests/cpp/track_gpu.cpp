// GPU test driver of rcr::tracker (run by tests/test_gpu_track.py on the MI355X box): the loop of the reference's
// apps/rcr/rcr-track.cpp:133-177 on synthetic video, with the scenario's boxes standing in for the face detector -- start every
// stream on the first frame, step all of them on every frame, and restart a stream from that frame's box once it is reported lost.
//   usage: track_gpu <dir>
//   <dir>/meta.txt      S T H W capacity
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T x S x H x W (stream s of frame t is image s)
//   <dir>/boxes.i32     T x S x 4
// writes <dir>/cpp_landmarks.f32 (T x S x 2L, the rows of every step) and <dir>/cpp_lost.i32 (T x S masks)
#include "rcr/tracker.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "track_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int S, T, H, W, capacity;
        meta >> S >> T >> H >> W >> capacity;
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto frames = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        if (frames.size() != (size_t)T * S * H * W || boxes.size() != (size_t)T * S * 4) throw std::runtime_error("scenario size mismatch");
        auto box = [&](int t, int s) { const int* b = &boxes[((size_t)t * S + s) * 4]; return cv::Rect(b[0], b[1], b[2], b[3]); };

        rcr::tracker tr(model, capacity);
        std::vector<int> ids(S);
        std::vector<bool> have_face(S, false);
        for (int s = 0; s < S; ++s) ids[s] = s;
        std::ofstream out_l(dir + "/cpp_landmarks.f32", std::ios::binary), out_m(dir + "/cpp_lost.i32", std::ios::binary);
        int restarts = 0;
        for (int t = 0; t < T; ++t) {
            std::vector<int> restart;
            std::vector<cv::Rect> restart_boxes;
            for (int s = 0; s < S; ++s)
                if (!have_face[s]) { restart.push_back(s); restart_boxes.push_back(box(t, s)); }   // "run the face detector"
            if (!restart.empty()) { tr.start(restart, restart_boxes); restarts += t > 0 ? (int)restart.size() : 0; }
            std::vector<Mat> images;
            for (int s = 0; s < S; ++s) images.push_back(Mat(H, W, CV_8UC1, frames.data() + ((size_t)t * S + s) * H * W));
            auto lms = tr.step(ids, images);
            if ((int)lms.size() != S) throw std::runtime_error("step returned the wrong number of rows");
            for (int s = 0; s < S; ++s) have_face[s] = tr.lost()[s] == 0;
            const Mat& rows = tr.rows();
            for (int r = 0; r < rows.rows; ++r) out_l.write((const char*)rows.ptr<float>(r), (std::streamsize)rows.cols * 4);
            out_m.write((const char*)tr.lost().data(), (std::streamsize)S * 4);
        }
        // the slot table after the run: statuses of every stream, and landmark access by id
        auto got = tr.get(ids);
        int tracked = 0;
        for (int s = 0; s < S; ++s) tracked += got.second[s] == rcr::tracker::tracked;
        std::printf("frames %d streams %d restarts %d tracked at the end %d\n", T, S, restarts, tracked);
        return 0;
    });
}
