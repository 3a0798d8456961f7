// GPU test driver of rcr::tracker's temporal landmark filter (run by tests/test_cpp_track_filter.py on the MI355X box): the loop of
// track_gpu.cpp through tracker::smooth and the step overloads that take dt -- a vector of step times on cv::Mat frames, one value
// for all rows on every third frame, and the same frames on the device (rcr::DeviceFrame) on every fourth.
//   usage: track_filter_gpu <dir>
//   <dir>/meta.txt      S T H W capacity min_cutoff beta d_cutoff
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T x S x H x W (stream s of frame t is image s)
//   <dir>/boxes.i32     T x S x 4
//   <dir>/dt.f32        T x S step times (a frame stepped with one value takes its first)
// writes <dir>/cpp_filtered.f32 and cpp_raw.f32 (T x S x 2L: the filtered rows and the cascade's own of every step), cpp_lost.i32
// (T x S masks), and of the slots after the run cpp_state.f32 (S x 2L filtered rows, then S x 2L derivative rows) and cpp_primed.i32
#include "rcr/tracker.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "track_filter_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int S, T, H, W, capacity;
        float min_cutoff, beta, d_cutoff;
        meta >> S >> T >> H >> W >> capacity >> min_cutoff >> beta >> d_cutoff;
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto frames = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        auto dts = read_all<float>(dir + "/dt.f32");
        if (!meta || frames.size() != (size_t)T * S * H * W || boxes.size() != (size_t)T * S * 4 || dts.size() != (size_t)T * S)
            throw std::runtime_error("scenario size mismatch");
        auto box = [&](int t, int s) { const int* b = &boxes[((size_t)t * S + s) * 4]; return cv::Rect(b[0], b[1], b[2], b[3]); };

        DeviceMemory mem;
        const uint8_t* frames_dev = mem.upload(frames.data(), frames.size());
        rcr::tracker tr(model, capacity);
        tr.smooth(min_cutoff, beta, d_cutoff);
        std::vector<int> ids(S);
        std::vector<bool> have_face(S, false);
        for (int s = 0; s < S; ++s) ids[s] = s;
        std::ofstream out_f(dir + "/cpp_filtered.f32", std::ios::binary), out_r(dir + "/cpp_raw.f32", std::ios::binary),
            out_m(dir + "/cpp_lost.i32", std::ios::binary);
        int restarts = 0, moved = 0;
        for (int t = 0; t < T; ++t) {
            std::vector<int> restart;
            std::vector<cv::Rect> restart_boxes;
            for (int s = 0; s < S; ++s)
                if (!have_face[s]) { restart.push_back(s); restart_boxes.push_back(box(t, s)); }
            if (!restart.empty()) { tr.start(restart, restart_boxes); restarts += t > 0 ? (int)restart.size() : 0; }
            const std::vector<float> dt(dts.begin() + (size_t)t * S, dts.begin() + (size_t)(t + 1) * S);
            std::vector<rcr::LandmarkCollection<cv::Vec2f>> lms;
            if (t % 4 == 3) {
                std::vector<rcr::DeviceFrame> dev;
                for (int s = 0; s < S; ++s) dev.push_back(rcr::DeviceFrame{frames_dev + ((size_t)t * S + s) * H * W, W, H, W, SDM_FRAME_GRAY});
                lms = t % 3 == 0 ? tr.step(ids, dev, dt[0]) : tr.step(ids, dev, dt);
            } else {
                std::vector<Mat> images;
                for (int s = 0; s < S; ++s) images.push_back(Mat(H, W, CV_8UC1, frames.data() + ((size_t)t * S + s) * H * W));
                lms = t % 3 == 0 ? tr.step(ids, images, dt[0]) : tr.step(ids, images, dt);
            }
            if ((int)lms.size() != S) throw std::runtime_error("step returned the wrong number of rows");
            for (int s = 0; s < S; ++s) have_face[s] = tr.lost()[s] == 0;
            const Mat &rows = tr.rows(), &raw = tr.raw_rows();
            for (int r = 0; r < rows.rows; ++r) {
                out_f.write((const char*)rows.ptr<float>(r), (std::streamsize)rows.cols * 4);
                out_r.write((const char*)raw.ptr<float>(r), (std::streamsize)raw.cols * 4);
                moved += std::memcmp(rows.ptr<float>(r), raw.ptr<float>(r), (size_t)rows.cols * 4) != 0;
            }
            out_m.write((const char*)tr.lost().data(), (std::streamsize)S * 4);
        }
        Mat derivative;
        auto got = tr.get_filtered(ids, &derivative);
        Mat state((int)ids.size(), derivative.cols, CV_32FC1);
        for (int s = 0; s < S; ++s) {
            const auto& lm = got.first[s];
            if ((int)lm.size() * 2 != derivative.cols) throw std::runtime_error("get_filtered returned the wrong number of landmarks");
            for (int k = 0; k < (int)lm.size(); ++k) {
                state.at<float>(s, k) = lm[k].coordinates[0];
                state.at<float>(s, k + (int)lm.size()) = lm[k].coordinates[1];
            }
        }
        std::ofstream out_s(dir + "/cpp_state.f32", std::ios::binary);
        for (const Mat* m : {&state, &derivative})
            for (int r = 0; r < m->rows; ++r) out_s.write((const char*)m->ptr<float>(r), (std::streamsize)m->cols * 4);
        write_bytes(dir + "/cpp_primed.i32", got.second.data(), got.second.size() * sizeof(int));
        std::printf("frames %d streams %d restarts %d rows the filter moved %d\n", T, S, restarts, moved);
        return 0;
    });
}
