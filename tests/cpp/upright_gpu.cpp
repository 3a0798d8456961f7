// GPU test driver of rcr::detection_model::detect_batch_upright and of rcr::tracker's upright mode (run by tests/test_cpp_upright.py on
// the MI355X box): rolled boxes on three frames of different sizes, then an upright tracker started from the same boxes and rolls and
// stepped over T sets of those frames.
//   usage: upright_gpu <dir>
//   <dir>/meta.txt      n T chip guard, then n lines "width height"
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T sets of the n frames, each dense
//   <dir>/boxes.i32     n x 4        <dir>/rolls.f32   n
// writes cpp_detect.f32 (n x 2L), cpp_mats.f32 (n x 6), cpp_flags.i32 (n), cpp_track.f32 (T x n x 2L), cpp_lost.i32 (T x n)
#include "rcr/tracker.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "upright_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int n, T, chip, guard;
        meta >> n >> T >> chip >> guard;
        std::vector<int> w(n), h(n);
        size_t set_bytes = 0;
        for (int i = 0; i < n; ++i) { meta >> w[i] >> h[i]; set_bytes += (size_t)w[i] * h[i]; }
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto frames = read_all<uint8_t>(dir + "/frames.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        auto rolls = read_all<float>(dir + "/rolls.f32");
        if (frames.size() != set_bytes * T || (int)boxes.size() != 4 * n || (int)rolls.size() != n) throw std::runtime_error("scenario size mismatch");
        auto images_of = [&](int t) {
            std::vector<Mat> images;
            uint8_t* p = frames.data() + (size_t)t * set_bytes;
            for (int i = 0; i < n; ++i) { images.push_back(Mat(h[i], w[i], CV_8UC1, p)); p += (size_t)w[i] * h[i]; }
            return images;
        };
        std::vector<cv::Rect> rects;
        std::vector<int> ids;
        for (int i = 0; i < n; ++i) { rects.push_back(cv::Rect(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3])); ids.push_back(i); }

        Mat x = model.detect_batch_upright(images_of(0), rects, rolls, chip, guard);
        if (x.rows != n || !x.isContinuous()) throw std::runtime_error("detect_batch_upright returned the wrong rows");
        write_bytes(dir + "/cpp_detect.f32", x.ptr<float>(0), (size_t)x.rows * x.cols * 4);
        write_bytes(dir + "/cpp_mats.f32", model.upright_matrices().ptr<float>(0), (size_t)n * 6 * 4);
        write_bytes(dir + "/cpp_flags.i32", model.upright_flags().data(), (size_t)n * 4);

        rcr::tracker tr(model, n);
        tr.upright(chip, guard);
        tr.start(ids, rects, rolls);
        std::ofstream out_l(dir + "/cpp_track.f32", std::ios::binary), out_m(dir + "/cpp_lost.i32", std::ios::binary);
        int lost = 0;
        for (int t = 0; t < T; ++t) {
            tr.step(ids, images_of(t));
            const Mat& rows = tr.rows();
            for (int r = 0; r < rows.rows; ++r) out_l.write((const char*)rows.ptr<float>(r), (std::streamsize)rows.cols * 4);
            out_m.write((const char*)tr.lost().data(), (std::streamsize)n * 4);
            std::vector<int> again;
            std::vector<cv::Rect> again_boxes;
            std::vector<float> again_rolls;
            for (int i = 0; i < n; ++i)
                if (tr.lost()[i]) { again.push_back(i); again_boxes.push_back(rects[i]); again_rolls.push_back(rolls[i]); ++lost; }
            if (!again.empty()) tr.start(again, again_boxes, again_rolls);
        }
        std::printf("upright detect of %d rows, %d upright tracker steps, %d restarts\n", n, T, lost);
        return 0;
    });
}
