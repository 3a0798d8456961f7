// GPU test driver of rcr/alignment.hpp (run by tests/test_gpu_align.py on the MI355X box): aligned crops of a tracker's streams after
// two frames, gray and from colour frames, and of detection_model::detect_batch's rows.
//   usage: align_gpu <dir>
//   <dir>/meta.txt      S T H W K idx_0 .. idx_{K-1}
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     T x S x H x W (stream s of frame t is image s)
//   <dir>/colour.u8     S x H x W x 3: colour versions of frame 1
//   <dir>/boxes.i32     T x S x 4
// writes track_gray.u8, track_mats.f32, track_flags.i32, track_colour.u8, detect_rows.f32, detect_gray.u8, detect_mats.f32
#include "rcr/alignment.hpp"

#include "gpu_driver.hpp"

using cv::Mat;

static void write_crops(const std::string& path, const rcr::aligned_crops_result& r)
{
    std::ofstream f(path, std::ios::binary);
    for (const auto& m : r.crops) f.write((const char*)m.ptr<uint8_t>(0), (std::streamsize)(m.rows * m.step()));
}

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "align_gpu", [](const std::string& dir) {
        std::ifstream meta(dir + "/meta.txt");
        int S, T, H, W, K;
        meta >> S >> T >> H >> W >> K;
        std::vector<int> lm(K);
        for (int k = 0; k < K; ++k) meta >> lm[k];
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto frames = read_all<uint8_t>(dir + "/frames.u8");
        auto colour = read_all<uint8_t>(dir + "/colour.u8");
        auto boxes = read_all<int>(dir + "/boxes.i32");
        if (frames.size() != (size_t)T * S * H * W || colour.size() != (size_t)S * H * W * 3 || boxes.size() != (size_t)T * S * 4 || T < 2)
            throw std::runtime_error("scenario size mismatch");
        auto frame = [&](int t) {
            std::vector<Mat> v;
            for (int s = 0; s < S; ++s) v.push_back(Mat(H, W, CV_8UC1, frames.data() + ((size_t)t * S + s) * H * W));
            return v;
        };
        std::vector<cv::Rect> b0;
        for (int s = 0; s < S; ++s) b0.push_back(cv::Rect(boxes[4 * s], boxes[4 * s + 1], boxes[4 * s + 2], boxes[4 * s + 3]));
        const Mat tmpl = rcr::alignment_template(model.get_mean(), lm, 112, 112, 0.2);

        rcr::tracker tr(model, S);
        std::vector<int> ids(S);
        for (int s = 0; s < S; ++s) ids[s] = s;
        tr.start(ids, b0);
        tr.step(ids, frame(0));
        tr.step(ids, frame(1));
        auto gray = rcr::aligned_crops(tr, lm, tmpl, 112, 112);
        std::vector<Mat> bgr;
        for (int s = 0; s < S; ++s) bgr.push_back(Mat(H, W, CV_8UC3, colour.data() + (size_t)s * H * W * 3));
        auto col = rcr::aligned_crops(tr, lm, tmpl, 112, 112, bgr);
        if ((int)gray.crops.size() != S || col.crops[0].channels() != 3) throw std::runtime_error("unexpected crop shapes");
        write_crops(dir + "/track_gray.u8", gray);
        write_mat(dir + "/track_mats.f32", gray.matrices);
        write_bytes(dir + "/track_flags.i32", gray.flags.data(), (size_t)S * 4);
        write_crops(dir + "/track_colour.u8", col);

        const std::vector<Mat> f0 = frame(0);
        Mat rows = model.detect_batch(f0, b0);
        auto det = rcr::aligned_crops(model, f0, rows, {}, lm, tmpl, 112, 112);
        write_mat(dir + "/detect_rows.f32", rows);
        write_crops(dir + "/detect_gray.u8", det);
        write_mat(dir + "/detect_mats.f32", det.matrices);
        int partial = 0;
        for (int f : gray.flags) partial += (f & SDM_ALIGN_PARTIAL) != 0;
        std::printf("streams %d, crops 112 x 112 gray + colour, partial %d\n", S, partial);
        return 0;
    });
}
