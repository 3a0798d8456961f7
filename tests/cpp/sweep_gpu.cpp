// GPU test driver of the regulariser sweep through the C++ header layer (run by tests/test_cpp_sweep.py on the MI355X box).
// Reads the scenario the Python test wrote (raw little-endian arrays), trains it with
// SupervisedDescentOptimiser<LinearRegressor<>, InterEyeDistanceNormalisation>::train(..., callback, holdout) over regressors
// constructed from a RegulariserSweep, and writes the regressors and the sweep records back for comparison with the Python layer.
//   usage: sweep_gpu <dir>
#include "rcr/model.hpp"

#include "gpu_driver.hpp"

#include <cmath>
#include <iostream>

using cv::Mat;
using namespace superviseddescent;

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "sweep_gpu", [](const std::string& dir) {
        // meta: n_images H W N L n_levels holdout, per level: variant cells cell bins rel, ids..., right eye ids, left eye ids,
        // then reg_type regularise_last_row K and the K candidates
        std::ifstream meta(dir + "/meta.txt");
        int n_img, H, W, N, L, n_levels, holdout;
        meta >> n_img >> H >> W >> N >> L >> n_levels >> holdout;
        std::vector<rcr::HoGParam> hog_params;
        for (int l = 0; l < n_levels; ++l) {
            int v, c, cs, b; float rel;
            meta >> v >> c >> cs >> b >> rel;
            hog_params.push_back({v ? VlHogVariantUoctti : VlHogVariantDalalTriggs, c, cs, b, rel});
        }
        std::vector<std::string> ids(L), re(2), le(2);
        for (auto& s : ids) meta >> s;
        for (auto& s : re) meta >> s;
        for (auto& s : le) meta >> s;
        int reg_type, reg_last, K;
        meta >> reg_type >> reg_last >> K;
        std::vector<float> candidates((size_t)K);
        for (auto& p : candidates) meta >> p;
        const auto type = reg_type ? Regulariser::RegularisationType::MatrixNorm : Regulariser::RegularisationType::Manual;

        auto img_bytes = read_all<uint8_t>(dir + "/images.u8");
        std::vector<Mat> images;
        for (int i = 0; i < n_img; ++i) images.push_back(Mat(H, W, CV_8UC1, img_bytes.data() + (size_t)i * H * W));
        auto x0v = read_all<float>(dir + "/x0.f32");
        auto xsv = read_all<float>(dir + "/xstar.f32");
        auto idx = read_all<int>(dir + "/img_index.i32");
        Mat x0(N, 2 * L, CV_32FC1, x0v.data()), xstar(N, 2 * L, CV_32FC1, xsv.data());

        using LR = LinearRegressor<>;
        std::vector<LR> regressors;
        for (int l = 0; l < n_levels; ++l) regressors.emplace_back(LR(RegulariserSweep(type, candidates, reg_last != 0)));
        SupervisedDescentOptimiser<LR, rcr::InterEyeDistanceNormalisation> model(regressors, rcr::InterEyeDistanceNormalisation(ids, re, le));
        rcr::HogTransform hog(images, hog_params, ids, re, le);
        hog.sample_image_index = idx;

        // a sweep without held-out rows is refused, on the device path and by the host-only generic path
        bool refused = false;
        try { model.train(xstar, x0, Mat(), hog); } catch (const std::invalid_argument&) { refused = true; }
        if (!refused) throw std::runtime_error("train() without a hold-out count accepted a RegulariserSweep");
        refused = false;
        try {
            SupervisedDescentOptimiser<LR> generic(std::vector<LR>(1, LR(RegulariserSweep(type, candidates, true))));
            Mat y = (cv::Mat_<float>(3, 1) << 1.0f, 2.0f, 3.0f), start = (cv::Mat_<float>(3, 1) << 0.5f, 0.5f, 0.5f);
            generic.train(y, start, Mat(), [](Mat v, size_t, int) { return v.at<float>(0) * 2.0f; });
        } catch (const std::invalid_argument&) { refused = true; }
        if (!refused) throw std::runtime_error("the generic host path accepted a RegulariserSweep");

        int epochs = 0;
        Mat last;
        model.train(xstar, x0, Mat(), hog, [&](const Mat& cur) { ++epochs; last = cur; }, holdout);
        if (epochs != n_levels) throw std::runtime_error("callback count");
        write_mat(dir + "/cpp_x_train.f32", last);
        std::ofstream rec(dir + "/cpp_sweep.txt");
        rec.precision(17);
        for (int l = 0; l < n_levels; ++l) {
            const LR& r = model.get_regressors()[l];
            const SweepRecord& s = r.get_sweep();
            if ((int)s.params.size() != K || s.best < 0 || s.best >= K) throw std::runtime_error("sweep record");
            if (r.get_regulariser().param() != candidates[(size_t)s.best]) throw std::runtime_error("the winner's parameter is not the regulariser's");
            write_mat(dir + "/cpp_R" + std::to_string(l) + ".f32", r.x);
            rec << s.best;
            for (int k = 0; k < K; ++k) rec << " " << s.holdout_errors[(size_t)k] << " " << s.fit_errors[(size_t)k] << " " << (double)s.lambdas[(size_t)k] << " " << s.status[(size_t)k];
            rec << "\n";
        }
        write_mat(dir + "/cpp_x_test.f32", model.test(x0, Mat(), hog));
        std::printf("sweep_gpu ok\n");
        return 0;
    });
}
