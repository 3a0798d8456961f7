// The reference's examples/pose_estimation.cpp (main, :249-340) written against the library ModelProjection
// (superviseddescent/model_projection.hpp): 6-DOF pose of a 10-point face model learned from 500 random poses with three
// LinearRegressor<> levels, then predicted for the example's landmark row.  With a ModelProjection the optimiser runs on the
// device (csrc/sdm_pose.hip).  The random poses come from a FIXED seed (the reference seeds from std::random_device), so the
// test can repeat the training in float64; argv[1] (optional) receives them, one row of 6 per line.
#include "superviseddescent/model_projection.hpp"

#include <cstdio>
#include <iostream>
#include <random>

using namespace superviseddescent;
using cv::Mat;

int main(int argc, char** argv)
{
    // the example's 3D points (iBug numbers 31, 34, 37, 40, 43, 46, 49, 52, 55, 58), one column per point, homogeneous
    const float pts[10][3] = {{-0.287526f, -2.0203f, 3.33725f},   {-0.11479f, -17.2056f, -13.5569f}, {-46.1668f, 34.7219f, -35.938f},
                              {-18.926f, 31.5432f, -29.9641f},    {19.2574f, 31.5767f, -30.229f},    {46.1914f, 34.452f, -36.1317f},
                              {-23.7552f, -35.7461f, -28.2573f},  {-0.0753515f, -28.3064f, -12.8984f}, {23.7138f, -35.7886f, -28.5949f},
                              {0.125511f, -44.7427f, -17.1411f}};
    Mat facemodel(4, 10, CV_32FC1);
    for (int k = 0; k < 10; ++k) {
        for (int r = 0; r < 3; ++r) facemodel.at<float>(r, k) = pts[k][r];
        facemodel.at<float>(3, k) = 1.0f;
    }

    std::mt19937 engine(20161016u);
    std::uniform_real_distribution<float> angle(-30.0f, 30.0f);

    std::vector<LinearRegressor<>> regressors;
    for (int i = 0; i < 3; ++i) regressors.emplace_back(Regulariser(Regulariser::RegularisationType::MatrixNorm, 2.0f, true));
    SupervisedDescentOptimiser<LinearRegressor<>> model(regressors);
    ModelProjection projection(facemodel);

    const int n = 500;
    Mat x_tr(n, 6, CV_32FC1);
    for (int r = 0; r < n; ++r) {
        for (int j = 0; j < 3; ++j) x_tr.at<float>(r, j) = angle(engine);
        x_tr.at<float>(r, 3) = 0.0f;
        x_tr.at<float>(r, 4) = 0.0f;
        x_tr.at<float>(r, 5) = -2000.0f;
    }
    Mat y_tr(n, 20, CV_32FC1);
    for (int r = 0; r < n; ++r) {
        Mat y = projection(x_tr.row(r), 0);
        Mat dst = y_tr.row(r);
        y.copyTo(dst);
    }
    Mat x0 = Mat::zeros(n, 6, CV_32FC1);
    for (int r = 0; r < n; ++r) x0.at<float>(r, 5) = -2000.0f;

    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "w");
        for (int r = 0; r < n; ++r)
            std::fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g\n", x_tr.at<float>(r, 0), x_tr.at<float>(r, 1), x_tr.at<float>(r, 2),
                         x_tr.at<float>(r, 3), x_tr.at<float>(r, 4), x_tr.at<float>(r, 5));
        std::fclose(f);
    }

    std::cout << "Training the model, printing the residual after each learned regressor: " << std::endl;
    auto print_residual = [&x_tr](const Mat& current) { std::cout << cv::norm(current, x_tr) / cv::norm(x_tr) << std::endl; };
    model.train(x_tr, x0, y_tr, projection, print_residual);

    const float lm[20] = {498.0f, 504.0f, 479.0f, 498.0f, 529.0f, 553.0f, 489.0f, 503.0f, 527.0f, 503.0f,
                          502.0f, 513.0f, 457.0f, 465.0f, 471.0f, 471.0f, 522.0f, 522.0f, 530.0f, 536.0f};
    Mat landmarks(1, 20, CV_32FC1);
    for (int i = 0; i < 20; ++i) landmarks.at<float>(0, i) = (lm[i] - 500.0f) / 1800.0f;     // :327
    Mat init = Mat::zeros(1, 6, CV_32FC1);
    init.at<float>(0, 5) = -2000.0f;
    Mat p = model.predict(init, landmarks, projection);
    std::cout << "Groundtruth pose: pitch = 11.0, yaw = -25.0, roll = -10.0" << std::endl;
    std::printf("Predicted pose: pitch = %.9g, yaw = %.9g, roll = %.9g, t = %.9g %.9g %.9g\n", p.at<float>(0, 0), p.at<float>(0, 1),
                p.at<float>(0, 2), p.at<float>(0, 3), p.at<float>(0, 4), p.at<float>(0, 5));
    return 0;
}
