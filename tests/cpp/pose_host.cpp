// Host operator() of the library ModelProjection (superviseddescent/model_projection.hpp), for tests/test_pose_host.py.
// Input file: K, K lines "X Y Z", the camera "focal width height near far", N, N lines of 6 parameters.
// Output: one line of 2K projections (%.9g) per parameter row.
#include "superviseddescent/model_projection.hpp"

#include <cstdio>

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: pose_host <input>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int K = 0, N = 0;
    if (std::fscanf(f, "%d", &K) != 1) return 2;
    cv::Mat model(4, K, CV_32FC1);
    for (int k = 0; k < K; ++k) {
        for (int r = 0; r < 3; ++r) if (std::fscanf(f, "%f", &model.at<float>(r, k)) != 1) return 2;
        model.at<float>(3, k) = 1.0f;
    }
    float cam[5];
    for (float& v : cam) if (std::fscanf(f, "%f", &v) != 1) return 2;
    superviseddescent::ModelProjection projection(model, cam[0], cam[1], cam[2], cam[3], cam[4]);
    if (std::fscanf(f, "%d", &N) != 1) return 2;
    for (int n = 0; n < N; ++n) {
        cv::Mat x(1, 6, CV_32FC1);
        for (int j = 0; j < 6; ++j) if (std::fscanf(f, "%f", &x.at<float>(0, j)) != 1) return 2;
        cv::Mat y = projection(x, 0);
        for (int i = 0; i < y.cols; ++i) std::printf(i ? " %.9g" : "%.9g", y.at<float>(0, i));
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
