// superviseddescent/model_projection.hpp -- the ModelProjection of the reference's examples/pose_estimation.cpp:187-240 as a
// library type: 6-DOF head pose [r_x, r_y, r_z, t_x, t_y, t_z] (degrees) -> normalised 2D projections of a 3D model.  The
// example defines it in its own source file; here it is a library type (as rcr::FixedHogTransform is for
// examples/landmark_detection.cpp) so that SupervisedDescentOptimiser can route it to the batched device path
// (csrc/sdm_pose.hip through include/sdm.h's sdm_pose_*):
//
//   SupervisedDescentOptimiser<LinearRegressor<PartialPivLUSolver | VerbosePartialPivLUSolver>, NoNormalisation>
//       ::train / test / predict with a ModelProjection   -> one device launch sequence per level (train), all levels in one
//                                                            launch (test / predict; per level when a callback is given)
//
// LinearRegressor<ColPivHouseholderQRSolver> stays on the generic host path (one task per sample, the solver's own QR), as do
// normalisations other than NoNormalisation.
#pragma once

#ifndef SUPERVISEDDESCENT_MODEL_PROJECTION_HPP_
#define SUPERVISEDDESCENT_MODEL_PROJECTION_HPP_

#include "superviseddescent/hip_backend.hpp"
#include "superviseddescent/regressors.hpp"
#include "superviseddescent/superviseddescent.hpp"

#include <cmath>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace superviseddescent {

/** Projects a 3D model with the parameters [r_x, r_y, r_z, t_x, t_y, t_z] through a pinhole camera (pose_estimation.cpp:187-240).
 *  The camera defaults are the example's: focal length 1800, a 1000 x 1000 screen, near 1, far 5000. */
class ModelProjection {
public:
    /** model: 4 x K homogeneous points (CV_32F), as the example builds it (:257-267); 3 x K is accepted too.  1 <= K <= 64. */
    explicit ModelProjection(cv::Mat model, float focal_length = 1800.0f, float screen_width = 1000.0f, float screen_height = 1000.0f,
                             float near_plane = 1.0f, float far_plane = 5000.0f)
        : focal(focal_length), width(screen_width), height(screen_height), near_plane(near_plane), far_plane(far_plane)
    {
        if ((model.rows != 4 && model.rows != 3) || model.cols < 1 || model.cols > 64)
            throw std::runtime_error("ModelProjection: the model must be 4 x K (or 3 x K), 1 <= K <= 64");
        points.resize((size_t)model.cols * 3);
        for (int k = 0; k < model.cols; ++k)
            for (int r = 0; r < 3; ++r) points[(size_t)k * 3 + r] = model.at<float>(r, k);
        // focalLengthToFovy (:46) and createPerspectiveProjectionMatrix (:142-154), in float as there
        const float fovy = (2.0f * std::atan2(height, 2.0f * focal)) * static_cast<float>(180 / 3.14159265358979323846);
        const float radians = (fovy / 2.0f) * static_cast<float>(3.14159265358979323846) / 180.0f;
        const float cotan = std::cos(radians) / std::sin(radians);
        const float aspect = width / height;
        const float P[16] = {cotan / aspect, 0.f, 0.f, 0.f, 0.f, cotan, 0.f, 0.f, 0.f, 0.f, -(near_plane + far_plane) / (far_plane - near_plane),
                             (-2.0f * near_plane * far_plane) / (far_plane - near_plane), 0.f, 0.f, -1.0f, 0.f};
        for (int i = 0; i < 16; ++i) projection[i] = P[i];
    }

    /** Normalised 2D projections [u_0..u_{K-1}, v_0..v_{K-1}] (1 x 2K) of one parameter row (1 x 6 or 6 x 1), evaluated on the host
     *  -- what users synthesise training data with (:305-309).  regressor_level and training_index are not used, as in the example. */
    cv::Mat operator()(cv::Mat parameters, size_t /*regressor_level*/, int /*training_index*/ = 0) const
    {
        if (!((parameters.rows == 1 && parameters.cols == 6) || (parameters.rows == 6 && parameters.cols == 1)))
            throw std::runtime_error("ModelProjection: parameters must be 1 x 6 or 6 x 1");
        float x[6];
        for (int i = 0; i < 6; ++i) x[i] = parameters.at<float>(i);
        const float d2r = static_cast<float>(3.14159265358979323846 / 180);        // deg2rad, :41
        const float rx = x[0] * d2r, ry = x[1] * d2r, rz = x[2] * d2r;
        const float cx = std::cos(rx), sx = std::sin(rx), cy = std::cos(ry), sy = std::sin(ry), cz = std::cos(rz), sz = std::sin(rz);
        const float T[16] = {1.f, 0.f, 0.f, x[3], 0.f, 1.f, 0.f, x[4], 0.f, 0.f, 1.f, x[5], 0.f, 0.f, 0.f, 1.f};
        const float Ry[16] = {cy, 0.f, sy, 0.f, 0.f, 1.f, 0.f, 0.f, -sy, 0.f, cy, 0.f, 0.f, 0.f, 0.f, 1.f};
        const float Rx[16] = {1.f, 0.f, 0.f, 0.f, 0.f, cx, -sx, 0.f, 0.f, sx, cx, 0.f, 0.f, 0.f, 0.f, 1.f};
        const float Rz[16] = {cz, -sz, 0.f, 0.f, sz, cz, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        float a[16], b[16], mvp[16];
        mul4(T, Ry, a);                 // model matrix T * R_y * R_x * R_z (:222)
        mul4(a, Rx, b);
        mul4(b, Rz, a);
        mul4(projection, a, mvp);
        const int K = num_points();
        cv::Mat out(1, 2 * K, CV_32FC1);
        const float hw = width / 2.0f, hh = height / 2.0f;
        for (int k = 0; k < K; ++k) {
            const float X = points[(size_t)k * 3], Y = points[(size_t)k * 3 + 1], Z = points[(size_t)k * 3 + 2];
            const float c0 = mvp[0] * X + mvp[1] * Y + mvp[2] * Z + mvp[3];
            const float c1 = mvp[4] * X + mvp[5] * Y + mvp[6] * Z + mvp[7];
            const float c3 = mvp[12] * X + mvp[13] * Y + mvp[14] * Z + mvp[15];
            const float x_ss = (c0 / c3 + 1.0f) * hw;                               // divide by w + viewport (:156-174)
            const float y_ss = height - (c1 / c3 + 1.0f) * hh;
            out.at<float>(0, k) = (x_ss - hw) / focal;                              // :232
            out.at<float>(0, K + k) = (y_ss - hh) / focal;
        }
        return out;
    }

    int num_points() const { return (int)(points.size() / 3); }
    const std::vector<float>& get_points() const { return points; }   // K x 3
    float get_focal_length() const { return focal; }
    float get_width() const { return width; }
    float get_height() const { return height; }
    float get_near() const { return near_plane; }
    float get_far() const { return far_plane; }

private:
    static void mul4(const float* a, const float* b, float* c)
    {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                c[i * 4 + j] = a[i * 4 + 0] * b[0 * 4 + j] + a[i * 4 + 1] * b[1 * 4 + j] + a[i * 4 + 2] * b[2 * 4 + j] + a[i * 4 + 3] * b[3 * 4 + j];
    }

    std::vector<float> points;
    float focal, width, height, near_plane, far_plane;
    float projection[16];
};

namespace detail {

template <class Solver>
struct is_lu_solver : std::integral_constant<bool, std::is_same<Solver, PartialPivLUSolver>::value ||
                                                       std::is_same<Solver, VerbosePartialPivLUSolver>::value> {};

/** ModelProjection + LinearRegressor<LU family> + NoNormalisation on the device (include/sdm.h: sdm_pose_*). */
template <class Solver>
struct BatchedBackend<ModelProjection, LinearRegressor<Solver>, NoNormalisation, typename std::enable_if<is_lu_solver<Solver>::value>::type> {
    static constexpr bool available = true;
    using Regressors = std::vector<LinearRegressor<Solver>>;

    static cv::Mat contiguous(const cv::Mat& m) { return m.isContinuous() ? m : m.clone(); }

    static void bind(sdm_ctx* c, const ModelProjection& p, const cv::Mat& x0, const cv::Mat& templates, size_t n_levels)
    {
        if (n_levels < 1 || n_levels > 16) throw std::runtime_error("ModelProjection cascade: 1 ... 16 regressor levels");
        if (x0.cols != 6) throw std::runtime_error("ModelProjection cascade: parameters are rows of 6");
        if (templates.empty() || templates.rows != x0.rows)
            throw std::runtime_error("ModelProjection cascade: a known-template SDM, one template row per sample expected");
        hip::check(sdm_pose_set_model(c, p.get_points().data(), p.num_points(), p.get_focal_length(), p.get_width(), p.get_height(),
                                      p.get_near(), p.get_far()), "sdm_pose_set_model");
        hip::check(sdm_pose_set_x(c, x0.ptr<float>(0), x0.rows), "sdm_pose_set_x");
        cv::Mat t = contiguous(templates);
        hip::check(sdm_pose_set_templates(c, t.ptr<float>(0), t.rows, t.cols), "sdm_pose_set_templates");
    }

    static cv::Mat fetch_x(sdm_ctx* c, int rows)
    {
        cv::Mat x(rows, 6, CV_32FC1);
        hip::check(sdm_pose_get_x(c, x.ptr<float>(0)), "sdm_pose_get_x");
        return x;
    }

    /** superviseddescent.hpp:165-219 for every level: projection - templates, b = x - x*, normal equations, LU solve, update. */
    template <class Callback>
    static void train(Regressors& regressors, NoNormalisation&, cv::Mat parameters, cv::Mat initialisations, cv::Mat templates,
                      ModelProjection& projection, Callback on_training_epoch_callback)
    {
        hip::Handle h(hip::device());
        sdm_ctx* c = h.get();
        cv::Mat x0 = contiguous(initialisations), xs = contiguous(parameters);
        bind(c, projection, x0, templates, regressors.size());
        hip::check(sdm_pose_set_targets(c, xs.ptr<float>(0), xs.rows), "sdm_pose_set_targets");
        for (size_t level = 0; level < regressors.size(); ++level) {
            if (regressors[level].has_sweep()) throw std::invalid_argument("the pose cascade has no regulariser sweep");
            const Regulariser& r = regressors[level].get_regulariser();
            cv::Mat R(2 * projection.num_points(), 6, CV_32FC1);
            hip::check(sdm_pose_train_level(c, (int)level, r.type() == Regulariser::RegularisationType::MatrixNorm ? SDM_REG_MATRIX_NORM : SDM_REG_MANUAL,
                                            r.param(), r.regularises_last_row() ? 1 : 0, R.ptr<float>(0), nullptr),
                       "sdm_pose_train_level");
            regressors[level].x = R;
            on_training_epoch_callback(fetch_x(c, x0.rows));
        }
    }

    /** superviseddescent.hpp:262-306 / 323-344: all levels in one launch, or level by level around the callback (same bits). */
    template <class Callback>
    static cv::Mat test(Regressors& regressors, NoNormalisation&, cv::Mat initialisations, cv::Mat templates, ModelProjection& projection,
                        Callback on_regressor_iteration_callback)
    {
        hip::Handle h(hip::device());
        sdm_ctx* c = h.get();
        cv::Mat x0 = contiguous(initialisations);
        bind(c, projection, x0, templates, regressors.size());
        for (size_t level = 0; level < regressors.size(); ++level) {
            if (regressors[level].x.empty()) throw std::runtime_error("ModelProjection cascade: regressor level not learned");
            cv::Mat R = contiguous(regressors[level].x);
            hip::check(sdm_pose_set_regressor(c, (int)level, R.ptr<float>(0)), "sdm_pose_set_regressor");
        }
        if (is_no_eval(on_regressor_iteration_callback)) {                   // (test / predict without a callback)
            hip::check(sdm_pose_test(c, 0, (int)regressors.size()), "sdm_pose_test");
            return fetch_x(c, x0.rows);
        }
        for (size_t level = 0; level < regressors.size(); ++level) {
            hip::check(sdm_pose_test(c, (int)level, 1), "sdm_pose_test");
            on_regressor_iteration_callback(fetch_x(c, x0.rows));
        }
        return fetch_x(c, x0.rows);
    }

private:
    template <class Callback> static bool is_no_eval(const Callback&) { return false; }
    static bool is_no_eval(void (*const& f)(const cv::Mat&)) { return f == &no_eval; }
};

}  // namespace detail
}  // namespace superviseddescent

#endif /* SUPERVISEDDESCENT_MODEL_PROJECTION_HPP_ */
