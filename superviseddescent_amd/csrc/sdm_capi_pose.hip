// sdm_capi_pose.hip -- C-ABI of the head-pose cascade (include/sdm.h, sdm_pose_*): the ModelProjection + known-template
// SupervisedDescentOptimiser of the reference's examples/pose_estimation.cpp on the device.  The state lives in sdm_ctx::pose,
// beside the landmark state, so that sdm_pose_templates_from_landmarks can take a detect batch's landmarks from HBM.
#include "sdm_capi_internal.h"

#include <cmath>

namespace {

int pose_ready(sdm_ctx* c)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->pose.cam.K <= 0) return fail(SDM_ERR_INVALID, "pose model not set (sdm_pose_set_model)");
    HIP_TRY(hipSetDevice(c->device));
    return SDM_OK;
}

int pose_F(const sdm_ctx* c) { return 2 * c->pose.cam.K; }

int pose_set_x_common(sdm_ctx* c, const float* x, int N, hipMemcpyKind kind)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (!x || N < 1) return fail(SDM_ERR_INVALID, "bad pose parameters (N x 6, N >= 1)");
    if ((rc = c->pose.x.ensure((size_t)N * 6))) return rc;
    if (N != c->pose.N) c->pose.have_targets = false;
    c->pose.N = N;
    HIP_TRY(hipMemcpyAsync(c->pose.x.p, x, (size_t)N * 6 * sizeof(float), kind, c->stream));
    if (kind == hipMemcpyHostToDevice) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int pose_check_run(sdm_ctx* c, int first_level, int n_levels)
{
    const sdm_ctx::Pose& p = c->pose;
    if (p.N < 1) return fail(SDM_ERR_INVALID, "pose parameters not set (sdm_pose_set_x)");
    if (p.tmpl_N != p.N) return fail(SDM_ERR_INVALID, "pose templates not set for the current rows (N x 2K)");
    if (first_level < 0 || n_levels < 1 || first_level + n_levels > SDM_POSE_MAX_LEVELS)
        return fail(SDM_ERR_INVALID, "pose levels out of range (1 <= levels <= 16)");
    for (int l = first_level; l < first_level + n_levels; ++l)
        if (!(p.have_R >> l & 1u)) return fail(SDM_ERR_INVALID, "pose regressor of level " + std::to_string(l) + " not set");
    return SDM_OK;
}

}  // namespace

int sdm_pose_set_model(sdm_ctx* c, const float* points, int K, float focal, float width, float height, float near_, float far_)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (!points || K < 1 || K > SDM_POSE_MAX_K) return fail(SDM_ERR_INVALID, "pose model: 1 <= K <= 64 points expected");
    if (!(focal > 0.f) || !(width > 0.f) || !(height > 0.f) || !(far_ != near_)) return fail(SDM_ERR_INVALID, "pose model: bad camera");
    HIP_TRY(hipSetDevice(c->device));
    sdm_ctx::Pose& p = c->pose;
    int rc;
    if ((rc = p.pts.ensure((size_t)K * 3)) || (rc = p.R.ensure((size_t)SDM_POSE_MAX_LEVELS * 2 * K * 6))) return rc;
    if (K != p.cam.K) { p.have_R = 0; p.tmpl_N = 0; }
    // the projection matrix as the reference builds it, in float: focalLengthToFovy (:46) + createPerspectiveProjectionMatrix (:142-154)
    const float fovy = (2.0f * std::atan2(height, 2.0f * focal)) * (float)(180 / 3.14159265358979323846);
    const float radians = (fovy / 2.0f) * (float)3.14159265358979323846 / 180.0f;
    const float cotan = std::cos(radians) / std::sin(radians);
    const float aspect = width / height;
    PoseCamDev cam{};
    const float P[16] = {cotan / aspect, 0.f, 0.f, 0.f, 0.f, cotan, 0.f, 0.f, 0.f, 0.f, -(near_ + far_) / (far_ - near_),
                         (-2.0f * near_ * far_) / (far_ - near_), 0.f, 0.f, -1.0f, 0.f};
    memcpy(cam.P, P, sizeof(P));
    cam.f = focal; cam.W = width; cam.H = height; cam.K = K;
    p.cam = cam;
    HIP_TRY(hipMemcpyAsync(p.pts.p, points, (size_t)K * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_pose_set_x(sdm_ctx* c, const float* x_host, int n_samples) { return pose_set_x_common(c, x_host, n_samples, hipMemcpyHostToDevice); }
int sdm_pose_set_x_device(sdm_ctx* c, const float* x_dev, int n_samples) { return pose_set_x_common(c, x_dev, n_samples, hipMemcpyDeviceToDevice); }

int sdm_pose_get_x(sdm_ctx* c, float* x_host)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (!x_host || c->pose.N < 1) return fail(SDM_ERR_INVALID, "pose parameters not set");
    HIP_TRY(hipMemcpyAsync(x_host, c->pose.x.p, (size_t)c->pose.N * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_pose_set_templates(sdm_ctx* c, const float* templates, int n_samples, int feature_dim)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (!templates || n_samples < 1 || feature_dim != pose_F(c)) return fail(SDM_ERR_INVALID, "pose templates must be N x 2K");
    if ((rc = c->pose.tmpl.ensure((size_t)n_samples * feature_dim))) return rc;
    HIP_TRY(hipMemcpyAsync(c->pose.tmpl.p, templates, (size_t)n_samples * feature_dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pose.tmpl_N = n_samples;
    return SDM_OK;
}

int sdm_pose_templates_from_landmarks(sdm_ctx* c, const int* landmark_index, int K, float focal)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (!landmark_index || K != c->pose.cam.K) return fail(SDM_ERR_INVALID, "the landmark index map must name one landmark per model point");
    if (!(focal > 0.f)) return fail(SDM_ERR_INVALID, "focal length must be positive");
    if (c->L <= 0 || c->N < 1) return fail(SDM_ERR_INVALID, "no landmark rows (set the geometry and x, or run a detect batch)");
    if (c->n_images < 1) return fail(SDM_ERR_INVALID, "no images: the gather normalises by each row's image centre");
    if ((rc = check_sample_index(c))) return rc;
    for (int k = 0; k < K; ++k)
        if (landmark_index[k] < 0 || landmark_index[k] >= c->L) return fail(SDM_ERR_INVALID, "landmark index out of range");
    sdm_ctx::Pose& p = c->pose;
    if ((rc = p.lm.ensure((size_t)K)) || (rc = p.tmpl.ensure((size_t)c->N * 2 * K))) return rc;
    HIP_TRY(hipMemcpyAsync(p.lm.p, landmark_index, (size_t)K * sizeof(int), hipMemcpyHostToDevice, c->stream));
    sdm_launch_pose_gather(c->x[c->cur].p, c->L, c->N, p.lm.p, K, c->idx_identity ? nullptr : c->img_idx.p, c->img_w.p, c->img_h.p, focal,
                           p.tmpl.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));     // (the host index map may go away)
    p.tmpl_N = c->N;
    return SDM_OK;
}

int sdm_pose_set_targets(sdm_ctx* c, const float* xstar_host, int n_samples)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (!xstar_host || n_samples != c->pose.N) return fail(SDM_ERR_INVALID, "pose targets must be N x 6 for the current rows");
    if ((rc = c->pose.xstar.ensure((size_t)n_samples * 6))) return rc;
    HIP_TRY(hipMemcpyAsync(c->pose.xstar.p, xstar_host, (size_t)n_samples * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pose.have_targets = true;
    return SDM_OK;
}

int sdm_pose_features(sdm_ctx* c, int level, float* out_host)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    sdm_ctx::Pose& p = c->pose;
    if (level < 0 || level >= SDM_POSE_MAX_LEVELS || !out_host || p.N < 1) return fail(SDM_ERR_INVALID, "bad pose feature request");
    const int F = pose_F(c);
    if ((rc = p.Ab.ensure((size_t)p.N * F))) return rc;
    // (the projection does not depend on the level, pose_estimation.cpp:205; templates are subtracted when set for these rows)
    sdm_launch_pose_project(p.x.p, nullptr, p.tmpl_N == p.N ? p.tmpl.p : nullptr, p.pts.p, p.cam, p.N, p.Ab.p, F, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, p.Ab.p, (size_t)p.N * F * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_pose_set_regressor(sdm_ctx* c, int level, const float* R_host)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (level < 0 || level >= SDM_POSE_MAX_LEVELS || !R_host) return fail(SDM_ERR_INVALID, "pose level out of range (0..15)");
    const size_t n = (size_t)pose_F(c) * 6;
    HIP_TRY(hipMemcpyAsync(c->pose.R.p + (size_t)level * n, R_host, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pose.have_R |= 1u << level;
    return SDM_OK;
}

int sdm_pose_get_regressor(sdm_ctx* c, int level, float* R_host)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if (level < 0 || level >= SDM_POSE_MAX_LEVELS || !R_host || !(c->pose.have_R >> level & 1u))
        return fail(SDM_ERR_INVALID, "pose level has no regressor");
    const size_t n = (size_t)pose_F(c) * 6;
    HIP_TRY(hipMemcpyAsync(R_host, c->pose.R.p + (size_t)level * n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_pose_test(sdm_ctx* c, int first_level, int n_levels)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    if ((rc = pose_check_run(c, first_level, n_levels))) return rc;
    sdm_ctx::Pose& p = c->pose;
    sdm_launch_pose_cascade(p.x.p, p.tmpl.p, p.R.p + (size_t)first_level * pose_F(c) * 6, p.pts.p, p.cam, p.N, n_levels, c->stream);
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

int sdm_pose_train_level(sdm_ctx* c, int level, int reg_type, float reg_param, int regularise_last_row, float* R_host, float* lambda_out)
{
    int rc = pose_ready(c);
    if (rc) return rc;
    sdm_ctx::Pose& p = c->pose;
    if (level < 0 || level >= SDM_POSE_MAX_LEVELS) return fail(SDM_ERR_INVALID, "pose level out of range (0..15)");
    if (reg_type != SDM_REG_MANUAL && reg_type != SDM_REG_MATRIX_NORM) return fail(SDM_ERR_INVALID, "unknown regularisation type");
    if (p.N < 1 || !p.have_targets) return fail(SDM_ERR_INVALID, "pose parameters / targets not set");
    if (p.tmpl_N != p.N) return fail(SDM_ERR_INVALID, "pose templates not set for the current rows (N x 2K)");
    const int F = pose_F(c), T = F + 6, npairs = T * (T + 1) / 2;
    if ((rc = p.Ab.ensure((size_t)p.N * T)) || (rc = p.partial.ensure((size_t)sdm_pose_gram_blocks(p.N) * npairs)) ||
        (rc = p.G.ensure((size_t)npairs)) || (rc = c->lambda_dev.ensure(1)))
        return rc;
    float* Rl = p.R.p + (size_t)level * F * 6;
    // superviseddescent.hpp:170-218 for one level: projection (- templates) and b = x - x* ...
    sdm_launch_pose_project(p.x.p, p.xstar.p, p.tmpl.p, p.pts.p, p.cam, p.N, p.Ab.p, T, c->stream);
    // ... LinearRegressor::learn -> PartialPivLUSolver::solve (regressors.hpp:199-234, 345-350) ...
    sdm_launch_pose_gram(p.Ab.p, p.N, T, p.partial.p, p.G.p, c->stream);
    sdm_launch_pose_solve(p.G.p, F, T, reg_type, reg_param, p.N, regularise_last_row, Rl, c->lambda_dev.p, c->stream);
    // ... and the update of the training rows (:209-216), through the test launch: the same bits as sdm_pose_test of this level
    sdm_launch_pose_cascade(p.x.p, p.tmpl.p, Rl, p.pts.p, p.cam, p.N, 1, c->stream);
    HIP_TRY(hipGetLastError());
    p.have_R |= 1u << level;
    if (R_host) HIP_TRY(hipMemcpyAsync(R_host, Rl, (size_t)F * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (lambda_out) HIP_TRY(hipMemcpyAsync(lambda_out, c->lambda_dev.p, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}
