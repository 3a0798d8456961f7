// sdm_capi_upright.hip -- C-ABI of upright-normalised detect and tracking (include/sdm.h, "Rolled faces"): the chip stack and the
// rows' records in sdm_ctx::upright, a detect call that cuts the chips, runs the cascade of sdm_detect_batch on them and maps the
// result back (csrc/sdm_upright.hip), and what the tracker's upright step (sdm_capi_track.hip) shares with it.  Every argument is
// checked before anything is launched.
#include "sdm_capi_internal.h"

#include <cmath>

namespace sdm_capi {

// (cos, sin) of a roll in degrees: a multiple of 90 gives exactly 0 / +-1
int upright_roll_cs(float roll_deg, double* cs)
{
    if (!std::isfinite(roll_deg)) return fail(SDM_ERR_INVALID, "a roll is not finite");
    const double d = (double)roll_deg, q = d / 90.0;
    if (q == std::floor(q)) {
        const int k = (int)std::fmod(std::fmod(q, 4.0) + 4.0, 4.0);
        static const double C[4] = {1.0, 0.0, -1.0, 0.0}, S[4] = {0.0, 1.0, 0.0, -1.0};
        cs[0] = C[k]; cs[1] = S[k];
    } else {
        const double a = d * 3.14159265358979323846 / 180.0;
        cs[0] = std::cos(a); cs[1] = std::sin(a);
    }
    return SDM_OK;
}

int upright_check(sdm_ctx* c, int n)
{
    if (c->upright.chip < 1) return fail(SDM_ERR_INVALID, "upright chips not configured (sdm_upright_configure)");
    if (c->L <= 0 || c->levels.empty()) return fail(SDM_ERR_INVALID, "geometry not set");
    if (n < 1) return fail(SDM_ERR_INVALID, "no rows (n >= 1)");
    for (size_t l = 0; l < c->levels.size(); ++l) {
        if (!c->have_R[l]) return fail(SDM_ERR_INVALID, "no regressor set for level " + std::to_string(l));
        if (c->levels[l].fixed_h == 0 && (c->eyes.nre <= 0 || c->eyes.nle <= 0))
            return fail(SDM_ERR_INVALID, "HOG features need eye landmark indices (IED-adaptive patch size)");
    }
    if (c->tmpl_N > 0) return fail(SDM_ERR_INVALID, "templates are set: the upright path runs the cascade without (sdm_set_templates(NULL))");
    if (!c->img_base || c->n_images < 1) return fail(SDM_ERR_INVALID, "no images set");
    if (c->idx_identity && n > c->n_images) return fail(SDM_ERR_INVALID, "more rows than images and no sample->image index set");
    if (!c->idx_identity && n > c->n_idx) return fail(SDM_ERR_INVALID, "sample->image index is shorter than the rows");
    if (!c->idx_identity && c->max_idx >= c->n_images)
        return fail(SDM_ERR_INVALID, "sample->image index refers to an image beyond the current image set");
    return SDM_OK;
}

int upright_ensure(sdm_ctx* c, int n)
{
    sdm_ctx::Upright& u = c->upright;
    const size_t chip_bytes = (size_t)sdm_upright_chip_stride(u.chip) * u.chip;
    int rc;
    if ((rc = ensure_sample_buffers(c, n)) || (rc = u.chips.ensure((size_t)n * chip_bytes)) || (rc = u.off.ensure(n)) || (rc = u.w.ensure(n)) ||
        (rc = u.h.ensure(n)) || (rc = u.stride.ensure(n)) || (rc = u.rows.ensure(n)))
        return rc;
    return SDM_OK;
}

// behind the set-up launch (records, chip table, x = the init in chip coordinates): the chips, the cascade on them, the back-map
int upright_run(sdm_ctx* c, int n)
{
    sdm_ctx::Upright& u = c->upright;
    sdm_launch_upright_chips(c->img_base, u.rows.p, n, u.chip, u.chips.p, c->stream);
    HIP_TRY(hipGetLastError());
    u.N = n;
    u.active = true;
    c->chain_timers = true; c->ev_fresh = false;
    int rc = SDM_OK;
    for (int l = 0; l < (int)c->levels.size() && !rc; ++l) rc = detect_level(c, l);
    c->chain_timers = false; c->ev_fresh = false;
    u.active = false;
    if (rc) return rc;
    sdm_launch_upright_back(u.rows.p, n, c->L, u.chip, u.guard, c->x[c->cur].p, c->stream);
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

}  // namespace sdm_capi

extern "C" {

int sdm_upright_configure(sdm_ctx* c, int chip, int guard)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (chip < 32 || chip > 1024) return fail(SDM_ERR_INVALID, "chip must be in [32, 1024]");
    if (guard < 0 || guard >= chip / 2) return fail(SDM_ERR_INVALID, "guard must be in [0, chip / 2)");
    if (chip != c->upright.chip) c->upright.N = 0;        // (the records and chips of the last call were laid out for the other size)
    c->upright.chip = chip; c->upright.guard = guard;
    return SDM_OK;
}

int sdm_detect_batch_upright(sdm_ctx* c, const float* mean, const int* boxes, const float* roll_deg, int n, float* x_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = upright_check(c, n))) return rc;
    if (!mean || !boxes || !roll_deg) return fail(SDM_ERR_INVALID, "no mean, boxes or rolls");
    const int M = c->M;
    // one staging block: n (cos, sin) pairs, n boxes, the mean
    const size_t words = (size_t)2 * n + ((size_t)4 * n * sizeof(int) + (size_t)M * sizeof(float) + sizeof(double) - 1) / sizeof(double);
    std::vector<double> in(words);
    for (int i = 0; i < n; ++i) {
        if (boxes[4 * i + 2] <= 0 || boxes[4 * i + 3] <= 0) return fail(SDM_ERR_INVALID, "a face box needs width and height > 0");
        if ((rc = upright_roll_cs(roll_deg[i], &in[(size_t)2 * i]))) return rc;
    }
    int* in_box = (int*)(in.data() + (size_t)2 * n);
    float* in_mean = (float*)(in_box + (size_t)4 * n);
    memcpy(in_box, boxes, (size_t)4 * n * sizeof(int));
    memcpy(in_mean, mean, (size_t)M * sizeof(float));
    HIP_TRY(hipSetDevice(c->device));
    sdm_ctx::Upright& u = c->upright;
    if ((rc = upright_ensure(c, n)) || (rc = u.in.ensure(words))) return rc;
    if (n != c->N) { c->have_targets = false; c->feat_level = -1; c->have_patch_idx = false; }
    c->N = n; c->cur = 0;
    HIP_TRY(hipMemcpyAsync(u.in.p, in.data(), words * sizeof(double), hipMemcpyHostToDevice, c->stream));
    UprightSetupDev a{};
    a.cs = u.in.p;
    a.boxes = (const int*)(u.in.p + (size_t)2 * n);
    a.mean = (const float*)(a.boxes + (size_t)4 * n);
    sdm_launch_upright_setup(a, n, c->L, u.chip, frame_set(c), c->idx_identity ? nullptr : c->img_idx.p, c->eyes, u.rows.p, u.off.p, u.w.p,
                             u.h.p, u.stride.p, c->x[0].p, nullptr, c->stream);
    HIP_TRY(hipGetLastError());
    if ((rc = upright_run(c, n))) return rc;
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, c->status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (x_host) HIP_TRY(hipMemcpyAsync(x_host, c->x[c->cur].p, (size_t)n * M * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (st) {
        HIP_TRY(hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream));
        if (st & SDM_DEV_ERR_EMPTY_PATCH)
            return fail(SDM_ERR_EMPTY_PATCH, "patch_width_half <= 0 for at least one row (inter-eye distance too small)");
        return fail(SDM_ERR_HIP, "a kernel reported status " + std::to_string(st));
    }
    return SDM_OK;
}

int sdm_upright_get(sdm_ctx* c, float* matrices_host, int* flags_host, uint8_t* chips_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    sdm_ctx::Upright& u = c->upright;
    if (u.N < 1) return fail(SDM_ERR_INVALID, "no upright call to report");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<UprightRow> rows;
    if (matrices_host || flags_host) {
        rows.resize(u.N);
        HIP_TRY(hipMemcpyAsync(rows.data(), u.rows.p, (size_t)u.N * sizeof(UprightRow), hipMemcpyDeviceToHost, c->stream));
    }
    if (chips_host)      // (the chips follow each other at one row pitch)
        HIP_TRY(hipMemcpy2DAsync(chips_host, (size_t)u.chip, u.chips.p, (size_t)sdm_upright_chip_stride(u.chip), (size_t)u.chip,
                                 (size_t)u.N * u.chip, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int r = 0; r < (int)rows.size(); ++r) {
        if (matrices_host) memcpy(matrices_host + (size_t)6 * r, rows[r].m, 6 * sizeof(float));
        if (flags_host) flags_host[r] = rows[r].flags;
    }
    return SDM_OK;
}

int sdm_track_configure_upright(sdm_ctx* c, int enable)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    sdm_ctx::Track& t = c->track;
    if (!enable) { t.upright = false; return SDM_OK; }
    if (t.S < 1) return fail(SDM_ERR_INVALID, "tracker not configured (sdm_track_configure)");
    if (c->L != t.L) return fail(SDM_ERR_INVALID, "the geometry's landmark count changed since sdm_track_configure");
    if (c->upright.chip < 1) return fail(SDM_ERR_INVALID, "upright chips not configured (sdm_upright_configure)");
    if (c->eyes.nre <= 0 || c->eyes.nle <= 0) return fail(SDM_ERR_INVALID, "upright tracking needs both eye landmark index sets");
    HIP_TRY(hipSetDevice(c->device));
    int rc = t.cs.ensure((size_t)2 * t.S);
    if (rc) return rc;
    std::vector<double> one((size_t)2 * t.S, 0.0);
    for (int i = 0; i < t.S; ++i) one[(size_t)2 * i] = 1.0;                  // every slot: roll 0
    HIP_TRY(hipMemcpyAsync(t.cs.p, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    t.upright = true;
    return SDM_OK;
}

}  // extern "C"
