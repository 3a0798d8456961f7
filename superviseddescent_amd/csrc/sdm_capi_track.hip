// sdm_capi_track.hip -- C-ABI of multi-stream face tracking (include/sdm.h, sdm_track_*): a table of stream slots in sdm_ctx::track,
// and a step that gathers n slots into the landmark state x, runs the detect cascade of sdm_detect_batch on them, and commits the
// results back with the lost decision (csrc/sdm_track.hip).  Every argument is checked before anything is launched.
#include "sdm_capi_internal.h"

#include <algorithm>
#include <cmath>

namespace {

int track_ready(sdm_ctx* c)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->track.S < 1) return fail(SDM_ERR_INVALID, "tracker not configured (sdm_track_configure)");
    if (c->L != c->track.L) return fail(SDM_ERR_INVALID, "the geometry's landmark count changed since sdm_track_configure");
    return SDM_OK;
}

// ids in [0, S), none twice within the call
int check_ids(sdm_ctx* c, const int* ids, int n)
{
    sdm_ctx::Track& t = c->track;
    if (!ids || n < 1) return fail(SDM_ERR_INVALID, "no stream ids (n >= 1)");
    if (++t.stamp == 0) { std::fill(t.seen.begin(), t.seen.end(), 0u); t.stamp = 1; }
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= t.S) return fail(SDM_ERR_INVALID, "stream id " + std::to_string(ids[i]) + " out of range");
        if (t.seen[ids[i]] == t.stamp) return fail(SDM_ERR_INVALID, "stream id " + std::to_string(ids[i]) + " named twice in one call");
        t.seen[ids[i]] = t.stamp;
    }
    return SDM_OK;
}

int ensure_pinned(sdm_ctx::Track& t, size_t n_ints)
{
    if (n_ints <= t.pin_cap) return SDM_OK;
    if (t.pin) { HIP_TRY(hipHostFree(t.pin)); t.pin = nullptr; t.pin_cap = 0; }
    HIP_TRY(hipHostMalloc((void**)&t.pin, n_ints * sizeof(int), hipHostMallocDefault));
    t.pin_cap = n_ints;
    return SDM_OK;
}

}  // namespace

extern "C" {

int sdm_track_configure(sdm_ctx* c, int capacity, const float* mean, int init_mode, float min_size, float max_scale_change)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    if (capacity < 1) return fail(SDM_ERR_INVALID, "capacity must be >= 1");
    if (!mean) return fail(SDM_ERR_INVALID, "no mean shape");
    if (init_mode != SDM_TRACK_INIT_PREVIOUS && init_mode != SDM_TRACK_INIT_REALIGN) return fail(SDM_ERR_INVALID, "unknown init mode");
    if (!(min_size >= 0.f) || !std::isfinite(min_size)) return fail(SDM_ERR_INVALID, "min_size must be finite and >= 0");
    if (!(max_scale_change >= 0.f) || !std::isfinite(max_scale_change)) return fail(SDM_ERR_INVALID, "max_scale_change must be finite and >= 0");
    const int L = c->L, M = 2 * L;
    float mb[4] = {mean[0], mean[0], mean[L], mean[L]};
    for (int j = 0; j < L; ++j) {
        if (!std::isfinite(mean[j]) || !std::isfinite(mean[L + j])) return fail(SDM_ERR_INVALID, "the mean shape is not finite");
        mb[0] = std::min(mb[0], mean[j]); mb[1] = std::max(mb[1], mean[j]);
        mb[2] = std::min(mb[2], mean[L + j]); mb[3] = std::max(mb[3], mean[L + j]);
    }
    if (!(mb[1] - mb[0] > 0.f) || !(mb[3] - mb[2] > 0.f)) return fail(SDM_ERR_INVALID, "the mean shape has no width or no height");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    sdm_ctx::Track& t = c->track;
    t.filter_off();                                // (the filter's state belongs to the slots that go: sdm_track_configure_filter again)
    t.motion_off();                                // (and the motion state: sdm_track_configure_motion again)
    int rc;
    if ((rc = t.mean.ensure(M)) || (rc = t.x.ensure((size_t)capacity * M)) || (rc = t.box.ensure((size_t)capacity * 4)) ||
        (rc = t.status.ensure((size_t)capacity)))
        return rc;
    HIP_TRY(hipMemcpyAsync(t.mean.p, mean, M * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(t.x.p, 0, (size_t)capacity * M * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(t.box.p, 0, (size_t)capacity * 4 * sizeof(int), c->stream));
    HIP_TRY(hipMemsetAsync(t.status.p, 0, (size_t)capacity * sizeof(int), c->stream));     // SDM_TRACK_FREE
    HIP_TRY(hipStreamSynchronize(c->stream));
    t.S = capacity; t.L = L; t.mode = init_mode; t.min_size = min_size; t.max_scale = max_scale_change;
    memcpy(t.mean_bounds, mb, sizeof(mb));
    t.host_status.assign(capacity, SDM_TRACK_FREE);
    t.seen.assign(capacity, 0u); t.stamp = 0;
    return SDM_OK;
}

// sdm_track_start (roll_deg null) and sdm_track_start_rolled: with the upright mode's per-slot (cos, sin) allocated every start writes
// the slot's pair as well -- (1, 0) without a roll
static int track_start_common(sdm_ctx* c, const int* ids, const int* boxes, const float* roll_deg, int n)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (roll_deg && !t.upright) return fail(SDM_ERR_INVALID, "a rolled start needs upright mode (sdm_track_configure_upright)");
    if (t.upright && t.cs.cap < (size_t)2 * t.S)
        return fail(SDM_ERR_INVALID, "the tracker was configured again: call sdm_track_configure_upright again");
    if ((rc = check_ids(c, ids, n))) return rc;
    if (!boxes) return fail(SDM_ERR_INVALID, "no face boxes");
    for (int i = 0; i < n; ++i)
        if (boxes[4 * i + 2] <= 0 || boxes[4 * i + 3] <= 0) return fail(SDM_ERR_INVALID, "a face box needs width and height > 0");
    std::vector<double> cs;
    if (roll_deg) {
        cs.resize((size_t)2 * n);
        for (int i = 0; i < n; ++i)
            if ((rc = upright_roll_cs(roll_deg[i], &cs[(size_t)2 * i]))) return rc;
    }
    const bool slots_cs = t.cs.cap >= (size_t)2 * t.S;
    // staging: (cos, sin) pairs first (8-byte aligned), then the ids and the boxes
    const size_t cs_ints = roll_deg ? (size_t)4 * n : 0;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_pinned(t, cs_ints + (size_t)5 * n)) || (rc = t.ids.ensure(cs_ints + (size_t)5 * n + 1))) return rc;
    if (roll_deg) memcpy(t.pin, cs.data(), cs_ints * sizeof(int));
    memcpy(t.pin + cs_ints, ids, (size_t)n * sizeof(int));
    memcpy(t.pin + cs_ints + n, boxes, (size_t)4 * n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(t.ids.p, t.pin, (cs_ints + (size_t)5 * n) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    sdm_launch_track_start(t.ids.p + cs_ints, t.ids.p + cs_ints + n, n, t.box.p, t.status.p, c->stream);
    if (t.filter) sdm_launch_track_filter_unprime(t.ids.p + cs_ints, n, t.primed.p, c->stream);
    if (t.motion) sdm_launch_track_motion_invalidate(t.ids.p + cs_ints, n, t.motion_state.p, c->stream);
    if (slots_cs) sdm_launch_upright_slot_cs(t.ids.p + cs_ints, roll_deg ? (const double*)t.ids.p : nullptr, n, t.cs.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the pinned staging is reused by the next call)
    for (int i = 0; i < n; ++i) t.host_status[ids[i]] = SDM_TRACK_STARTED;
    return SDM_OK;
}

int sdm_track_start(sdm_ctx* c, const int* ids, const int* boxes, int n) { return track_start_common(c, ids, boxes, nullptr, n); }

int sdm_track_start_rolled(sdm_ctx* c, const int* ids, const int* boxes, const float* roll_deg, int n)
{
    if (!roll_deg) return fail(SDM_ERR_INVALID, "no rolls");
    return track_start_common(c, ids, boxes, roll_deg, n);
}

int sdm_track_stop(sdm_ctx* c, const int* ids, int n)
{
    int rc = track_ready(c);
    if (rc) return rc;
    if ((rc = check_ids(c, ids, n))) return rc;
    for (int i = 0; i < n; ++i) c->track.host_status[ids[i]] = SDM_TRACK_FREE;
    return SDM_OK;
}

// sdm_track_step (dt null) and sdm_track_step_filtered: the same checks, copies and launches; with dt the filter launch behind the
// commit, the raw rows copied out before it and the filtered rows after it
static int track_step_common(sdm_ctx* c, const int* ids, int n, const float* dt, float* landmarks_host, int* lost_host, float* filtered_host)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (dt && t.filter == SDM_TRACK_FILTER_OFF) return fail(SDM_ERR_INVALID, "no filter configured (sdm_track_configure_filter)");
    if (c->levels.empty()) return fail(SDM_ERR_INVALID, "geometry not set");
    for (size_t l = 0; l < c->levels.size(); ++l)
        if (!c->have_R[l]) return fail(SDM_ERR_INVALID, "no regressor set for level " + std::to_string(l));
    if ((rc = check_ids(c, ids, n))) return rc;
    for (int i = 0; i < n; ++i) {
        const int st = t.host_status[ids[i]];
        if (st == SDM_TRACK_FREE) return fail(SDM_ERR_INVALID, "stream " + std::to_string(ids[i]) + " is not started");
        if (st == SDM_TRACK_LOST) return fail(SDM_ERR_INVALID, "stream " + std::to_string(ids[i]) + " is lost: start it again from a face box");
    }
    for (int i = 0; dt && i < n; ++i)
        if (!(dt[i] >= 1e-4f && dt[i] <= 1e4f)) return fail(SDM_ERR_INVALID, "a step time outside [1e-4, 1e4] seconds");
    if (c->tmpl_N > 0) return fail(SDM_ERR_INVALID, "templates are set: the tracker runs the cascade without (sdm_set_templates(NULL))");
    if (t.upright) {
        if (t.cs.cap < (size_t)2 * t.S) return fail(SDM_ERR_INVALID, "the tracker was configured again: call sdm_track_configure_upright again");
        if (c->eyes.nre <= 0 || c->eyes.nle <= 0) return fail(SDM_ERR_INVALID, "upright tracking needs both eye landmark index sets");
        if ((rc = upright_check(c, n))) return rc;
    }
    if (!c->img_base || c->n_images < 1) return fail(SDM_ERR_INVALID, "no images set");
    if (c->idx_identity && n > c->n_images) return fail(SDM_ERR_INVALID, "more rows than images and no sample->image index set");
    if (!c->idx_identity && n > c->n_idx) return fail(SDM_ERR_INVALID, "sample->image index is shorter than the step's rows");
    if (!c->idx_identity && c->max_idx >= c->n_images)
        return fail(SDM_ERR_INVALID, "sample->image index refers to an image beyond the current image set");
    HIP_TRY(hipSetDevice(c->device));
    const int M = c->M;
    // staging: the ids and, for a filtered step, the step times behind them go to the device in one copy; the masks come back
    const size_t in_ints = dt ? (size_t)2 * n : (size_t)n;
    if ((rc = ensure_sample_buffers(c, n)) || (rc = t.init.ensure((size_t)n * M)) || (rc = t.ids.ensure(in_ints)) ||
        (rc = t.masks.ensure((size_t)n + 1)) || (rc = ensure_pinned(t, in_ints + n + 1)))
        return rc;
    if (t.upright && (rc = upright_ensure(c, n))) return rc;
    if (t.motion && (rc = t.motion_shift.ensure((size_t)2 * n))) return rc;
    // the rows become the current x, as after sdm_set_x + sdm_detect_batch
    if (n != c->N) { c->have_targets = false; c->feat_level = -1; c->have_patch_idx = false; }
    c->N = n; c->cur = 0;
    memcpy(t.pin, ids, (size_t)n * sizeof(int));
    if (dt) memcpy(t.pin + n, dt, (size_t)n * sizeof(float));
    HIP_TRY(hipMemcpyAsync(t.ids.p, t.pin, in_ints * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int* row_image = c->idx_identity ? nullptr : c->img_idx.p;
    const float* shift = nullptr;
    if (t.motion) {
        // the translation of every tracked row's face between its slot's chip and the new image, ahead of the gather
        sdm_launch_track_motion_search(t.ids.p, n, t.status.p, t.motion_state.p, t.motion_chips.p, frame_set(c), row_image, t.motion_search,
                                       t.motion_min_gain, t.motion_shift.p, t.motion_last.p, c->stream);
        HIP_TRY(hipGetLastError());
        shift = t.motion_shift.p;
    }
    if (t.upright) {
        // upright mode: the rows' chips and their init in chip coordinates, the cascade on the chips, the result back in the frame
        UprightSetupDev a{};
        a.ids = t.ids.p; a.slot_status = t.status.p; a.slot_box = t.box.p; a.slot_cs = t.cs.p; a.slot_x = t.x.p; a.mean = t.mean.p;
        a.mb = make_float4(t.mean_bounds[0], t.mean_bounds[1], t.mean_bounds[2], t.mean_bounds[3]);
        a.shift = shift;
        sdm_ctx::Upright& u = c->upright;
        sdm_launch_upright_setup(a, n, c->L, u.chip, frame_set(c), row_image, c->eyes, u.rows.p, u.off.p,
                                 u.w.p, u.h.p, u.stride.p, c->x[0].p, t.init.p, c->stream);
        HIP_TRY(hipGetLastError());
        if ((rc = upright_run(c, n))) return rc;
    } else {
    sdm_launch_track_gather(t.ids.p, n, c->L, t.mode, t.status.p, t.box.p, t.x.p, t.mean.p, t.mean_bounds, c->x[0].p, t.init.p, c->stream,
                            shift);
    HIP_TRY(hipGetLastError());
    // the cascade: exactly sdm_detect_batch's level sequence (fused or unfused per level)
    c->chain_timers = true; c->ev_fresh = false;
    for (int l = 0; l < (int)c->levels.size() && !rc; ++l) rc = detect_level(c, l);
    c->chain_timers = false; c->ev_fresh = false;
    if (rc) return rc;
    }
    sdm_launch_track_commit(t.ids.p, n, c->L, c->x[c->cur].p, t.init.p, c->idx_identity ? nullptr : c->img_idx.p, c->img_w.p, c->img_h.p,
                            c->eyes, t.min_size, t.max_scale, t.x.p, t.status.p, t.masks.p, c->status.p, c->stream);
    HIP_TRY(hipGetLastError());
    if (t.motion) {
        // the tracked rows' grids and reference chips from the committed raw rows; a lost row's slot is invalidated
        sdm_launch_track_motion_store(t.ids.p, n, c->L, c->x[c->cur].p, t.masks.p, frame_set(c), row_image, t.motion_scale, t.motion_state.p,
                                      t.motion_chips.p, c->stream);
        HIP_TRY(hipGetLastError());
    }
    int* masks = t.pin + in_ints;
    HIP_TRY(hipMemcpyAsync(masks, t.masks.p, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (landmarks_host)
        HIP_TRY(hipMemcpyAsync(landmarks_host, c->x[c->cur].p, (size_t)n * M * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (dt) {
        // the current rows become the filtered rows; the slots' landmark rows stay raw
        const size_t SM = (size_t)t.S * M;
        sdm_launch_track_filter(t.ids.p, n, c->L, t.masks.p, (const float*)(t.ids.p + n), t.min_cutoff, t.beta, t.d_cutoff, c->x[c->cur].p,
                                t.filter_state.p, t.filter_state.p + SM, t.filter_state.p + 2 * SM, t.primed.p, c->stream);
        HIP_TRY(hipGetLastError());
        if (filtered_host)
            HIP_TRY(hipMemcpyAsync(filtered_host, c->x[c->cur].p, (size_t)n * M * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) t.host_status[ids[i]] = masks[i] ? SDM_TRACK_LOST : SDM_TRACK_TRACKED;
    if (lost_host) memcpy(lost_host, masks, (size_t)n * sizeof(int));
    const int st = masks[n];
    if (st) {
        HIP_TRY(hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream));
        if (st & SDM_DEV_ERR_EMPTY_PATCH)
            return fail(SDM_ERR_EMPTY_PATCH, "patch_width_half <= 0 for at least one row (inter-eye distance too small)");
        return fail(SDM_ERR_HIP, "a kernel reported status " + std::to_string(st));
    }
    return SDM_OK;
}

int sdm_track_step(sdm_ctx* c, const int* ids, int n, float* landmarks_host, int* lost_host)
{
    return track_step_common(c, ids, n, nullptr, landmarks_host, lost_host, nullptr);
}

int sdm_track_configure_filter(sdm_ctx* c, int mode, float min_cutoff_hz, float beta, float d_cutoff_hz)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (mode != SDM_TRACK_FILTER_OFF && mode != SDM_TRACK_FILTER_ONE_EURO) return fail(SDM_ERR_INVALID, "unknown filter mode");
    if (mode == SDM_TRACK_FILTER_ONE_EURO) {
        if (!std::isfinite(min_cutoff_hz) || !(min_cutoff_hz > 0.f)) return fail(SDM_ERR_INVALID, "min_cutoff must be finite and > 0");
        if (!std::isfinite(beta) || !(beta >= 0.f)) return fail(SDM_ERR_INVALID, "beta must be finite and >= 0");
        if (!std::isfinite(d_cutoff_hz) || !(d_cutoff_hz > 0.f)) return fail(SDM_ERR_INVALID, "d_cutoff must be finite and > 0");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (mode == SDM_TRACK_FILTER_OFF) { t.filter_off(); return SDM_OK; }
    const size_t SM = (size_t)t.S * 2 * t.L;
    if ((rc = t.filter_state.ensure(3 * SM)) || (rc = t.primed.ensure((size_t)t.S))) { t.filter_off(); return rc; }
    HIP_TRY(hipMemsetAsync(t.filter_state.p, 0, 3 * SM * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(t.primed.p, 0, (size_t)t.S * sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    t.filter = mode; t.min_cutoff = min_cutoff_hz; t.beta = beta; t.d_cutoff = d_cutoff_hz;
    return SDM_OK;
}

int sdm_track_step_filtered(sdm_ctx* c, const int* ids, int n, const float* dt_seconds, float* landmarks_host, int* lost_host,
                            float* filtered_host)
{
    if (!dt_seconds) return fail(SDM_ERR_INVALID, "no step times");
    return track_step_common(c, ids, n, dt_seconds, landmarks_host, lost_host, filtered_host);
}

int sdm_track_get_filtered(sdm_ctx* c, const int* ids, int n, float* filtered_host, float* derivative_host, int* primed_host)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (t.filter == SDM_TRACK_FILTER_OFF) return fail(SDM_ERR_INVALID, "no filter configured (sdm_track_configure_filter)");
    if ((rc = check_ids(c, ids, n))) return rc;
    if (!filtered_host && !derivative_host && !primed_host) return SDM_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nM = (size_t)n * c->M, SM = (size_t)t.S * c->M;
    if ((rc = t.filter_out.ensure(2 * nM + n)) || (rc = t.ids.ensure((size_t)n)) || (rc = ensure_pinned(t, (size_t)n))) return rc;
    memcpy(t.pin, ids, (size_t)n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(t.ids.p, t.pin, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    float* out_f = t.filter_out.p;
    float* out_d = out_f + nM;
    int* out_p = (int*)(out_d + nM);
    sdm_launch_track_filter_get(t.ids.p, n, c->L, t.filter_state.p + SM, t.filter_state.p + 2 * SM, t.primed.p, out_f, out_d, out_p, c->stream);
    HIP_TRY(hipGetLastError());
    if (filtered_host) HIP_TRY(hipMemcpyAsync(filtered_host, out_f, nM * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (derivative_host) HIP_TRY(hipMemcpyAsync(derivative_host, out_d, nM * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (primed_host) HIP_TRY(hipMemcpyAsync(primed_host, out_p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_track_configure_motion(sdm_ctx* c, int mode, int search, float scale, int min_gain)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (mode != SDM_TRACK_MOTION_OFF && mode != SDM_TRACK_MOTION_SAD) return fail(SDM_ERR_INVALID, "unknown motion mode");
    if (mode == SDM_TRACK_MOTION_SAD) {
        if (search < 1 || search > 16) return fail(SDM_ERR_INVALID, "search must lie in [1, 16] chip pixels");
        if (!std::isfinite(scale) || !(scale >= 0.5f && scale <= 4.f)) return fail(SDM_ERR_INVALID, "scale must be finite and lie in [0.5, 4]");
        if (min_gain < 0 || min_gain > 255) return fail(SDM_ERR_INVALID, "min_gain must lie in [0, 255]");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (mode == SDM_TRACK_MOTION_OFF) { t.motion_off(); return SDM_OK; }
    const size_t S = (size_t)t.S;
    if ((rc = t.motion_state.ensure(4 * S)) || (rc = t.motion_chips.ensure(1024 * S)) || (rc = t.motion_last.ensure(6 * S))) { t.motion_off(); return rc; }
    HIP_TRY(hipMemsetAsync(t.motion_state.p, 0, 4 * S * sizeof(int), c->stream));         // every slot invalid
    HIP_TRY(hipMemsetAsync(t.motion_chips.p, 0, 1024 * S, c->stream));
    HIP_TRY(hipMemsetAsync(t.motion_last.p, 0, 6 * S * sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    t.motion = mode; t.motion_search = search; t.motion_scale = scale; t.motion_min_gain = min_gain;
    return SDM_OK;
}

int sdm_track_get_motion(sdm_ctx* c, const int* ids, int n, int* motion_host, int* grid_host, uint8_t* chips_host)
{
    int rc = track_ready(c);
    if (rc) return rc;
    sdm_ctx::Track& t = c->track;
    if (t.motion == SDM_TRACK_MOTION_OFF) return fail(SDM_ERR_INVALID, "no motion mode configured (sdm_track_configure_motion)");
    if ((rc = check_ids(c, ids, n))) return rc;
    if (!motion_host && !grid_host && !chips_host) return SDM_OK;
    HIP_TRY(hipSetDevice(c->device));
    // scratch: n x 6 and n x 3 ints (9 n, padded to a multiple of 4 ints), then the n chips
    const size_t head = ((size_t)9 * n + 3) & ~(size_t)3;
    if ((rc = t.motion_out.ensure(head + (size_t)256 * n)) || (rc = t.ids.ensure((size_t)n)) || (rc = ensure_pinned(t, (size_t)n))) return rc;
    memcpy(t.pin, ids, (size_t)n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(t.ids.p, t.pin, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    int* out_m = t.motion_out.p;
    int* out_g = out_m + (size_t)6 * n;
    uint8_t* out_c = (uint8_t*)(t.motion_out.p + head);
    sdm_launch_track_motion_get(t.ids.p, n, t.motion_state.p, t.motion_chips.p, t.motion_last.p, out_m, out_g, out_c, c->stream);
    HIP_TRY(hipGetLastError());
    if (motion_host) HIP_TRY(hipMemcpyAsync(motion_host, out_m, (size_t)6 * n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (grid_host) HIP_TRY(hipMemcpyAsync(grid_host, out_g, (size_t)3 * n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (chips_host) HIP_TRY(hipMemcpyAsync(chips_host, out_c, (size_t)1024 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_track_get(sdm_ctx* c, const int* ids, int n, float* landmarks_host, int* status_host)
{
    int rc = track_ready(c);
    if (rc) return rc;
    if ((rc = check_ids(c, ids, n))) return rc;
    sdm_ctx::Track& t = c->track;
    if (landmarks_host) {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = t.init.ensure((size_t)n * c->M)) || (rc = t.ids.ensure((size_t)n)) || (rc = ensure_pinned(t, (size_t)n))) return rc;
        memcpy(t.pin, ids, (size_t)n * sizeof(int));
        HIP_TRY(hipMemcpyAsync(t.ids.p, t.pin, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        sdm_launch_track_gather(t.ids.p, n, c->L, SDM_TRACK_INIT_PREVIOUS, t.status.p, t.box.p, t.x.p, t.mean.p, t.mean_bounds, t.init.p,
                                nullptr, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(landmarks_host, t.init.p, (size_t)n * c->M * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (status_host)
        for (int i = 0; i < n; ++i) status_host[i] = t.host_status[ids[i]];
    return SDM_OK;
}

}  // extern "C"
