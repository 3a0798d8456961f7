// sdm_capi_detect.hip -- feature extraction, regressors, the update step, detect: the launch sequences of a cascade level (C-ABI of include/sdm.h; shared declarations: sdm_capi_internal.h)
#include "sdm_capi_internal.h"

namespace sdm_capi {

// the kernels' per-coordinate arithmetic (hog.c:697-704), IEEE on the host: {weight of band slot 0, of band slot 1, cell index, upper weight}
// (packed_row_const, sdm_kernels.h: the one definition, which the detect instances of the pixel kernel evaluate at compile time)
void fill_row_tab(HogLevelDev& lv)
{
    for (int d = 0; d < 64 && d < lv.S; ++d) {
        const HogRowConst rc = packed_row_const(d, lv.cell, lv.C);
        lv.row_tab[d][0] = rc.ws0;
        lv.row_tab[d][1] = rc.ws1;
        memcpy(&lv.row_tab[d][2], &rc.band, sizeof(int));
        lv.row_tab[d][3] = rc.w2;
    }
}



void drain_timing(sdm_ctx* c)
{
    for (auto& p : c->pending) {
        hipError_t e = hipEventSynchronize(p.b); (void)e;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { c->t_ms[p.slot] += ms; c->t_n[p.slot] += 1; }
        if (!p.a_shared) c->pool.push_back(p.a);
        c->pool.push_back(p.b);
    }
    c->pending.clear();
    c->ev_fresh = false;
}

int check_status(sdm_ctx* c)
{
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, c->status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (st) {
        HIP_TRY(hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream));
        if (st & SDM_DEV_ERR_EMPTY_PATCH)
            return fail(SDM_ERR_EMPTY_PATCH, "patch_width_half <= 0 for at least one sample (inter-eye distance too small)");
        if (st & 2) return fail(SDM_ERR_NOT_SPD, "regularised Gram matrix is not positive definite; increase lambda");
        if (st & 4) return fail(SDM_ERR_HIP, "back substitution: a tile row waited for its predecessor beyond the spin limit");
        if (st & 8) return fail(SDM_ERR_NOT_SPD, "Cholesky update: a factor entry exceeds the square root of the largest diagonal entry (matrix not positive definite?)");
    }
    return SDM_OK;
}

// feature row length: L patches + the bias of the adaptive transform (the non-adaptive example transform has none)

ImageSetDev frame_set(const sdm_ctx* c)
{
    ImageSetDev s;
    s.base = c->img_base; s.offset = c->img_off.p; s.w = c->img_w.p; s.h = c->img_h.p;
    s.stride = c->img_stride.p; s.n_images = c->n_images;
    return s;
}

// The images the cascade reads and the rows' index into them: the context's, or -- while an upright call is in flight
// (sdm_capi_upright.hip) -- the stack of chips, one per row.  With no such call every launch is what it was.
ImageSetDev image_set(const sdm_ctx* c)
{
    if (!c->upright.active) return frame_set(c);
    const sdm_ctx::Upright& u = c->upright;
    ImageSetDev s;
    s.base = u.chips.p; s.offset = u.off.p; s.w = u.w.p; s.h = u.h.p; s.stride = u.stride.p; s.n_images = u.N;
    return s;
}
const int* sample_index(const sdm_ctx* c) { return (c->upright.active || c->idx_identity) ? nullptr : c->img_idx.p; }
// (a chip is never one of the images the fused pixel kernels cannot serve)
static bool narrow_set(const sdm_ctx* c) { return !c->upright.active && c->narrow_images; }

int ensure_sample_buffers(sdm_ctx* c, int N)
{
    int rc;
    const size_t nx = (size_t)N * c->M;
    if ((rc = c->x[0].ensure(nx))) return rc;
    if ((rc = c->x[1].ensure(nx))) return rc;
    const size_t nf = (size_t)N * (size_t)c->ldf;
    if (nf > c->feat.cap) {
        // zero once: the padding columns must stay exactly 0 for the GEMMs that read full tiles
        if ((rc = c->feat.ensure(nf, true, c->stream))) return rc;
        c->feat_level = -1; c->feat_wide_F = 0; c->feat_wide_N = 0;
    }
    if ((rc = c->patch_idx.ensure((size_t)N * (1 + 2 * c->L)))) return rc;
    return SDM_OK;
}

// The kernels read img_idx[s] for every s < N and use it as an image number: both bounds are checked at every launch,
// because the index, the images and x may be set in any order.
int check_sample_index(const sdm_ctx* c)
{
    if (c->upright.active) return SDM_OK;      // (one chip per row, identity index)
    if (c->idx_identity && c->N > c->n_images)
        return fail(SDM_ERR_INVALID, "more samples than images and no sample->image index set");
    if (!c->idx_identity && c->N > c->n_idx)
        return fail(SDM_ERR_INVALID, "sample->image index is shorter than the sample count");
    if (!c->idx_identity && c->max_idx >= c->n_images)
        return fail(SDM_ERR_INVALID, "sample->image index refers to an image beyond the current image set");
    return SDM_OK;
}

// the default mode's lane-packed launch is usable for this level
bool packed_ok(const sdm_ctx* c, int level)
{
    return c->fast_kernel[level] && !narrow_set(c) && c->packing && c->hog_mode == SDM_HOG_COLUMNS &&
           c->fast_bins[level] == 2 && c->plans[level].ok;
}
bool split_ok(const sdm_ctx* c, int level) { return packed_ok(c, level) && sdm_desc_supported(c->levels[level]); }

int hog_checks(sdm_ctx* c, int level)
{
    if (!c->img_base) return fail(SDM_ERR_INVALID, "no images set");
    if (c->N <= 0) return fail(SDM_ERR_INVALID, "no samples set (sdm_set_x)");
    if (c->levels[level].fixed_h == 0 && (c->eyes.nre <= 0 || c->eyes.nle <= 0))
        return fail(SDM_ERR_INVALID, "HOG features need eye landmark indices (IED-adaptive patch size)");
    return check_sample_index(c);
}

// the level's plan as the cells launch takes it (option hog_two_load)
static HogPlanDev cells_plan(const sdm_ctx* c, int level)
{
    HogPlanDev pd = c->plans[level].dev;
    pd.two_load = c->hog_two_load ? 1 : 0;
    return pd;
}

// pixel kernel of the split launch: images -> raw cell histograms of every (sample, landmark)
int launch_cells(sdm_ctx* c, int level)
{
    int rc = c->cells.ensure(sdm_cells_floats(c->levels[level], c->N, c->L));
    if (rc) return rc;
    sdm_launch_hog_cells(image_set(c), sample_index(c), c->x[c->cur].p, c->N, c->L, c->eyes,
                         c->levels[level], cells_plan(c, level), c->cells.p, c->patch_idx.p, c->status.p, c->stream);
    return SDM_OK;
}

int do_hog(sdm_ctx* c, int level)
{
    { const int rci = hog_checks(c, level); if (rci) return rci; }
    if (c->feat_wide_F > level_F(c, level)) {
        // an earlier launch wrote wider rows: its columns beyond this level's F would be stale -- clear every row written since the
        // last clear, once
        const size_t rows = (size_t)(c->feat_wide_N > c->N ? c->feat_wide_N : c->N);
        HIP_TRY(hipMemsetAsync(c->feat.p, 0, rows * c->ldf * sizeof(float), c->stream));
        c->feat_wide_F = 0; c->feat_wide_N = 0;
        c->ev_fresh = false;      // (untimed work: the next timed stage records its own start)
    }
    {
        Timer t(c, SDM_T_HOG);
        if (c->split_store && split_ok(c, level)) {
            const int rcc = launch_cells(c, level);
            if (rcc) return rcc;
            sdm_launch_desc_store(c->levels[level], c->cells.p, c->plans[level].cut.p, c->N, c->L, c->feat.p, c->ldf, c->stream);
        } else if (packed_ok(c, level))
            sdm_launch_hog_packed(image_set(c), sample_index(c), c->x[c->cur].p, c->N, c->L,
                                  c->eyes, c->levels[level], c->plans[level].dev, c->feat.p, c->ldf, c->patch_idx.p,
                                  c->status.p, c->stream);
        else if (c->fast_kernel[level] && !narrow_set(c))
            sdm_launch_hog_fast(image_set(c), sample_index(c), c->x[c->cur].p, c->N, c->L,
                                c->eyes, c->levels[level], c->feat.p, c->ldf, c->patch_idx.p, c->status.p,
                                c->hog_mode /* = the kernel's ACC_* value */, c->fast_bins[level], c->stream);
        else   // generic S > 64 geometry: the reference-order kernel
            sdm_launch_hog(image_set(c), sample_index(c), c->x[c->cur].p, c->N, c->L,
                           c->eyes, c->levels[level], c->feat.p, c->ldf, c->patch_idx.p, c->status.p, c->stream);
    }
    if (c->tmpl_N > 0) {   // known-template mode: the regressors see features - templates (superviseddescent.hpp:195-197)
        if (c->tmpl_N != c->N || c->tmpl_F != level_F(c, level))
            return fail(SDM_ERR_INVALID, "templates do not match the sample count / feature dimension of this level");
        sdm_launch_subtract_templates(c->feat.p, c->ldf, c->tmpl.p, c->N, c->tmpl_F, c->stream);
        c->ev_fresh = false;
    }
    HIP_TRY(hipGetLastError());
    c->feat_level = level;
    if (level_F(c, level) > c->feat_wide_F) c->feat_wide_F = level_F(c, level);
    if (c->N > c->feat_wide_N) c->feat_wide_N = c->N;
    c->feat_bounded = c->tmpl_N == 0;
    c->have_patch_idx = true;
    return SDM_OK;
}

// the level's regressor operand as float16 planes (after every write of Rt[level])
int build_apply_planes(sdm_ctx* c, int level)
{
    int rc;
    if ((rc = c->Rp[level].ensure(sdm_apply_planes_bytes(c->ldf, c->M))) || (rc = c->Rmax.ensure(c->levels.size() * (size_t)Mp_of(c->M)))) return rc;
    sdm_launch_apply_planes(c->Rt[level].p, c->ldf, c->M, c->Rp[level].p, c->Rmax.p + (size_t)level * Mp_of(c->M), c->stream);
    if (c->plans[level].ok && sdm_desc_supported(c->levels[level])) {      // the same pieces per landmark, in fragment order (fused detect)
        if ((rc = c->Rd[level].ensure(sdm_desc_planes_bytes(c->levels[level], c->L, c->M)))) return rc;
        sdm_launch_desc_planes(c->levels[level], c->Rt[level].p, c->ldf, c->L, c->M, c->Rmax.p + (size_t)level * Mp_of(c->M),
                               c->Rd[level].p, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

int do_apply(sdm_ctx* c, int level)
{
    if (c->feat_level != level) return fail(SDM_ERR_INVALID, "sdm_apply: features of this level not extracted");
    if (!c->have_R[level]) return fail(SDM_ERR_INVALID, "sdm_apply: no regressor set for this level");
    const int F = level_F(c, level);
    const int splits = sdm_apply_splits(c->N, F, c->M);
    int rc = c->partial.ensure((size_t)splits * c->N * Mp_of(c->M));
    if (rc) return rc;
    {
        Timer t(c, SDM_T_APPLY);
        sdm_launch_apply(c->feat.p, c->ldf, c->N, F, c->Rt[level].p, c->ldf, c->M, c->x[c->cur].p,
                         c->x[c->cur ^ 1].p, c->L, c->eyes, c->partial.p, splits, c->stream,
                         (c->feat_bounded && !c->env_apply_f32) ? c->Rp[level].p : nullptr,
                         (c->feat_bounded && !c->env_apply_f32 && c->Rp[level].p) ? c->Rmax.p + (size_t)level * Mp_of(c->M) : nullptr);
    }
    HIP_TRY(hipGetLastError());
    c->cur ^= 1;
    return SDM_OK;
}

// one cascade level of sdm_detect_batch without the feature matrix: cells -> (descriptors x regressor slices) -> landmark update
bool fused_ok(const sdm_ctx* c, int level)
{
    // Wide outputs stay on the feature-matrix path: a fused workgroup (32 samples x one landmark) reads the landmark's whole P x 2L
    // slice of the regressor from L2 -- 77 KB at 2L = 44, 230 KB at 2L = 136, where that traffic (4 GB per level at 8 192 samples)
    // makes the launch slower than writing the rows and running the GEMM (RCR-68 detect: 0.53 against 0.25 ms per level;
    // SDM_DETECT_FUSE_WIDE=1 fuses anyway)
    return c->fuse_apply && (Mp_of(c->M) <= 64 || c->env_fuse_wide || c->fuse_wide) && split_ok(c, level) && c->have_R[level] && c->Rd[level].p &&
           c->Rp[level].p && c->tmpl_N == 0;
}
// A cascade level of detect, fused: cells -> (descriptors x regressor slices) -> landmark update; the feature matrix is not
// written.  (Measured and dropped: the batch as two blocks of rows on two queues, so that the short descriptor / update launches of
// one block overlap the pixel kernel of the other -- 1.352 against 1.354 ms: the pixel kernel's workgroups hold every register
// and LDS slot of a CU, the 51 KB descriptor workgroups of the other queue are admitted only when it drains.  Round 5 repeated it
// as VERDICT r04 item 4b asks -- two half batches, each its own chain of levels on its own queue, the second started one pixel
// kernel behind the first, optionally with the descriptor / update launches on highest-priority queues: 1.72 / 1.86 ms against
// 1.12 ms per 4 096 faces (profiles/r05_experiments.txt): two pixel kernels sharing the chip are slower than one after the other.)
int detect_level_fused(sdm_ctx* c, int l)
{
    { const int rci = hog_checks(c, l); if (rci) return rci; }
    const int Mp = Mp_of(c->M);
    int rc;
    size_t cells_max = 0;
    for (size_t q = 0; q < c->levels.size(); ++q) { const size_t n = sdm_cells_floats(c->levels[q], c->N, c->L); if (n > cells_max) cells_max = n; }
    if ((rc = c->cells.ensure(cells_max)) || (rc = c->partial.ensure((size_t)c->L * c->N * Mp))) return rc;
    const HogLevelDev& lv = c->levels[l];
    {
        Timer t(c, SDM_T_HOG);
        sdm_launch_hog_cells(image_set(c), sample_index(c), c->x[c->cur].p, c->N, c->L, c->eyes, lv,
                             cells_plan(c, l), c->cells.p, c->patch_idx.p, c->status.p, c->stream);
    }
    {
        Timer t(c, SDM_T_APPLY);
        sdm_launch_desc_apply(lv, c->cells.p, c->plans[l].cut.p, c->N, c->L, c->M, c->Rd[l].p, c->Rmax.p + (size_t)l * Mp,
                              c->Rt[l].p, c->ldf, c->partial.p, c->stream);
        sdm_launch_apply_reduce(c->partial.p, c->L, c->N, c->M, c->x[c->cur].p, c->x[c->cur ^ 1].p, c->L, c->eyes, c->stream);
    }
    HIP_TRY(hipGetLastError());
    c->cur ^= 1;
    c->feat_level = -1;          // (the feature rows were not produced)
    c->have_patch_idx = true;    // (this level's patch half-widths and centres)
    return SDM_OK;
}

// one cascade level of detect: fused when the level qualifies, else feature rows + apply GEMM
int detect_level(sdm_ctx* c, int l)
{
    if (fused_ok(c, l)) return detect_level_fused(c, l);
    int rc = do_hog(c, l);
    if (!rc) rc = do_apply(c, l);
    return rc;
}

}  // namespace sdm_capi

extern "C" {

int sdm_hog_features(sdm_ctx* c, int level, float* feat_host)
{
    if (!c || level < 0 || level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "bad level");
    HIP_TRY(hipSetDevice(c->device));
    int rc = do_hog(c, level);
    if (rc) return rc;
    if (feat_host) {
        const int F = level_F(c, level);
        HIP_TRY(hipMemcpy2DAsync(feat_host, (size_t)F * sizeof(float), c->feat.p, (size_t)c->ldf * sizeof(float),
                                 (size_t)F * sizeof(float), c->N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return check_status(c);
    }
    return SDM_OK;
}

int sdm_get_patch_indices(sdm_ctx* c, int* idx)
{
    if (!c || !idx || c->N <= 0 || !c->have_patch_idx) return fail(SDM_ERR_INVALID, "no HOG call to report");
    HIP_TRY(hipMemcpyAsync(idx, c->patch_idx.p, (size_t)c->N * (1 + 2 * c->L) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_set_regressor(sdm_ctx* c, int level, const float* R)
{
    if (!c || !R || level < 0 || level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "bad regressor");
    HIP_TRY(hipSetDevice(c->device));
    const int F = level_F(c, level), M = c->M, Mp = Mp_of(M);
    int rc = c->Rt[level].ensure((size_t)Mp * c->ldf);
    if (rc) return rc;
    std::vector<float> t((size_t)Mp * c->ldf, 0.0f);
    for (int k = 0; k < F; ++k)
        for (int j = 0; j < M; ++j) t[(size_t)j * c->ldf + k] = R[(size_t)k * M + j];
    HIP_TRY(hipMemcpyAsync(c->Rt[level].p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = build_apply_planes(c, level))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_R[level] = true;
    return SDM_OK;
}

int sdm_get_regressor(sdm_ctx* c, int level, float* R)
{
    if (!c || !R || level < 0 || level >= (int)c->levels.size() || !c->have_R[level]) return fail(SDM_ERR_INVALID, "no regressor");
    const int F = level_F(c, level), M = c->M, Mp = Mp_of(M);
    std::vector<float> t((size_t)Mp * c->ldf);
    HIP_TRY(hipMemcpyAsync(t.data(), c->Rt[level].p, t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < F; ++k)
        for (int j = 0; j < M; ++j) R[(size_t)k * M + j] = t[(size_t)j * c->ldf + k];
    return SDM_OK;
}

int sdm_apply(sdm_ctx* c, int level)
{
    if (!c || level < 0 || level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "bad level");
    HIP_TRY(hipSetDevice(c->device));
    return do_apply(c, level);
}

int sdm_detect_batch(sdm_ctx* c, float* x_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    c->chain_timers = true; c->ev_fresh = false;
    int rc = SDM_OK;
    for (int l = 0; l < (int)c->levels.size() && !rc; ++l) rc = detect_level(c, l);
    c->chain_timers = false; c->ev_fresh = false;
    if (rc) return rc;
    if (x_host) return sdm_get_x(c, x_host);
    return SDM_OK;
}

int sdm_detect_level(sdm_ctx* c, int level)
{
    if (!c || level < 0 || level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "bad level");
    HIP_TRY(hipSetDevice(c->device));
    return detect_level(c, level);
}


}  // extern "C"
