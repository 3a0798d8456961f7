// sdm_capi_sweep.hip -- regulariser sweep of one cascade level: one feature extraction and one Gram product, K regularise + factor +
// solve passes against a kept copy of the normal equations, every candidate scored on held-out rows that never leave the device
// (C-ABI of include/sdm.h; shared declarations: sdm_capi_internal.h)
#include "sdm_capi_internal.h"

#include <limits>

namespace {

// a collective on this handle: the sweep sums the fit rows of ONE rank and scores ITS held-out rows
bool collectives_installed(const sdm_ctx* c)
{
    return c->allreduce || c->rccl_comm || c->reduce_scatter || c->rccl_reduce_scatter || c->shard_bcast || c->shard_allgather || c->shard_comm;
}

}  // namespace

extern "C" {

int sdm_train_level_sweep(sdm_ctx* c, int level, int reg_type, const float* reg_params, int K, int regularise_last_row,
                          long long n_train_global, int n_fit_rows, double* holdout_err, double* fit_err, float* lambdas,
                          int* status, int* best)
{
    if (!c || level < 0 || level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "bad level");
    if (!reg_params || !holdout_err || !lambdas || !status || !best) return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: null argument");
    if (K < 1 || K > 32) return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: 1 ... 32 candidates");
    if (reg_type != SDM_REG_MANUAL && reg_type != SDM_REG_MATRIX_NORM) return fail(SDM_ERR_INVALID, "bad regulariser type");
    if (n_fit_rows < 1 || n_fit_rows >= c->N) return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: 1 <= n_fit_rows < sample count required (the rows behind the fit rows are held out)");
    if (collectives_installed(c))
        return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: a collective is installed on this handle; the sweep runs on one rank (the held-out sums are not reduced)");
    if (!c->have_targets) return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: no targets set");
    if (c->eyes.nre <= 0 || c->eyes.nle <= 0) return fail(SDM_ERR_INVALID, "sdm_train_level_sweep: no eye landmarks (the score is normalised by the inter-eye distance)");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    // 1 + 2: features and targets of all rows, [A^T A | A^T b] over the fit rows
    if ((rc = sdm_hog_features(c, level, nullptr))) return rc;
    if ((rc = gram_rhs_rows(c, level, n_fit_rows))) return rc;
    const int F = level_F(c, level), M = c->M, Mp = Mp_of(M), N = c->N;
    const int Fp = round_up(F, 128), ncols = c->g_ncols;
    sdm_ctx::Sweep& sw = c->sweep;
    sw.K = 0; sw.level = -1; sw.ok = 0;                // (the slots are rewritten from here on)
    c->g_level = -1;                                   // G is factored in place below, K times
    const size_t rt_floats = (size_t)Mp * c->ldf, rp_bytes = sdm_apply_planes_bytes(c->ldf, M);
    const int splits = sdm_apply_splits(N, F, M);
    if ((rc = sw.snap.ensure(sdm_packed_tiles_count(F, c->rhs_tiles))) || (rc = sw.Rt.ensure((size_t)K * rt_floats)) ||
        (rc = sw.Rp.ensure((size_t)K * rp_bytes)) || (rc = sw.Rmax.ensure((size_t)K * Mp)) || (rc = sw.x.ensure((size_t)N * M)) ||
        (rc = sw.score.ensure((size_t)2 * 32 + 2 * SDM_SWEEP_SCORE_PARTS)) || (rc = sw.arrived.ensure(2)) ||
        (rc = c->partial.ensure((size_t)splits * N * Mp)) ||
        (rc = c->fro.ensure((size_t)F + 1)) || (rc = c->Rsol.ensure((size_t)Fp * Mp)) ||
        (rc = c->winv.ensure((size_t)Fp * 128 + sdm_backsolve_flag_floats(Fp))))
        return rc;
    // 3: the unregularised system beside G; ||G||_F^2 once (every candidate's lambda is a multiple of its root)
    {
        Timer t(c, SDM_T_GRAM);
        sdm_launch_sweep_snapshot(c->G.p, ncols, F, c->rhs_tiles, sw.snap.p, c->stream);
        if (reg_type == SDM_REG_MATRIX_NORM) sdm_launch_fro2_upper(c->G.p, ncols, F, c->fro.p, c->stream);
    }
    HIP_TRY(hipGetLastError());
    const int n_reg = (int)(n_train_global > 0 ? n_train_global : n_fit_rows);
    const bool planes = c->feat_bounded && !c->env_apply_f32;
    double* score_part = sw.score.p + 2 * 32;
    // 4 + 5: one pass per candidate -- restore, regularise, factor + solve (sdm_solve's launches), keep R_k, score its update
    for (int k = 0; k < K; ++k) {
        float* Rt_k = sw.Rt.p + (size_t)k * rt_floats;
        unsigned char* Rp_k = sw.Rp.p + (size_t)k * rp_bytes;
        unsigned* Rmax_k = sw.Rmax.p + (size_t)k * Mp;
        {
            Timer t(c, SDM_T_REG);
            if (k > 0) sdm_launch_sweep_restore(c->G.p, ncols, F, c->rhs_tiles, sw.snap.p, c->stream);      // (candidate 0 finds the product itself)
            sdm_launch_add_diag(c->G.p, ncols, F, c->fro.p + F, reg_type, reg_params[k], n_reg, regularise_last_row, c->lambda_dev.p, c->stream);
        }
        {
            Timer t(c, SDM_T_FACTOR);
            if (c->solver_kind == SDM_SOLVER_COLPIV_QR) {
                if ((rc = qr_solve(c, c->G.p, ncols, F, Fp, Mp, c->Rsol.p))) return rc;
            } else {
                if ((rc = solve_update_scratch(c, ncols))) return rc;
                (void)sdm_launch_cholesky_solve(c->G.p, ncols, F, Fp, Mp, c->Rsol.p, Mp, c->winv.p, c->status.p, c->stream, &c->solve_aux, nullptr);
            }
        }
        HIP_TRY(hipGetLastError());
        sdm_launch_pack_regressor(c->Rsol.p, F, M, Mp, Rt_k, c->ldf, nullptr, c->stream);
        sdm_launch_apply_planes(Rt_k, c->ldf, M, Rp_k, Rmax_k, c->stream);
        {
            // x_{k+1} of this candidate into the scratch rows (sdm_apply's launch: the same bits), then both means in one launch.
            // Queued before the status is known: a failed candidate's numbers are never read.
            Timer t(c, SDM_T_APPLY);
            sdm_launch_apply(c->feat.p, c->ldf, N, F, Rt_k, c->ldf, M, c->x[c->cur].p, sw.x.p, c->L, c->eyes, c->partial.p, splits, c->stream,
                             planes ? Rp_k : nullptr, planes ? Rmax_k : nullptr);
            sdm_launch_sweep_score(sw.x.p, c->xstar.p, N, n_fit_rows, c->L, c->eyes, score_part, sw.arrived.p, sw.score.p + 2 * k, c->stream);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(lambdas + k, c->lambda_dev.p, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        status[k] = check_status(c);                   // (synchronises the stream; clears the kernel status word)
        if (status[k] != SDM_OK && status[k] != SDM_ERR_NOT_SPD) return status[k];
        if (status[k] == SDM_OK) sw.ok |= 1u << k;
    }
    double means[2 * 32];
    HIP_TRY(hipMemcpyAsync(means, sw.score.p, (size_t)2 * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    sw.K = K; sw.level = level;
    // 6: the arg-min of the held-out means, ties to the lowest k
    int win = -1;
    for (int k = 0; k < K; ++k) {
        const bool ok = status[k] == SDM_OK;
        holdout_err[k] = ok ? means[2 * k] : std::numeric_limits<double>::infinity();
        if (fit_err) fit_err[k] = ok ? means[2 * k + 1] : std::numeric_limits<double>::infinity();
        if (ok && (win < 0 || holdout_err[k] < holdout_err[win])) win = k;
    }
    *best = win;
    if (win < 0) return fail(SDM_ERR_NOT_SPD, "sdm_train_level_sweep: no candidate gave a positive definite system; increase the regulariser");
    if ((rc = c->Rt[level].ensure(rt_floats))) return rc;
    HIP_TRY(hipMemcpyAsync(c->Rt[level].p, sw.Rt.p + (size_t)win * rt_floats, rt_floats * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = build_apply_planes(c, level))) return rc;
    c->have_R[level] = true;
    return sdm_apply(c, level);
}

int sdm_sweep_get_regressor(sdm_ctx* c, int k, float* R)
{
    if (!c || !R) return fail(SDM_ERR_INVALID, "sdm_sweep_get_regressor: null argument");
    const sdm_ctx::Sweep& sw = c->sweep;
    if (sw.K <= 0 || sw.level < 0 || sw.level >= (int)c->levels.size()) return fail(SDM_ERR_INVALID, "sdm_sweep_get_regressor: no sweep has run on this handle");
    if (k < 0 || k >= sw.K) return fail(SDM_ERR_INVALID, "sdm_sweep_get_regressor: no such candidate");
    if (!(sw.ok >> k & 1u)) return fail(SDM_ERR_NOT_SPD, "sdm_sweep_get_regressor: this candidate's system was not positive definite");
    HIP_TRY(hipSetDevice(c->device));
    const int F = level_F(c, sw.level), M = c->M, Mp = Mp_of(M);
    std::vector<float> t((size_t)Mp * c->ldf);
    HIP_TRY(hipMemcpyAsync(t.data(), sw.Rt.p + (size_t)k * t.size(), t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < M; ++j) R[(size_t)i * M + j] = t[(size_t)j * c->ldf + i];
    return SDM_OK;
}

}  // extern "C"
