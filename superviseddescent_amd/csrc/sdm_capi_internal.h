// sdm_capi_internal.h -- what the translation units of the C-ABI (include/sdm.h) share: the handle (struct sdm_ctx), device buffers,
// error reporting, the stage timer, and the launch sequences of a cascade level that more than one entry point runs.
// Host-side bookkeeping only: all arithmetic of the hot path runs in the gfx950 kernels; there is no CPU fallback -- without a
// device sdm_create() fails.
//   sdm_capi_context.hip   lifetime, geometry, images, samples            sdm_capi_detect.hip    features, regressors, apply, detect
//   sdm_capi_train.hip     targets, Gram / right-hand side, solvers       sdm_capi_exchange.hip  the several-GPU exchange of the normal equations
//   sdm_capi_debug.hip     device pointers, timing, debug entry points   sdm_capi_pose.hip / sdm_capi_track.hip  head pose, tracking
//   sdm_capi_align.hip     aligned face crops                          sdm_capi_sweep.hip     regulariser sweep on one Gram product
//   sdm_capi_frames.hip    device-resident frames as the image set     sdm_capi_upright.hip   upright chips for rolled faces
//   sdm_capi_warp.hip      piecewise-affine warped faces               sdm_capi_paste.hip     crop tensors pasted back into frames
#pragma once
#include "../../include/sdm.h"
#include "sdm_kernels.h"

#include <dlfcn.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace sdm_capi {


// the last error of the calling thread (sdm_last_error)
inline std::string& err_string() { static thread_local std::string e; return e; }

inline int fail(int code, const std::string& msg)
{
    err_string() = msg;
    return code;
}

// The one rule of every image entry point: an image the fused pixel kernels cannot serve sends its whole set to the generic kernel
// (same results, slower).  Their paired-byte loads need 2 columns, their packed row tables rows below 2^16, their buffer
// descriptor (num_records) a plane of at most INT_MAX bytes.  They form (row of the patch) * stride in 32 bits, for rows above and
// below the image too, and rely on the range check against num_records to read those as black: a product that passes 2^31 outside
// the plane wraps back into it.  The stride bound keeps that 2 048 rows away at the least (include/sdm.h, "Frame geometry").
constexpr long long SDM_FUSED_MAX_STRIDE = 1ll << 20;
inline bool image_needs_generic(int w, int h, long long stride)
{
    return w < 2 || h > 65535 || stride > SDM_FUSED_MAX_STRIDE || stride * h > (long long)INT_MAX;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(SDM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    int ensure(size_t n, bool zero = false, hipStream_t s = nullptr)
    {
        if (n <= cap) return SDM_OK;
        if (p) { hipError_t e = hipFree(p); (void)e; p = nullptr; cap = 0; }
        hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e != hipSuccess) return fail(SDM_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        cap = n;
        if (zero) {
            e = hipMemsetAsync(p, 0, n * sizeof(T), s);
            if (e != hipSuccess) return fail(SDM_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
        }
        return SDM_OK;
    }
    void release()
    {
        if (p) { hipError_t e = hipFree(p); (void)e; }
        p = nullptr; cap = 0;
    }
};

// function-local scratch: freed on every exit path (the context's own buffers are released in sdm_destroy)
template <class T>
struct ScopedBuf : DevBuf<T> {
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf&) = delete;
    ScopedBuf& operator=(const ScopedBuf&) = delete;
    ~ScopedBuf() { this->release(); }
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }


}  // namespace sdm_capi
using namespace sdm_capi;

struct sdm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    SolveAux solve_aux = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};   // second queue of the Cholesky look-ahead (+ the scratch of its float16 updates, set per solve)
    DevBuf<unsigned char> upd_planes;    // one panel group as float16 planes (sdm_update_f16_plane_bytes)
    DevBuf<unsigned> upd_maxdiag;

    // geometry
    int L = 0, M = 0;
    EyeIdxDev eyes{};
    std::vector<HogLevelDev> levels;
    std::vector<sdm_hog_param> params;
    std::vector<int> fast_kernel;   // per level: fused S<=64 kernel usable
    std::vector<int> fast_bins;     // per level: un-normalised arg-max verified on all 511x511 gradients
    // per level: lane-packed launch plan (sdm_hog_packed.hip::hog_packed_kernel), device tables owned here
    struct Plan { bool ok = false; HogPlanDev dev{}; DevBuf<unsigned> lane_tab; DevBuf<float> wb; DevBuf<unsigned short> wb16; DevBuf<int> pass_info; DevBuf<int> cut; DevBuf<int> taps; DevBuf<int> pair_taps; };
    std::vector<Plan> plans;
    // round 4: the packed launch stops at the raw cell histograms (cells[N][L][2 parts][C*C][2O]); sdm_desc.hip normalises them into the
    // feature rows, or -- sdm_detect_batch -- multiplies the descriptors by the regressor without writing the feature matrix
    DevBuf<float> cells;
    int solver_kind = SDM_SOLVER_CHOLESKY;      // sdm_set_solver
    int last_rank = -1, last_rank_full = 0;     // of the last column-pivoted QR (sdm_last_rank)
    DevBuf<float> qr_work;
    // The feature ROWS (training, sdm_hog_features) still come from the launch that normalises inside the pixel kernel: writing the
    // rows is HBM-bound on its own (55 us per 4 096 x 22 patches) and hides behind the pixel work there; measured 5 % slower split.
    bool split_store = false;       // option hog_split_store: feature rows through cells + sdm_desc.hip's store form (A/B, tests)
    bool fuse_apply = true;         // option detect_unfused: sdm_detect_batch through the feature matrix + apply GEMM (A/B)
    bool fuse_wide = false;         // sdm_debug_set_detect_path(fused = 2): fuse also when 2L > 64 (tests of the wide launch)
    bool hog_two_load = false;      // option hog_two_load: the CELLS pixel kernel never takes its one-load row loop (A/B, tests)
    bool packing = true;            // sdm_debug_set_hog_packing / option hog_no_pack: run the one-patch-per-wave kernel instead
    // development switches, set by sdm_debug_set_option (the library reads no environment variable; names in sdm_capi_debug.hip)
    bool env_fuse_wide = false;     // option detect_fuse_wide: fuse descriptor + apply also when 2L > 64
    bool env_apply_f32 = false;     // option apply_f32: sdm_apply always on the f32 matrix-core kernel
    bool env_gram_f32 = false;      // option gram_f32: Gram matrix on the f32 matrix-core kernel of rounds 1-2
    bool env_gram_bf16 = false;     // option gram_bf16x3: Gram matrix always in the three-bf16-piece form
    int env_shard_emulate = 0;      // option solve_shard_emulate: timing harness of the sharded factorisation (scripts/sharded_solve_timing.py)
    int hog_mode = SDM_HOG_COLUMNS;
    int Fmax = 0;
    long long ldf = 0;      // feature row stride: round_up(Fmax,128) + 128*rhs_tiles (tail tiles = training targets)
    int rhs_tiles = 1;      // 128-column tiles that hold the 2L target columns (2 when 2L > 128)

    // images
    DevBuf<uint8_t> img_owned;
    const uint8_t* img_base = nullptr;
    DevBuf<long long> img_off;
    DevBuf<int> img_w, img_h, img_stride;
    int n_images = 0;
    bool narrow_images = false;   // an image less than 2 pixels wide or 65536+ rows high: the fused kernel's paired-byte
                                  // loads need w >= 2, its packed row tables h < 2^16 -> the generic kernel runs instead
    DevBuf<int> img_idx;
    bool idx_identity = true;
    int n_idx = 0, max_idx = -1;   // length and largest entry of the sample -> image index (checked against N / n_images per launch)

    // samples
    int N = 0;
    DevBuf<float> x[2];
    int cur = 0;
    DevBuf<float> xstar;
    DevBuf<float> tmpl;     // known-template mode: N x tmpl_F templates subtracted from the features of every level
    int tmpl_F = 0, tmpl_N = 0;
    bool have_targets = false;
    DevBuf<float> feat;
    int feat_level = -1;            // level whose rows are resident (-1: none) -- only the "features of this level extracted" check
    // what the rows may still hold from EARLIER launches: the widest feature row and the most rows written since the
    // buffer was last cleared.  A level with a narrower row clears them first, whatever ran in between (a fused detect level, a
    // different sample count): the Gram kernel multiplies whole 128-column tiles and add_diag assumes the padding is zero.
    int feat_wide_F = 0, feat_wide_N = 0;
    // The float16-piece apply (sdm_apply.hip) scales every feature by 2^12 before the split: exact for |feature| < 16, which HOG
    // descriptors (<= 0.4) satisfy by construction.  Rows that are NOT plain HOG output -- templates subtracted, or the caller holds
    // the device pointer (sdm_features_device_ptr) and may have written them -- go through the f32 matrix-core kernel.
    bool feat_bounded = false;
    DevBuf<int> patch_idx;
    bool have_patch_idx = false;    // the last HOG launch (feature rows or fused cascade level) left its integer decisions in patch_idx
    DevBuf<int> status;
    DevBuf<float> partial;

    // regressors, transposed + padded: [Mp][ldf]
    std::vector<DevBuf<float>> Rt;
    std::vector<DevBuf<unsigned char>> Rp;   // the same regressors as two float16 planes (the 16-bit matrix-core apply, sdm_apply.hip)
    std::vector<DevBuf<unsigned char>> Rd;   // ... and per landmark in matrix-core fragment order (the fused descriptor + apply launch, sdm_desc.hip)
    DevBuf<unsigned> Rmax;                   // per level and output column: bits of max |R| (the planes' power-of-two scales)
    std::vector<bool> have_R;

    // normal equations
    DevBuf<float> G;       // [ncols][ncols]
    DevBuf<float> gpack;   // data-parallel exchange buffer: upper Gram tiles + RHS tiles, packed
    int g_ncols = 0;
    int g_fp = 0;
    int g_level = -1;
    DevBuf<double> fro;
    DevBuf<float> Rsol;    // [Fp][Mp_ld]
    DevBuf<float> winv;    // [Fp/128][128][128] transposed inverses of the diagonal factor tiles
    DevBuf<int> gram_flag;               // raised by the float16 split when an operand leaves float16's range
    // exchange behind the Gram kernel (round 4): with the factorisation sharded and a reduce-scatter installed, the Gram matrix is
    // multiplied in up to SDM_XBLOCKS ranges of tile columns; an event behind each range lets the second queue ship that range's
    // tiles (pack -> reduce-scatter -> unpack) while the next range is being multiplied
    static const int XBLOCKS_MAX = 8;
    hipEvent_t gram_ev[XBLOCKS_MAX] = {}; hipEvent_t gram_xdone = nullptr;
    int gram_blocks = 0;                 // ranges of the Gram matrix in G (0: one launch, no events recorded)
    int gram_block_c[XBLOCKS_MAX + 1] = {};      // their boundaries in OWNED column numbers (tile column = rank + world * number)
    int env_xblocks = -1;                // option gram_xblocks: -1 = automatic (4 from 128 tile columns on), 1 = never, n = always n
    int gram_fallbacks = 0;              // launches repeated with three bf16 pieces (sdm_debug_gram_fallbacks)
    int update_range_fallbacks = 0;      // factorisations that ran their trailing updates in f32 because the diagonal spanned > 2^20
    int gram_f32_fallbacks = 0;          // launches that ran on the f32 matrix-core kernel because the planes could not be allocated
    DevBuf<unsigned char> gram_planes;   // the feature matrix as three bf16 planes (sdm_gram_bf16.hip), scratch of sdm_gram_rhs
    DevBuf<float> lambda_dev;

    sdm_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    int world_size = 1;
    // native exchange: ncclAllReduce of the RCCL the process already uses (or librccl loaded on demand)
    void* rccl_comm = nullptr;
    int (*rccl_allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    // sharded factorisation (sdm_set_solve_sharding*): rank / world of the SOLVE, its two collectives, staging tiles
    int shard_rank = 0, shard_world = 0;          // world 0 = replicated solve
    sdm_bcast_fn shard_bcast = nullptr;
    sdm_allgather_fn shard_allgather = nullptr;
    void* shard_user = nullptr;
    void* shard_comm = nullptr;                   // ncclComm_t of the native path
    int (*rccl_bcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*rccl_allgather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    DevBuf<float> shard_stage;
    // reduce-scatter exchange of the Gram matrix (sdm_set_reduce_scatter*): used by sdm_allreduce_gram_rhs when the solve is sharded
    sdm_reduce_scatter_fn reduce_scatter = nullptr;
    void* reduce_scatter_user = nullptr;
    int (*rccl_reduce_scatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    bool g_scattered = false;                     // the Gram matrix holds the summed tiles of the OWNED tile columns only
    DevBuf<float> gsmall;                         // summed diagonal + the Frobenius share (the small all-reduce of that exchange)

    // head pose (sdm_capi_pose.hip): the ModelProjection cascade, state of its own beside the landmark state above, so that a
    // detect batch's landmarks reach it without leaving the device (sdm_pose_templates_from_landmarks)
    struct Pose {
        PoseCamDev cam{};                  // cam.K == 0: no model set
        DevBuf<float> pts;                 // K x 3 model points
        int N = 0;                         // rows of x
        DevBuf<float> x, xstar, tmpl;      // N x 6, N x 6, tmpl_N x 2K
        int tmpl_N = 0;
        bool have_targets = false;
        DevBuf<float> R;                   // SDM_POSE_MAX_LEVELS x 2K x 6, level l at l * 2K * 6
        unsigned have_R = 0;               // bit l: level l holds a regressor
        DevBuf<float> Ab;                  // training scratch: N x (2K + 6)
        DevBuf<double> partial, G;
        DevBuf<int> lm;                    // landmark index map of the gather
        void release() { pts.release(); x.release(); xstar.release(); tmpl.release(); R.release(); Ab.release(); partial.release(); G.release(); lm.release(); }
    } pose;

    // multi-stream tracking (sdm_capi_track.hip): a table of S stream slots beside the landmark state; a step gathers its rows into
    // x, runs the detect cascade and commits the results back, so that a stream's landmarks stay in HBM between frames
    struct Track {
        int S = 0;                         // capacity; 0: not configured
        int L = 0;                         // landmarks of the geometry at sdm_track_configure
        int mode = 0;                      // SDM_TRACK_INIT_*
        float min_size = 0.f, max_scale = 0.f;
        float mean_bounds[4] = {0.f, 0.f, 0.f, 0.f};    // min, max of the mean's x; min, max of its y
        DevBuf<float> mean;                // 2L
        DevBuf<float> x;                   // S x 2L slot landmarks
        DevBuf<int> box, status;           // S x 4 start boxes, S device statuses (read by the gather: STARTED or not)
        DevBuf<float> init;                // n x 2L: the rows the cascade started from (the scale rule), scratch of sdm_track_get
        DevBuf<int> ids, masks;            // n ids; n masks + the kernel status word
        bool upright = false;              // sdm_track_configure_upright: a step cuts upright chips (sdm_capi_upright.hip)
        DevBuf<double> cs;                 // S x (cos, sin) of the roll a slot was started with (upright mode)
        std::vector<int> host_status;      // mirror of the slots' statuses, refreshed from the masks every step
        std::vector<unsigned> seen;        // per slot: stamp of the last call that named it (duplicate check)
        unsigned stamp = 0;
        int* pin = nullptr;                // pinned staging of the ids / boxes in and the masks out
        size_t pin_cap = 0;                // ints
        // the temporal landmark filter (sdm_track_configure_filter, csrc/sdm_track_filter.hip): per slot the previous raw row, the
        // filtered derivative and the previous filtered row, and whether they hold anything
        int filter = 0;                    // SDM_TRACK_FILTER_*
        float min_cutoff = 0.f, beta = 0.f, d_cutoff = 0.f;
        DevBuf<float> filter_state;        // 3 x S x 2L: r, d, f
        DevBuf<int> primed;                // S
        DevBuf<float> filter_out;          // scratch of sdm_track_get_filtered: 2 x n x 2L + n ints
        void filter_off() { filter = 0; filter_state.release(); primed.release(); filter_out.release(); }
        // the motion-compensated initialisation (sdm_track_configure_motion, csrc/sdm_track_motion.hip): per slot {valid, k, ox, oy}, the
        // 32 x 32 reference chip and the last search's result; per row of a step the shift the gather adds
        int motion = 0;                    // SDM_TRACK_MOTION_*
        int motion_search = 0, motion_min_gain = 0;
        float motion_scale = 0.f;
        DevBuf<int> motion_state;          // S x 4
        DevBuf<uint8_t> motion_chips;      // S x 32 x 32
        DevBuf<int> motion_last;           // S x 6
        DevBuf<float> motion_shift;        // n x 2
        DevBuf<int> motion_out;            // scratch of sdm_track_get_motion: n x (6 + 3) ints + n x 1024 bytes
        void motion_off() { motion = 0; motion_state.release(); motion_chips.release(); motion_last.release(); motion_shift.release(); motion_out.release(); }
        void release()
        {
            mean.release(); x.release(); box.release(); status.release(); init.release(); ids.release(); masks.release(); cs.release();
            filter_off();
            motion_off();
            upright = false;
            if (pin) { hipError_t e = hipHostFree(pin); (void)e; }
            pin = nullptr; pin_cap = 0; S = 0;
        }
    } track;

    // aligned face crops (sdm_capi_align.hip): the source of the taps -- the images above (base null) or an external stack -- and
    // the per-call scratch
    struct Align {
        const uint8_t* base = nullptr;     // external stack; null: the context's images
        int n = 0, w = 0, h = 0, stride = 0, C = 1;
        DevBuf<uint8_t> owned;             // a host stack's copy
        DevBuf<int> in;                    // K indices + K x 2 template floats
        DevBuf<AlignFace> faces;           // N records
        DevBuf<uint8_t> crops;             // the crops of a host-memory out
        // a frame list as the source (sdm_align_set_source_frames; base stays null): the frames as given, their device table, the
        // lowest plane-0 address and the bytes per pixel all frames share (0: NV12 among them, or mixed)
        std::vector<sdm_frame> fr;
        DevBuf<AlignFrameDev> fr_dev;
        const uint8_t* fr_base = nullptr;
        int fr_bpp = 0;
        // the paste (sdm_capi_paste.hip): a call's frame table, row -> frame index and row lists in one block, and the rows' records
        DevBuf<unsigned char> paste_tab, paste_rows;
        // the landmark region masks (sdm_capi_mask.hip): a call's matrices and points (_at form), the rows' records, the hulls' sort
        // buffer and the vertex lists in one block
        DevBuf<unsigned char> region;
        void release()
        {
            in.release(); faces.release(); crops.release(); owned.release(); fr_dev.release(); paste_tab.release(); paste_rows.release();
            region.release();
            base = nullptr; n = 0; C = 1; fr.clear();
        }
    } align;
    // regulariser sweep (sdm_capi_sweep.hip): the unregularised normal equations kept as packed tiles, one regressor slot per
    // candidate (the apply GEMM's operand Rt + its float16 planes + their scale words) and the scoring scratch; allocated at the
    // first sweep
    struct Sweep {
        DevBuf<float> snap;                // upper Gram tiles + right-hand-side tiles (the exchange buffer's layout)
        DevBuf<float> Rt;                  // K slots of Mp x ldf
        DevBuf<unsigned char> Rp;          // K slots of sdm_apply_planes_bytes
        DevBuf<unsigned> Rmax;             // K slots of Mp scale words
        DevBuf<float> x;                   // N x 2L: x_{k+1} of the candidate being scored (the state x is not touched)
        DevBuf<double> score;              // 2 K means (held-out, fit) + the score kernel's partial sums
        DevBuf<unsigned> arrived;          // per row range: workgroups of the score kernel that have delivered their partial sum
        int K = 0, level = -1;             // candidates and level of the last sweep (K == 0: none); ok: bit k = candidate k solved
        unsigned ok = 0;
        void release() { snap.release(); Rt.release(); Rp.release(); Rmax.release(); x.release(); score.release(); arrived.release(); K = 0; level = -1; ok = 0; }
    } sweep;
    // frames on the device (sdm_capi_frames.hip): the gray images converted from a call's colour frames -- each starts on a 16-byte
    // boundary, row stride sdm_frames_gray_stride(w) -- and the conversion launch's descriptor table
    struct Frames {
        DevBuf<uint8_t> gray;
        DevBuf<FrameConvDev> desc;
        void release() { gray.release(); desc.release(); }
    } frames;
    // upright-normalised detect and tracking (sdm_capi_upright.hip): the stack of chips with its image table, and the rows' records.
    // While `active` the cascade's launches read the chips, one per row, in place of the context's images (sdm_capi_detect.hip).
    struct Upright {
        int chip = 0, guard = 0;           // chip == 0: sdm_upright_configure not called
        bool active = false;
        int N = 0;                         // rows of the last upright call (the records and chips sdm_upright_get returns)
        DevBuf<uint8_t> chips;
        DevBuf<long long> off;
        DevBuf<int> w, h, stride;
        DevBuf<UprightRow> rows;
        DevBuf<double> in;                 // a detect call's (cos, sin) pairs, boxes and mean
        void release() { chips.release(); off.release(); w.release(); h.release(); stride.release(); rows.release(); in.release(); chip = 0; N = 0; }
    } upright;
    // piecewise-affine warped faces (sdm_capi_warp.hip): the mesh of sdm_warp_set_mesh -- label map, triangle table, landmark indices --
    // and the per-call records with the N x T x 6 matrices behind them
    struct Warp {
        int K = 0, T = 0, L = 0;           // T == 0: no mesh; L: landmarks of the geometry at sdm_warp_set_mesh
        int out_w = 0, out_h = 0;
        std::vector<uint8_t> labels_host;  // out_h x out_w
        DevBuf<uint8_t> labels;
        DevBuf<unsigned char> tri;         // T WarpTri records (csrc/sdm_warp_device.h)
        DevBuf<int> lm;                    // K
        DevBuf<unsigned char> rows;        // N WarpFace records, then N x T x 6 floats, then (filtered call) N x T x 2 ints
        // the piecewise-affine paste (sdm_capi_paste.hip): the landmark indices on the host, the uploaded points of the _at form in the
        // landmark state's layout, and a call's N WarpPasteRow records with the N x T WarpPasteTri records behind them
        std::vector<int> lm_host;
        DevBuf<float> points;
        DevBuf<unsigned char> paste;
        void drop() { K = T = L = out_w = out_h = 0; labels_host.clear(); lm_host.clear(); }
        void release() { drop(); labels.release(); tri.release(); lm.release(); rows.release(); points.release(); paste.release(); }
    } warp;
    // host copies of the image sizes and of the sample -> image index (the checks of an external crop source)
    std::vector<int> img_w_host, img_h_host, img_idx_host;

    // timing
    bool timing = false;
    float t_ms[SDM_T_COUNT] = {0};
    int t_n[SDM_T_COUNT] = {0};
    struct Pending { int slot; hipEvent_t a, b; bool a_shared; };
    // inside sdm_detect_batch consecutive timed stages share one event (stop of one = start of the next): every recorded
    // event is a pipeline bubble of a few microseconds between two kernels
    hipEvent_t last_stop = nullptr;
    bool ev_fresh = false, chain_timers = false;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

namespace sdm_capi {

inline int Mp_of(int M) { return round_up(M, 16); }
inline int level_F(const sdm_ctx* c, int level) { return c->L * c->levels[level].P + (c->levels[level].fixed_h > 0 ? 0 : 1); }

struct Timer {
    sdm_ctx* c; int slot; hipEvent_t a = nullptr, b = nullptr; bool a_shared = false;
    Timer(sdm_ctx* ctx, int s) : c(ctx), slot(s)
    {
        if (!c->timing) return;
        if (c->chain_timers && c->ev_fresh) { a = c->last_stop; a_shared = true; }      // nothing was enqueued since that stop
        else { a = take(); hipError_t e = hipEventRecord(a, c->stream); (void)e; }
        b = take();
    }
    hipEvent_t take()
    {
        if (!c->pool.empty()) { hipEvent_t ev = c->pool.back(); c->pool.pop_back(); return ev; }
        hipEvent_t ev; hipError_t e = hipEventCreate(&ev); (void)e; return ev;
    }
    ~Timer()
    {
        if (!c->timing) return;
        hipError_t e = hipEventRecord(b, c->stream); (void)e;
        c->pending.push_back({slot, a, b, a_shared});
        c->last_stop = b; c->ev_fresh = true;
    }
};

// (defined in sdm_capi_detect.hip unless noted)
void fill_row_tab(HogLevelDev& lv);
void drain_timing(sdm_ctx* c);
int check_status(sdm_ctx* c);
ImageSetDev image_set(const sdm_ctx* c);
const int* sample_index(const sdm_ctx* c);
ImageSetDev frame_set(const sdm_ctx* c);              // the context's images, whatever is in flight
// (sdm_capi_upright.hip) what an upright call of n rows checks before anything is launched, its buffers, and the launches behind the
// set-up kernel: chips, the cascade on them, the back-map
int upright_check(sdm_ctx* c, int n);
int upright_ensure(sdm_ctx* c, int n);
int upright_run(sdm_ctx* c, int n);
int upright_roll_cs(float roll_deg, double* cs);
// (sdm_capi_frames.hip) bytes per pixel of a frame's plane 0 (NV12: luma; 0: unknown format), and what every entry point that takes
// frames refuses of frame i: format, null pointer, width / height, stride -- with allow_nv12 false (the pastes) an NV12 frame first
int frame_bpp(int format);
int check_frame(int i, const sdm_frame& frame, bool allow_nv12);
// SDM_FRAME_BGR_PLANAR | SDM_FRAME_RGB_PLANAR (frame_bpp: 1, the bytes per pixel of a plane)
bool frame_planar(int format);
// GRAY and NV12 (any colour description): the image set reads plane 0 where it lies
bool frame_in_place(int format);
// what the calls that read or write the UV plane refuse of an NV12 or P010 frame: a UV row that does not fit stride_bytes; P010: an odd
// UV pointer (uv: the plane's address)
int check_frame_uv(int i, const sdm_frame& frame, const void* uv);
// D of a planar frame: second - data, or height * stride_bytes when second is null; 0 is refused
int frame_plane_distance(int i, const sdm_frame& frame, const void* second, long long& D);
// (sdm_capi_align.hip) the checks and the element stage's constants that sdm_align_crops_tensor and sdm_warp_crops_tensor share: the
// specification, the output pointer, that the crop source covers every row's image with that image's size, the source itself and the
// landmark subset of a template
int align_check_call(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h);      // geometry, rows, indices, template, crop size
int align_fit_rows(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h);        // the fit of every row into align.faces
int align_check_spec(const sdm_align_tensor* spec);
int align_check_filter(const sdm_align_filter* filter);                                                    // mode, max_samples, min_scale
int align_check_out(const void* out_dev);
int align_check_rows(sdm_ctx* c);
AlignTensorDev align_tensor_dev(const sdm_align_tensor* spec);
// the current crop source as the two fits and the tensor kernels read it
AlignSourceDev align_source_dev(const sdm_ctx* c);
struct AlignTapSource { const uint8_t* base; const AlignFrameDev* frames; int stack_format; };     // (frames null: stack_format at base + off)
AlignTapSource align_tap_source(const sdm_ctx* c);
// what the filtered crop and paste calls share behind their checks: the checked filter as the kernels read it; the records of
// align.faces that hold N rows -- with room for N ints, the rows' S, behind them when with_samples --; and, behind a call's launches,
// the N records -- and S behind them when samples_host is given -- in one copy, one synchronise, scattered to the caller's arrays
// (each may be null)
AlignAreaDev align_area_dev(const sdm_align_filter* filter);
size_t align_face_records(int N, bool with_samples);
int align_fetch_rows(sdm_ctx* c, int N, float* matrices_host, int* flags_host, int* samples_host);
// K in [Kmin, L], K distinct landmark indices in [0, L), a finite template of K points
int check_landmark_subset(const sdm_ctx* c, const int* lm, const float* tmpl, int K, int Kmin);
int ensure_sample_buffers(sdm_ctx* c, int N);
int check_sample_index(const sdm_ctx* c);
bool packed_ok(const sdm_ctx* c, int level);
bool split_ok(const sdm_ctx* c, int level);
int hog_checks(sdm_ctx* c, int level);
int launch_cells(sdm_ctx* c, int level);
int do_hog(sdm_ctx* c, int level);
int build_apply_planes(sdm_ctx* c, int level);
int do_apply(sdm_ctx* c, int level);
bool fused_ok(const sdm_ctx* c, int level);
int detect_level_fused(sdm_ctx* c, int l);
int detect_level(sdm_ctx* c, int l);
int solve_update_scratch(sdm_ctx* c, int ncols);      // (sdm_capi_train.hip)
int gram_rhs_rows(sdm_ctx* c, int level, int rows);   // (sdm_capi_train.hip)
int qr_solve(sdm_ctx* c, float* G, int ncols, int F, int Fp, int Mp, float* R_out);      // (sdm_capi_train.hip)
int shard_bcast_thunk(void* self, float* buf, size_t count, int root, hipStream_t stream);      // (sdm_capi_exchange.hip)
int shard_allgather_thunk(void* self, const float* send, float* recv, size_t count, hipStream_t stream);

}  // namespace sdm_capi
