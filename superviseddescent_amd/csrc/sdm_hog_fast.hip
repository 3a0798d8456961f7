// sdm_hog_fast.hip -- the production HOG kernel for gfx950 (resized ROI edge S <= 64).
//
// Same reference semantics as sdm_hog.hip (rcr::HogTransform::operator(), include/rcr/adaptive_vlhog.hpp:
// 109-185; vl_hog_put_image / vl_hog_extract, include/rcr/hog.c:595-728, 857-1062) and the same mapping
// (one 64-lane wavefront per (sample, landmark) patch, lane = pixel column), restructured around what the
// first profile showed (profiles/r01_*): the v1 kernel was bound by LDS float atomics (ds_add_f32 retires
// ONE lane per 3 cycles: 192 cycles per wave-instruction, measured with scripts/ubench/lds_atomic*.hip)
// and by ~11k VALU instructions per patch.
//
//  * crop + cv::resize + u8->f32 are fused into the gradient loop: every lane keeps the two previous resized rows of
//    its column in registers, left/right neighbours come through DPP wave shifts, the resized ROI never touches
//    LDS; the two source bytes of a lane's horizontal taps arrive as ONE 16-bit load per source row (requested two
//    output rows ahead), the horizontal pass is v_perm_b32 + v_dot2_u32_u16, the vertical pass two v_mul_hi_u32_u24;
//  * everything that depends only on the column (resize taps, cell index, bilinear weights) lives in registers for
//    the whole patch; everything that depends only on the row sits in a register of lane `row` and is moved to
//    scalar registers with v_readlane -- or, for the level constants, comes from the kernel arguments by scalar load;
//  * in the two atomic modes the histogram is padded by one cell on every side so that the four bilinear updates
//    need no bounds predicates;
//  * accumulation has three modes (template ACC):
//      ACC_EXACT_ORDER  ds_add_f32 in the reference's raster order -> histogram bit-identical to hog.c
//                       (what sdm_hog.hip does; kept for validation, ~3 cycles per contributing pixel);
//      ACC_FIXED64      every f32 contribution (g*wx)*wy is converted EXACTLY to 2^-36 fixed point (one
//                       v_fma_f64 "magic number" + mask) and summed with ds_add_u64 (16x faster than the
//                       float atomic); the sum is exact and order independent, converted back to f32 with
//                       ONE rounding.  Differs from the reference's sequentially rounded f32 sum by a few
//                       ulp at most; integer decisions (ROI geometry, resized bytes, bins) are identical.
//      ACC_COLUMNS      the spatial interpolation is separated: during the row loop lane x adds g*wy to ITS OWN
//                       pixel column [bin][x][band slot] -- a plain 8-byte LDS read / two f32 adds / write of the two
//                       cell rows (bands) the pixel row feeds, no atomics: nothing is shared between lanes, so the order
//                       is fixed and the result deterministic; the read-modify-write runs one pixel row behind the
//                       gradient.  Only two bands are live at a time (slot = band & 1): when the rows leave a band its
//                       columns are folded into cells, hist[bin][band][cx] = sum_x col[bin][x] * W[x][cx], as a
//                       (2O x 64) x (64 x 16) product on the matrix cores, and the slot is cleared for band + 2.  Same
//                       integer decisions; the f32 roundings happen in a different order ((sum_y g*wy)*wx instead of
//                       sum (g*wx)*wy).  Per wave this needs 2O*S*8 bytes of LDS instead of a histogram per lane group,
//                       which is what lets 6-7 waves per SIMD stay resident.
//  * the orientation arg-max uses the un-normalised gradient (gx*ox + gy*oy) when, for the level's
//    orientation count, that shortcut has been verified on the device to give the reference's bin for
//    EVERY possible pair of u8 central differences (511 x 511 inputs); otherwise the reference's
//    normalise-then-score arithmetic is used;
//  * blockIdx is remapped so that the 22/68 patches of one face run on one XCD (its image is then fetched
//    from HBM into one L2 instead of eight).
//
// Also here: verify_fast_bins_kernel / sdm_launch_verify_fast_bins, the exhaustive check of the fast arithmetic of BOTH families
// (it shares sqrt_int_exact and the un-normalised arg-max with this family only; the lane-packed kernel's forms it checks --
// raw v_sqrt_f32, the rotated octant code -- come from sdm_hog_device.h).  The lane-packed kernel is sdm_hog_packed.hip, its
// launch-plan builder sdm_hog_plan.hip.
#include "sdm_kernels.h"
#include "sdm_hog_device.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

#define HF_WAVES 4
#define HF_PREFETCH 2   /* rows in flight = rows per unrolled group (the slot of row y is y & 1) */
#define ACC_EXACT_ORDER 0
#define ACC_FIXED64 1
#define ACC_COLUMNS 2
// ACC_COLUMNS: the fold weights W[x][n] (n = patch * C + cell column, 16 columns) are the same for every patch of a
// launch; one copy per workgroup behind the waves' private regions
#define HF_WT_BYTES (64 * 16 * 4)

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// per-wave LDS layout.  Region A lives for the whole patch, region B is first the rolling private
// accumulators of the row loop and afterwards the scratch of the normalisation phase.
struct FastLds {
    void* hfin;       // A: fixed point: u64 [2O][CC] finished histogram; exact order: f32 [2O][PW][PW] (padded)
    u64* copies;      // B (row loop, fixed point): [2 band slots][2O][PW][R] private accumulators
    float* histv;     // B (after): [2O][CC] histogram as f32
    float* nrm;       // B: [CC]
    double* fac;      // B: [4][CC]
    double* hcc;      // B: [O][CC][4] clamped hc values for the texture sums
    float* desc;      // B: [D][CC]
};

// private accumulator copies per (band, bin, column): lane x uses copy x % 8, so no two lanes of one instruction that
// fall into the same cell column share an address (8 is also the 64-byte stride that lets the two column
// neighbours of a contribution sit in the immediate offset of the LDS instruction)
#define HF_COPIES 8
#define HF_TWO52_BITS 0x4330000000000000ull
// PAIR mode (two patches of one sample side by side in the two 32-lane halves of a wave, S <= 32) keeps 4 copies per
// half: half as many lanes map to a cell column
#define HF_COPIES_PAIR 4
__host__ __device__ inline int copies_R(bool pair) { return pair ? HF_COPIES_PAIR : HF_COPIES; }

__host__ __device__ inline size_t fast_region_a(int C, int O)
{
    const int CC = C * C, PW = C + 2;
    const size_t a_fixed = al16((size_t)2 * O * CC * 8), a_exact = al16((size_t)2 * O * PW * PW * 4);
    return a_fixed > a_exact ? a_fixed : a_exact;
}
__host__ __device__ inline size_t fast_copies_bytes(int C, int O, bool pair)
{
    return al16((size_t)2 * 2 * O * (C + 2) * copies_R(pair) * 8);
}

// ---- ACC_COLUMNS per-wave layout: [ column rows f32 [2O][ST][2 band slots] | later: nrm, fac, desc of the finish phase ]
//      [ finished histograms f32 [patches][2O][C*C] ] ----
// pixel columns folded per band (a multiple of 8: two MFMA k-steps of 4 columns per trip) and the stride between the
// column rows of two bins.  The stride is padded so that 2 * stride = 20 (mod 32) dwords: the fold reads the 16 bin rows of
// one pixel column with ONE ds_read_b32 (banks = dword mod 32) -- with the unpadded strides 56 / 40 / 64 the sixteen rows
// fell into 2 / 2 / 1 banks (8- and 16-way conflicts, 58 % of all LDS cycles in the round-1 counters), now into 8
// (2-way, which a 32-bit LDS access hides) -- and so that the row loop's per-lane 8-byte read-modify-write of [bin][x]
// (banks = dword mod 64) only collides for lanes >= 6 columns apart whose bins differ.
__host__ __device__ inline int fast_columns_k(int cell, int C, bool pair) { return pair ? 64 : ((C * cell + 7) & ~7); }
__host__ __device__ inline int fast_columns_stride(int cell, int C, bool pair)
{
    const int k = fast_columns_k(cell, C, pair);
    int st = k + 2;
    while ((2 * st) % 32 != 20 && (2 * st) % 32 != 12) st += 2;
    return st;
}
__host__ __device__ inline size_t fast_columns_rows_bytes(int cell, int C, int O, bool pair)
{
    return al16((size_t)2 * O * fast_columns_stride(cell, C, pair) * 8);
}
__host__ __device__ inline size_t fast_columns_scratch_bytes(int C, int D)
{
    return al16((size_t)C * C * 4) + al16((size_t)(C + 1) * (C + 1) * 8) + al16((size_t)D * C * C * 4);
}
__host__ __device__ inline size_t fast_columns_hist_off(int cell, int C, int O, int D, bool pair)
{
    const size_t a = fast_columns_rows_bytes(cell, C, O, pair), b = fast_columns_scratch_bytes(C, D);
    return a > b ? a : b;
}
__host__ __device__ inline size_t fast_columns_hist_bytes(int C, int O) { return al16((size_t)2 * O * C * C * 4); }

// region A (per patch: the finished histogram) x patches, then region B = max(accumulator copies x patches,
// normalisation scratch of ONE patch: the patches of a pair are normalised one after the other)
__host__ __device__ inline size_t fast_lds_bytes(int cell, int C, int O, int D, bool pair = false, bool columns = false)
{
    const int CC = C * C, np = pair ? 2 : 1;
    if (columns) return fast_columns_hist_off(cell, C, O, D, pair) + np * fast_columns_hist_bytes(C, O);
    const size_t b_rows = np * fast_copies_bytes(C, O, pair);
    const size_t b_norm = al16((size_t)2 * O * CC * 4) + al16((size_t)CC * 4) + al16((size_t)4 * CC * 8) +
                          al16((size_t)O * CC * 4 * 8) + al16((size_t)D * CC * 4);
    return np * fast_region_a(C, O) + (b_rows > b_norm ? b_rows : b_norm);
}
// dynamic LDS of one workgroup
__host__ __device__ inline size_t fast_wg_lds_bytes(int cell, int C, int O, int D, bool pair, bool columns)
{
    return fast_lds_bytes(cell, C, O, D, pair, columns) * HF_WAVES + (columns ? HF_WT_BYTES : 0);
}

__device__ inline FastLds fast_carve(unsigned char* base, int C, int O, int D, bool pair = false)
{
    const int CC = C * C;
    FastLds w;
    w.hfin = (void*)base;
    size_t o = (pair ? 2 : 1) * fast_region_a(C, O);
    w.copies = (u64*)(base + o);
    w.histv = (float*)(base + o); o += al16((size_t)2 * O * CC * 4);
    w.nrm = (float*)(base + o); o += al16((size_t)CC * 4);
    w.fac = (double*)(base + o); o += al16((size_t)4 * CC * 8);
    w.hcc = (double*)(base + o); o += al16((size_t)O * CC * 4 * 8);
    w.desc = (float*)(base + o);
    return w;
}

// sum and clear 2*N2 private accumulator copies of one (band, bin, column)
template <int N2>
__device__ inline u64 fold_copies(u64x2* c2)
{
    u64x2 q[N2];
#pragma unroll
    for (int i = 0; i < N2; ++i) q[i] = c2[i];
    const u64x2 z2 = {0ull, 0ull};
#pragma unroll
    for (int i = 0; i < N2; ++i) c2[i] = z2;
    u64 sum = 0;
#pragma unroll
    for (int i = 0; i < N2; ++i) sum += q[i].x + q[i].y;
    return sum;
}

// (a * b) >> 32 for a, b < 2^24 on the full-rate 24-bit multiplier; a is wave-uniform (scalar operand)
__device__ inline unsigned mul_hi_u24(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "s"(a), "v"(b));
    return r;
}

__device__ inline float lane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// ---- one finished histogram -> descriptor -> feature row segment (vl_hog_extract, hog.c:857-1062, and the Matlab-order
//      flatten of adaptive_vlhog.hpp:166-175).  `w` is the calling wave's scratch; hfin_p / histf_p the patch's finished
//      histogram (fixed point / exact order).  Runs on one wave. ----------------------------------------------------------
template <int ACC, int TO, int TC>
__device__ void hog_finish_patch(const FastLds& w, const u64* hfin_p, const float* histf_p, float* __restrict__ out_desc,
                                 const HogLevelDev& lv, int lane)
{
    const int O = TO ? TO : lv.O;
    const int C = TC ? TC : lv.C;
    const int CC = C * C, PW = C + 2, PWW = PW * PW;
    // ---- histogram -> f32 [2O][CC] (one conversion per accumulator; region B, dead since the last flush,
    //      becomes the scratch of the normalisation phase; region A is only read) ----------------------------
    for (int t = lane; t < 2 * O * CC; t += 64) {
        const int k = t / CC, c = t - k * CC;
        const int cyy = c / C, cxx = c - cyy * C;
        // fixed point: exact sum, ONE rounding (u64 -> f32), then the exact scale 2^-36
        w.histv[t] = (ACC == ACC_FIXED64)
                         ? (float)(__builtin_bit_cast(double, hfin_p[t]) - 4503599627370496.0) * 1.4551915228366852e-11f
                         : histf_p[k * PWW + (cyy + 1) * PW + (cxx + 1)];
    }
    wave_sync();

    // ---- cell norms (hog.c:875-890) ---------------------------------------------------------------------------
    for (int c = lane; c < CC; c += 64) {
        float n = 0.0f;
        for (int k = 0; k < O; ++k) {
            const float hs = w.histv[c + k * CC] + w.histv[c + (k + O) * CC];
            n += hs * hs;
        }
        w.nrm[c] = n;
    }
    wave_sync();
    // ---- block factors (hog.c:930-981).  The four factors of a cell are those of the 2x2-cell blocks around its four
    //      corners, clamped at the border; a block is shared by up to four cells, so the (C+1)^2 distinct ones are
    //      computed once: block (bx, by) sums cells (xa,ya) (xb,ya) (xa,yb) (xb,yb), left to right, + 1e-4 last, with
    //      xa = max(bx-1, 0), xb = min(bx, C-1) -- the same operands in the same order as the reference's n1..n9 ----
    const int CB = C + 1;
    for (int t = lane; t < CB * CB; t += 64) {
        const int byb = t / CB, bxb = t - byb * CB;
        const int xa = bxb - 1 > 0 ? bxb - 1 : 0, xb = bxb < C - 1 ? bxb : C - 1;
        const int ya = byb - 1 > 0 ? byb - 1 : 0, yb = byb < C - 1 ? byb : C - 1;
        const double na = w.nrm[xa + ya * C], nb = w.nrm[xb + ya * C];
        const double nc = w.nrm[xa + yb * C], nd = w.nrm[xb + yb * C];
        w.fac[t] = 1.0 / sqrt(na + nb + nc + nd + 1e-4);
    }
    wave_sync();
    // ---- normalise, clamp, emit the 3 (UoCTTI) or 4 (Dalal-Triggs) outputs of every (cell, orientation) ------
    //      desc is written in the Matlab order of the feature row (adaptive_vlhog.hpp:166-175): [dim][x][y]
    for (int t = lane; t < O * CC; t += 64) {
        const int k = t / CC, c = t - k * CC;
        const int y = c / C, x = c - y * C, ct = x * C + y;
        const double ha = w.histv[c + k * CC], hb = w.histv[c + (k + O) * CC];
        // j=0: n1+n2+n4+n5  j=1: n2+n3+n5+n6  j=2: n4+n5+n7+n8  j=3: n5+n6+n8+n9
        const double f1 = w.fac[x + y * CB], f2 = w.fac[x + 1 + y * CB];
        const double f3 = w.fac[x + (y + 1) * CB], f4 = w.fac[x + 1 + (y + 1) * CB];
        double ha1 = f1 * ha, ha2 = f2 * ha, ha3 = f3 * ha, ha4 = f4 * ha;
        double hb1 = f1 * hb, hb2 = f2 * hb, hb3 = f3 * hb, hb4 = f4 * hb;
        double hc1 = ha1 + hb1, hc2 = ha2 + hb2, hc3 = ha3 + hb3, hc4 = ha4 + hb4;
#define CL02(v) __builtin_fmin(0.2, (v))          /* VL_MIN(0.2, v): the values are finite and non-negative */
        ha1 = CL02(ha1); ha2 = CL02(ha2); ha3 = CL02(ha3); ha4 = CL02(ha4);
        hb1 = CL02(hb1); hb2 = CL02(hb2); hb3 = CL02(hb3); hb4 = CL02(hb4);
        hc1 = CL02(hc1); hc2 = CL02(hc2); hc3 = CL02(hc3); hc4 = CL02(hc4);
#undef CL02
        if (lv.variant == 1) {
            w.desc[ct + k * CC] = (float)(0.5 * (ha1 + ha2 + ha3 + ha4));
            w.desc[ct + (k + O) * CC] = (float)(0.5 * (hb1 + hb2 + hb3 + hb4));
            w.desc[ct + (k + 2 * O) * CC] = (float)(0.5 * (hc1 + hc2 + hc3 + hc4));
            double* q = w.hcc + (size_t)(k * CC + c) * 4;
            q[0] = hc1; q[1] = hc2; q[2] = hc3; q[3] = hc4;
        } else {
            w.desc[ct + k * CC] = (float)hc1;
            w.desc[ct + (k + O) * CC] = (float)hc2;
            w.desc[ct + (k + 2 * O) * CC] = (float)hc3;
            w.desc[ct + (k + 3 * O) * CC] = (float)hc4;
        }
    }
    wave_sync();
    // ---- texture features: t_j = sum over k (in order) of the clamped hc_j (hog.c:1020-1023, 1047-1052) ------
    if (lv.variant == 1) {
        const float tex = 1.0f / sqrtf(18.0f);
        for (int t = lane; t < 4 * CC; t += 64) {
            const int j = t / CC, c = t - j * CC;
            const int y = c / C, x = c - y * C, ct = x * C + y;
            double acc = 0.0;
            for (int k = 0; k < O; ++k) acc += w.hcc[(size_t)(k * CC + c) * 4 + j];
            w.desc[ct + (3 * O + j) * CC] = (float)(tex * acc);
        }
        wave_sync();
    }
    // ---- the feature row segment of this landmark: desc is already in its order -------------------------------
    for (int o = lane; o < lv.P; o += 64) out_desc[o] = w.desc[o];
    wave_sync();   // the caller may reuse the scratch for the next patch
}

// ---- ACC_COLUMNS finish: the same arithmetic as hog_finish_patch on a third of its scratch.  hist = f32 [2O][C*C] (cell
//      index cy*C + cx) as the folds left it; nrm / fac / desc overlay the dead column rows; the texture sums recompute
//      their clamped terms instead of staging them (O products per output).  FT: the arithmetic type of hog.c:930-1052
//      (double). ---------------------------------------------------------------------------------------------------
template <int TO, int TC, typename FT>
__device__ void hog_finish_lean(const float* hist, unsigned char* scratch, float* __restrict__ out_desc,
                                const HogLevelDev& lv, int lane)
{
    const int O = TO ? TO : lv.O;
    const int C = TC ? TC : lv.C;
    const int CC = C * C, CB = C + 1;
    float* nrm = (float*)scratch;
    FT* fac = (FT*)(scratch + al16((size_t)CC * 4));
    float* desc = (float*)(scratch + al16((size_t)CC * 4) + al16((size_t)CB * CB * 8));
    // ---- cell norms (hog.c:875-890) ---------------------------------------------------------------------------
    for (int c = lane; c < CC; c += 64) {
        float n = 0.0f;
        for (int k = 0; k < O; ++k) {
            const float hs = hist[c + k * CC] + hist[c + (k + O) * CC];
            n += hs * hs;
        }
        nrm[c] = n;
    }
    wave_sync();
    // ---- block factors (hog.c:930-981): see hog_finish_patch ------------------------------------------------------
    for (int t = lane; t < CB * CB; t += 64) {
        const int byb = t / CB, bxb = t - byb * CB;
        const int xa = bxb - 1 > 0 ? bxb - 1 : 0, xb = bxb < C - 1 ? bxb : C - 1;
        const int ya = byb - 1 > 0 ? byb - 1 : 0, yb = byb < C - 1 ? byb : C - 1;
        const FT na = nrm[xa + ya * C], nb = nrm[xb + ya * C];
        const FT nc = nrm[xa + yb * C], nd = nrm[xb + yb * C];
        fac[t] = (FT)1.0 / (FT)sqrt(na + nb + nc + nd + (FT)1e-4);
    }
    wave_sync();
#define CL02(v) (sizeof(FT) == 8 ? (FT)__builtin_fmin(0.2, (double)(v)) : (FT)__builtin_fminf(0.2f, (float)(v)))          /* VL_MIN(0.2, v): the values are finite and non-negative */
    // ---- normalise, clamp, emit the 3 (UoCTTI) or 4 (Dalal-Triggs) outputs of every (cell, orientation), in the Matlab
    //      order of the feature row (adaptive_vlhog.hpp:166-175): [dim][x][y] ---------------------------------------
    for (int t = lane; t < O * CC; t += 64) {
        const int k = t / CC, c = t - k * CC;
        const int y = c / C, x = c - y * C, ct = x * C + y;
        const FT ha = hist[c + k * CC], hb = hist[c + (k + O) * CC];
        const FT f1 = fac[x + y * CB], f2 = fac[x + 1 + y * CB];
        const FT f3 = fac[x + (y + 1) * CB], f4 = fac[x + 1 + (y + 1) * CB];
        FT ha1 = f1 * ha, ha2 = f2 * ha, ha3 = f3 * ha, ha4 = f4 * ha;
        FT hb1 = f1 * hb, hb2 = f2 * hb, hb3 = f3 * hb, hb4 = f4 * hb;
        FT hc1 = ha1 + hb1, hc2 = ha2 + hb2, hc3 = ha3 + hb3, hc4 = ha4 + hb4;
        ha1 = CL02(ha1); ha2 = CL02(ha2); ha3 = CL02(ha3); ha4 = CL02(ha4);
        hb1 = CL02(hb1); hb2 = CL02(hb2); hb3 = CL02(hb3); hb4 = CL02(hb4);
        hc1 = CL02(hc1); hc2 = CL02(hc2); hc3 = CL02(hc3); hc4 = CL02(hc4);
        if (lv.variant == 1) {
            desc[ct + k * CC] = (float)((FT)0.5 * (ha1 + ha2 + ha3 + ha4));
            desc[ct + (k + O) * CC] = (float)((FT)0.5 * (hb1 + hb2 + hb3 + hb4));
            desc[ct + (k + 2 * O) * CC] = (float)((FT)0.5 * (hc1 + hc2 + hc3 + hc4));
        } else {
            desc[ct + k * CC] = (float)hc1;
            desc[ct + (k + O) * CC] = (float)hc2;
            desc[ct + (k + 2 * O) * CC] = (float)hc3;
            desc[ct + (k + 3 * O) * CC] = (float)hc4;
        }
    }
    // ---- texture features: t_j = sum over k (in order) of the clamped hc_j (hog.c:1020-1023, 1047-1052) ------
    if (lv.variant == 1) {
        const float tex = 1.0f / sqrtf(18.0f);
        for (int t = lane; t < 4 * CC; t += 64) {
            const int j = t / CC, c = t - j * CC;
            const int y = c / C, x = c - y * C, ct = x * C + y;
            const FT fj = fac[x + (j & 1) + (y + (j >> 1)) * CB];
            FT acc = 0;
            for (int k = 0; k < O; ++k) {
                const FT ha = hist[c + k * CC], hb = hist[c + (k + O) * CC];
                const FT haj = fj * ha, hbj = fj * hb;
                acc += CL02(haj + hbj);
            }
            desc[ct + (3 * O + j) * CC] = (float)(tex * acc);
        }
    }
#undef CL02
    wave_sync();
    // ---- the feature row segment of this landmark: desc is already in its order -------------------------------
    for (int o = lane; o < lv.P; o += 64) out_desc[o] = desc[o];
    wave_sync();   // the next patch of a pair reuses the scratch
}

// TO / TC: compile-time orientation count / cell count (0 = take the run-time value from lv)
// PAIR: landmarks `landmark` and `landmark + 1` of the same sample side by side in lanes 0-31 / 32-63 (S <= 32).  They
// share the image, the IED, hence h, the scale and every per-coordinate table; only the patch centre differs, which
// turns the row addresses and the vertical border masks into per-lane values.  `second_valid` is false for the last,
// single landmark of an odd count (its half then carries zero weights and stores nothing).
template <int ACC, int FASTBIN, int TO, int TC, bool PAIR, bool PROF = false>
__device__ void hog_patch_fast(const ImageSetDev& imgs, int im_in, const float* __restrict__ xr, int L, int landmark,
                               bool second_valid, const EyeIdxDev& eyes, const HogLevelDev& lv, unsigned char* lds_base,
                               float* __restrict__ out_row, int* idx_row, int* status,
                               unsigned long long* prof = nullptr, float* wt = nullptr, bool valid = true)
{
    long long tprev = PROF ? clock64() : 0;
    auto mark = [&](int slot) {
        if (PROF) {
            const long long t = clock64();
            if ((threadIdx.x & 63) == 0) atomicAdd(&prof[slot], (unsigned long long)(t - tprev));
            tprev = t;
        }
    };
    const int lane = threadIdx.x & 63;
    const int S = lv.S, cell = lv.cell, D = lv.D;
    const int O = TO ? TO : lv.O;
    const int C = TC ? TC : lv.C;
    const int CC = C * C, PW = C + 2, PWW = PW * PW;
    constexpr int NP = PAIR ? 2 : 1;
    const int half = PAIR ? (lane >> 5) : 0, col = PAIR ? (lane & 31) : lane;
    FastLds w = fast_carve(lds_base, C, O, D, PAIR);
    const size_t a_bytes = fast_region_a(C, O);                 // per patch: finished histogram
    const size_t copies_u64 = fast_copies_bytes(C, O, PAIR) / 8;   // per patch: accumulator copies
    float* histf = (float*)((unsigned char*)w.hfin + (size_t)half * a_bytes);   // exact order: this lane's padded f32 histogram
    constexpr int R = PAIR ? HF_COPIES_PAIR : HF_COPIES;
    constexpr bool NOMASK = (TC == 5);   // 5 cells and S <= 64: cell <= 12 (checked again by the launcher)

    // ---- patch geometry (wave-uniform, moved to scalar registers; adaptive_vlhog.hpp:123,132-133) ------
    const int h = lv.fixed_h > 0 ? lv.fixed_h : uni((int)round((double)lv.rel * ied_of(xr, L, eyes) / 2));
    const int lmB = (PAIR && second_valid) ? landmark + 1 : landmark;
    const int cxA = uni(__float2int_rn(xr[landmark])), cyA = uni(__float2int_rn(xr[landmark + L]));
    const int cxB = uni(__float2int_rn(xr[lmB])), cyB = uni(__float2int_rn(xr[lmB + L]));
    if (idx_row && lane == 0) {
        if (landmark == 0) idx_row[0] = h;
        idx_row[1 + landmark] = cxA; idx_row[1 + L + landmark] = cyA;
        if (PAIR && second_valid) { idx_row[1 + lmB] = cxB; idx_row[1 + L + lmB] = cyB; }
    }
    const int cx = half ? cxB : cxA, cy = half ? cyB : cyA;     // (per lane in PAIR mode, scalar otherwise)
    const bool empty = h <= 0;
    if (empty && lane == 0) atomicOr(status, SDM_DEV_ERR_EMPTY_PATCH);
    const int sw = empty ? 1 : 2 * h;
    const int x0 = cx - h, y0 = cy - h;
    const bool area2 = (sw == 2 * S);   // both scales exactly 2: INTER_LINEAR is redirected to the 2x2 box average
    // (the f64 divisions of cv::resize's scale come from a per-level table in the kernel arguments: one scalar load)
    const double scale = (h < SDM_SCALE_TAB) ? lv.scale_tab[h > 0 ? h : 0] : 1.0 / ((double)S / (double)sw);

    const int im = uni(im_in);
    const uint8_t* img = imgs.base + imgs.offset[im];
    const int iw = imgs.w[im], ih = imgs.h[im], istride = imgs.stride[im];

    // ---- per-coordinate values: lane d computes coordinate d once.  The COLUMN copy stays in this lane's
    //      registers; the ROW copy of coordinate yy is fetched from lane yy with v_readlane (no LDS) -----------
    const int d = col < S ? col : S - 1;
    int bxc; float wx1, wx2;          // HOG cell index / bilinear weights of coordinate d   (hog.c:697-704)
    int row_src, row_beta;            // vertical resize taps of coordinate d (packed)
    int px0, px1, a0, a1;             // horizontal resize taps of column d (image columns, masked weights)
    int pl; unsigned wpk;             // ... as ONE 16-bit load at column pl with the weights of its two bytes packed
    {
        // hog.c:697-704 per coordinate: hx = (d + 0.5) / cell - 0.5, cell floor(hx), weights hx - floor(hx) and its
        // complement -- level constants, computed by the host with the same arithmetic (sdm_set_model_geometry)
        bxc = __builtin_bit_cast(int, lv.row_tab[d][2]);
        wx2 = lv.row_tab[d][3];
        wx1 = (float)(1.0 - wx2);
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s = (int)floorf(f);
        f -= (float)s;
        const int c0 = sat_short_f((1.f - f) * 2048.0f), c1 = sat_short_f(f * 2048.0f);
        // vertical taps: clip the ROWS, keep the fraction
        int sy0 = s < 0 ? 0 : (s > sw - 1 ? sw - 1 : s);
        int sy1 = s + 1 < 0 ? 0 : (s + 1 > sw - 1 ? sw - 1 : s + 1);
        if (area2) { sy0 = 2 * d; sy1 = 2 * d + 1; }
        row_src = sy0 | (sy1 << 16);
        row_beta = area2 ? (1024 | (1024 << 16)) : ((c0 & 0xffff) | (c1 << 16));
        if (!PAIR) {
            // one patch per wave: the patch origin is wave-uniform, so the image rows of the two taps are final here -- clamped
            // into the image (< 2^16 rows, checked by the host), a row on the black canvas keeps its address but loses its weight
            int py0 = (cy - h) + sy0, py1 = (cy - h) + sy1;
            if (py0 < 0 || py0 >= ih) row_beta &= 0xffff0000;
            if (py1 < 0 || py1 >= ih) row_beta &= 0x0000ffff;
            py0 = py0 < 0 ? 0 : (py0 > ih - 1 ? ih - 1 : py0);
            py1 = py1 < 0 ? 0 : (py1 > ih - 1 ? ih - 1 : py1);
            row_src = py0 | (py1 << 16);
        }
        // horizontal taps: clamped in the table
        int sx = s;
        a0 = c0; a1 = c1;
        if (sx < 0) { sx = 0; a0 = 2048; a1 = 0; }
        if (sx >= sw - 1) { sx = sw - 1; a0 = 2048; a1 = 0; }
        // exact 2x reduction (INTER_AREA 2x2 box): with all four weights 1024 the bilinear fixed-point formula below gives
        // exactly (p00 + p01 + p10 + p11 + 2) >> 2 -- (1024 * (1024 * s >> 4)) >> 16 = s -- so the row loop needs no second form
        if (area2) { sx = 2 * d; a0 = 1024; a1 = 1024; }
        const int sx1 = (sx + 1 < sw) ? sx + 1 : sx;
        px0 = x0 + sx; px1 = x0 + sx1;
        // columns on the black canvas (or an empty patch) get weight 0 instead of a per-row mask
        if (px0 < 0 || px0 >= iw || empty) a0 = 0;
        if (px1 < 0 || px1 >= iw || empty) a1 = 0;
        px0 = px0 < 0 ? 0 : (px0 > iw - 1 ? iw - 1 : px0);
        px1 = px1 < 0 ? 0 : (px1 > iw - 1 ? iw - 1 : px1);
        // Two live taps are neighbours (px1 = px0 + 1): one 16-bit load at px0.  A single live tap p is paired with a
        // zero-weight neighbour INSIDE the row (the load never crosses the end of the row, hence never the end of the image).
        if (a0 != 0 && a1 != 0) {
            pl = px0; wpk = (unsigned)a0 | ((unsigned)a1 << 16);
        } else {
            const int p = a0 != 0 ? px0 : px1;
            const unsigned wt = (unsigned)(a0 != 0 ? a0 : a1);
            if (p + 1 <= iw - 1 || p == 0) { pl = p; wpk = wt; }       // (p == 0 in a 1-pixel-wide image: see sdm_capi, not used)
            else { pl = p - 1; wpk = wt << 16; }
        }
    }
    const float row_w1 = wx1, row_w2 = wx2;   // weights of coordinate d when it is used as a ROW
    const int row_cell = bxc;
    const bool col_active = (col >= 1) && (col < S - 1) && (!PAIR || half == 0 || second_valid);
    // padded histogram column of this lane (lanes outside the ROI contribute exact zeros to cell 0)
    const int hcol = col_active ? bxc + 1 : 0;
    if (!col_active) { wx1 = 0.0f; wx2 = 0.0f; }

    mark(0);   // geometry + per-coordinate tables
    float* colrows = (float*)lds_base;      // ACC_COLUMNS: [2O][ST][2 band slots]
    const int ST = fast_columns_stride(cell, C, PAIR), KST = fast_columns_k(cell, C, PAIR);
    float* chist = (float*)(lds_base + fast_columns_hist_off(cell, C, O, D, PAIR));    // [patch][2O][CC]
    const int chist_stride = (int)(fast_columns_hist_bytes(C, O) / 4);
    if (ACC == ACC_COLUMNS) {
        const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = lane; i < (int)(fast_columns_rows_bytes(cell, C, O, PAIR) / 16); i += 64) ((f32x4*)colrows)[i] = z4;
        for (int i = lane; i < NP * chist_stride / 4; i += 64) ((f32x4*)chist)[i] = z4;
        // the fold weights of coordinate x = this lane: W[x][patch * C + cell] = wx1 for cell(x), wx2 for cell(x) + 1
        // (hog.c:697-704), 0 elsewhere and for the columns outside the ROI interior.  Pure level geometry: the four waves
        // of the workgroup write identical tables, and the barrier orders every write before the first fold.
        float* wrow = wt + lane * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) ((f32x4*)wrow)[i] = z4;
        if (col >= 1 && col < S - 1) {
            const int nb = half * C;
            if (bxc >= 0) wrow[nb + bxc] = row_w1;              // (the unmasked weights: wx1 / wx2 are zeroed per patch)
            if (bxc + 1 <= C - 1) wrow[nb + bxc + 1] = row_w2;
        }
        __syncthreads();
        if (!valid) return;
    } else if (ACC == ACC_FIXED64) {
        // (16-byte stores: both counts are even and both regions 16-byte aligned)
        const u64x2 z2 = {0ull, 0ull};
        for (int i = lane; i < NP * 2 * O * PW * R; i += 64) ((u64x2*)w.copies)[i] = z2;
        const u64x2 b2 = {HF_TWO52_BITS, HF_TWO52_BITS};   // = 0.0 in the biased form the fold stores (see flush_band)
        for (int hp = 0; hp < NP; ++hp)
            for (int i = lane; i < O * CC; i += 64) ((u64x2*)((unsigned char*)w.hfin + (size_t)hp * a_bytes))[i] = b2;
    } else {
        for (int hp = 0; hp < NP; ++hp)
            for (int i = lane; i < 2 * O * PWW; i += 64) ((float*)((unsigned char*)w.hfin + (size_t)hp * a_bytes))[i] = 0.0f;
    }
    wave_sync();
    mark(1);   // histogram clear + barrier
    // fixed point: the two cell-row bands (by, by+1) a pixel row feeds are accumulated in private copies (no two
    // lanes of one instruction share an address); a band is folded into hfin when the rows have moved past it
    const int lane_off = hcol * R + col % R + half * (int)copies_u64;   // (+ this half's accumulator region)
    int cur_by = -2;
    auto flush_band = [&](int band) {
        const int slot = band & 1;
        for (int hp = 0; hp < NP; ++hp) {
            u64* hfin = (u64*)((unsigned char*)w.hfin + (size_t)hp * a_bytes);
            for (int t = lane; t < 2 * O * PW; t += 64) {
                u64* cp = w.copies + (size_t)hp * copies_u64 + (size_t)(slot * 2 * O * PW + t) * R;
                // all 16-byte reads in flight, then the clears (integer sum: any order)
                const u64 sum = fold_copies<R / 2>((u64x2*)cp) & 0xfffffffffffffull;   // (see fx: bits >= 52 are not data)
                const int kbin = t / PW, hc = t - kbin * PW;
                // stored as the bit pattern of the double 2^52 + sum (sum < 2^52), which makes the final u64 -> f32
                // conversion one f64 subtraction and one (single) rounding
                if (band >= 0 && band < C && hc >= 1 && hc <= C) hfin[kbin * CC + band * C + (hc - 1)] = sum | HF_TWO52_BITS;
            }
        }
    };

    // ---- fused crop + resize + gradient + accumulation, one output row per iteration -------------------
    // issue: the four source bytes of output row y (two clipped source rows x two horizontal taps)
    // the image as a raw buffer: per-lane byte offset (column) in the vector offset, the row offset in a scalar
    // register -> no per-row vector address arithmetic at all
    const __amdgpu_buffer_rsrc_t img_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)img, 0, ih * istride, 0x00020000);
    // PAIR: y0 differs between the halves, so the row offset cannot sit in the scalar operand.  Each lane keeps
    // px + y0 * stride (possibly negative) and adds the scalar row term; rows above or below the image then fall outside
    // the buffer's num_records and the hardware range check returns 0 -- the black canvas -- without any clamp or mask.
    const int vb = PAIR ? pl + y0 * istride : 0;
    auto issue_row = [&](int y, unsigned short& q0, unsigned short& q1, int& bb) {
        // (rows past the last one -- the pipeline's harmless extra loads -- need no clamp: v_readlane takes the lane index
        // modulo 64 and every lane holds the taps of a valid row)
        const int yy = y;
        const int src = __builtin_amdgcn_readlane(row_src, yy);
        int beta = __builtin_amdgcn_readlane(row_beta, yy);
        if (PAIR) {
            const int r0 = (src & 0xffff) * istride, r1 = (src >> 16) * istride;     // scalar
            q0 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + r0, 0, 0);
            q1 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + r1, 0, 0);
        } else {
            // (image rows, clamped into the image and with the weight of a row on the black canvas already 0: see row_src)
            q0 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, pl, (src & 0xffff) * istride, 0);
            q1 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, pl, (int)((unsigned)src >> 16) * istride, 0);
        }
        bb = beta;
    };
    // horizontal pass of one output row: byte0 * w0 + byte1 * w1 per source row (the loaded registers are dead afterwards
    // and take a later row)
    unsigned spread_sel = HF_SPREAD_SEL;
    asm volatile("" : "+v"(spread_sel));      // (kept in a register: v_perm_b32 takes no literal selector)
    const u16x2 wpk2 = __builtin_bit_cast(u16x2, wpk);
    auto horizontal = [&](unsigned short q0, unsigned short q1, int& H0, int& H1) {
        H0 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, spread_bytes(q0, spread_sel)), wpk2, 0u, false);
        H1 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, spread_bytes(q1, spread_sel)), wpk2, 0u, false);
    };
    auto vertical = [&](int H0, int H1, int beta) -> float {
        // (b * (H >> 4)) >> 16 as the high half of the 48-bit product (b << 12) * (H & ~15): b <= 2048 and H < 2^19, so
        // both operands fit the full-rate 24-bit multiplier and the separate shifts disappear
        const unsigned b0 = (unsigned)(beta & 0xffff) << 12, b1 = (unsigned)(beta >> 16) << 12;      // scalar
        const int out = (int)((mul_hi_u24(b0, (unsigned)H0 & ~15u) + mul_hi_u24(b1, (unsigned)H1 & ~15u) + 2u) >> 2);
        return (float)out;      // convertTo(CV_32F), adaptive_vlhog.hpp:157
    };

    double two52 = 4503599627370496.0;   // 2^52, kept in a register pair for the fixed-point conversion
    asm volatile("" : "+v"(two52));       // (opaque to the optimiser so that it is not re-materialised per use)
    float rm2 = 0.0f, rm1 = 0.0f;       // resized rows y-2, y-1 of this lane's column
    // ACC_COLUMNS: the contribution of the previous pixel row, added while this row's gradient is computed
    // (lanes beyond the ROI share column 0, which is never active: its sums are finite garbage with fold weight 0)
    const unsigned col_off = (unsigned)(PAIR ? lane : (col < S ? col : 0)) * 8u;
    const unsigned bin_stride = (unsigned)(ST * 8);
    unsigned col_off1 = col_off + bin_stride;      // (opaque: the select between the two bases is then ONE v_cndmask)
    asm volatile("" : "+v"(col_off1));
    f32x2* pend_p = (f32x2*)((unsigned char*)colrows + col_off);
    f32x2 pend_v = {0.0f, 0.0f};
    int prev_by = -1;
    // fold band b (slot b & 1) into the cells of cell row b, then clear the slot for band b + 2.  v_mfma_f32_16x16x4_f32:
    // lane (li, lq) feeds A[row li][k lq] = col[bin li][x = 4 ks + lq], B[k lq][col li] = W[x][li] and receives
    // D[row 4 lq + e][col li]; two accumulators per tile halve the dependent chain.
    auto fold_band = [&](const int b) __attribute__((always_inline)) {
        constexpr int NTB = (2 * TO + 15) / 16 > 0 ? (2 * TO + 15) / 16 : 1;
        const int sl = b & 1;
        const int li = lane & 15, lq = lane >> 4;
        wave_sync();
        f32x4 fa[NTB][2];
        const float* ap[NTB];
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
            fa[t][0] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f}; fa[t][1] = fa[t][0];
            const int br = 16 * t + li;
            ap[t] = colrows + ((br < 2 * O ? br : 2 * O - 1) * ST + lq) * 2 + sl;
        }
        const float* bp = wt + lq * 16 + li;
        // (ST is a multiple of 8: an even number of k steps, two per trip, one accumulator each; a plain counted loop keeps
        // the accumulators in place -- guarding unrolled steps individually makes the compiler shuttle them through VGPRs)
        for (int kp = 0; kp < KST / 8; ++kp) {
            const float bw0 = bp[0], bw1 = bp[64];
#pragma unroll
            for (int t = 0; t < NTB; ++t) {
                float* a = const_cast<float*>(ap[t]);
                const float a0v = a[0], a1v = a[8];
                // one patch per wave: clear what was just read (the LDS unit executes a wave's instructions in order).  The
                // 16 rows x 4 + 4 columns of a step pair are exactly the slot's entries of these 8 pixel columns; rows beyond 2O
                // repeat the last bin.  (With the compile-time 64 columns of a landmark pair the loop is unrolled and the
                // stores would serialise the operand reads: there the slot is cleared afterwards.)
                if (!PAIR) { a[0] = 0.0f; a[8] = 0.0f; }
                fa[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0v, bw0, fa[t][0], 0, 0, 0);
                fa[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, bw1, fa[t][1], 0, 0, 0);
                ap[t] += 16;
            }
            bp += 128;
        }
        if (PAIR)
            for (int i = lane; i < 2 * O * ST; i += 64) colrows[2 * i + sl] = 0.0f;
        const int hp_n = li / C, cx_n = li - hp_n * C;
        if (hp_n < NP) {
            float* hf = chist + hp_n * chist_stride + b * C + cx_n;
#pragma unroll
            for (int t = 0; t < NTB; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int br = 16 * t + 4 * lq + e;
                    if (br < 2 * O) hf[br * CC] = fa[t][0][e] + fa[t][1][e];
                }
        }
        wave_sync();
    };
    // Rows are processed in pairs: each row's two source loads and the two previous resized rows stay in fixed registers (no
    // rotation copies), the pair is one straight-line block the scheduler can interleave (row y+1's resize does not depend on
    // row y's gradient), and the loads of row y+2 are issued as soon as row y's bytes are consumed.  (Deeper prefetch
    // measures the same: the loop is bound by instruction issue, not by the load latency.)
    constexpr int PD = HF_PREFETCH;
    unsigned short q0[PD], q1[PD];
    int qbeta[PD];
#pragma unroll
    for (int j = 0; j < PD; ++j) issue_row(j, q0[j], q1[j], qbeta[j]);
    auto row_step = [&](const int j, const int y, const bool grad) __attribute__((always_inline)) {
        int H0, H1;
        horizontal(q0[j], q1[j], H0, H1);
        const int cbeta = qbeta[j];
        issue_row(y + PD, q0[j], q1[j], qbeta[j]);      // (past the last row: a harmless reload of row S-1)
        f32x2 qv = {0.0f, 0.0f};
        if (ACC == ACC_COLUMNS && grad) qv = *pend_p;     // (in flight during the arithmetic below)
        const float r0 = vertical(H0, H1, cbeta);
        if (grad) {
            // gradient of row yy = y-1 (hog.c:616-672)
            const int yy = y - 1;
            const float gx = from_right(rm1) - from_left(rm1);
            const float gy = r0 - rm2;
            const float g2 = gx * gx + gy * gy;
            float g = FASTBIN == 2 ? sqrt_int_up(g2) : (FASTBIN == 1 ? sqrt_int_exact(g2) : sqrtf(g2));
            int bin;
            unsigned bin_off = 0;      // ACC_COLUMNS: byte offset of the bin's column row
            if (FASTBIN == 2 && TO == 4 && ACC == ACC_COLUMNS) {
                // 4 orientations = 8 directed bins of 45 degrees: the three bits of the bin as lane masks (the compiler keeps
                // them in scalar registers and combines them on the scalar unit), see bin_sector4_bits
                bool b0 = false, b1 = false, b2 = false;
                int bin_any = 0;
                if constexpr (TO == 4) bin_sector4_bits(gx, gy, lv, b0, b1, b2);
                else bin_sector<TO>(gx, gy, lv, TO, bin_any);      // (a zero gradient lands in bin 0 with magnitude 0)
                bin_off = (b0 ? col_off1 : col_off) + (b1 ? 2u * bin_stride : 0u) + (b2 ? 4u * bin_stride : 0u);
                bin = 0;
            } else if (FASTBIN == 2) {
                bin_sector<TO>(gx, gy, lv, O, bin);
            } else if (FASTBIN == 1) {
                float best = 0.0f;
                bin = -1;
#pragma unroll
                for (int k = 0; k < (TO ? TO : SDM_MAX_ORIENT); ++k) {
                    if (TO == 0 && k >= O) break;
                    float sc = __builtin_fmaf(gx, lv.ox[k], gy * lv.oy[k]);
                    const int bsel = sc < 0 ? k + O : k;
                    sc = __builtin_fabsf(sc);
                    if (sc > best) { best = sc; bin = bsel; }
                }
            } else {
                const float nx = g > 0.0f ? gx / g : 0.0f;
                const float ny = g > 0.0f ? gy / g : 0.0f;
                float best = 0.0f;
                bin = -1;
#pragma unroll
                for (int k = 0; k < (TO ? TO : SDM_MAX_ORIENT); ++k) {
                    if (TO == 0 && k >= O) break;
                    float sc = nx * lv.ox[k] + ny * lv.oy[k];
                    int bsel = k;
                    if (sc < 0) { sc = -sc; bsel += O; }
                    if (sc > best) { best = sc; bin = bsel; }
                }
            }
            // lanes outside the ROI carry wx1 = wx2 = 0 and the sector form always yields a valid bin: nothing to mask
            if (FASTBIN != 2 && (!col_active || bin < 0)) { g = 0.0f; bin = 0; }
            const int by = __builtin_amdgcn_readlane(row_cell, yy);
            const float wy1 = lane_f(row_w1, yy), wy2 = lane_f(row_w2, yy);
            if (ACC == ACC_COLUMNS) {
                *pend_p = qv + pend_v;
                // the row's level constants come from the kernel arguments with one scalar load (no cross-lane reads)
                const float* rt = lv.row_tab[yy];
                const float ws0 = rt[0], ws1 = rt[1];
                const int cby = __builtin_bit_cast(int, rt[2]);
                // the rows entered the next band (wave-uniform): the one they left is complete
                if (cby != prev_by) {
                    if (prev_by >= 0) fold_band(prev_by);
                    prev_by = cby;
                }
                // this row: g * (slot weights) into the two band slots of this lane's own column, next iteration
                // (24-bit multiply-add on the bin + the lane's byte offset)
                if (FASTBIN == 2 && TO == 4) pend_p = (f32x2*)((unsigned char*)colrows + bin_off);
                else pend_p = (f32x2*)((unsigned char*)colrows + (__umul24((unsigned)bin, bin_stride) + col_off));
                pend_v = (f32x2){ws0, ws1} * g;
            } else {
            // (grad * wx) * wy, hog.c:714-723: six f32 products as three packed multiplies
            const f32x2 t = (f32x2){wx2, wx1} * g;
            const f32x2 ab = t * wy1, cd = t * wy2;
            const float va = ab.x, vb = ab.y, vc = cd.x, vd = cd.y;
            if (ACC == ACC_FIXED64) {
                if (by != cur_by) {          // wave-uniform: the rows entered the next cell-row band
                    if (cur_by != -2) flush_band(cur_by);
                    cur_by = by;
                }
                // exact f32 -> 2^-36 fixed point: fma(v, 2^36, 2^52) leaves the integer in the low 52 mantissa bits
                // The high dword keeps the exponent bits of 2^52 when a histogram entry cannot reach 2^52 anyway (NOMASK):
                // a cell collects at most cell^2 * 255*sqrt(2) * 2^36 < 2^52 for cell <= 13, so the low 52 bits of the
                // wrapped u64 sums are the exact sums and one mask in the fold replaces four per pixel.
                auto fx = [&](float v) -> u64 {
                    double yv;
                    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(yv) : "v"((double)v), "s"(68719476736.0), "v"(two52));
                    if (NOMASK) return (u64)__builtin_bit_cast(long long, yv);
                    const unsigned hi = (unsigned)__double2hiint(yv) & 0xfffffu, lo = (unsigned)__double2loint(yv);
                    return ((u64)hi << 32) | lo;
                };
                // private copy ((slot*2O + bin)*PW + hcol)*R + (x % R): one 24-bit multiply-add on the bin + a per-lane
                // constant, a scalar band-slot offset each for by / by+1, the column neighbour in the immediate offset
                const unsigned base = __umul24((unsigned)bin, (unsigned)(PW * R * 8)) + (unsigned)lane_off * 8u;
                const unsigned slot_bytes = (unsigned)(2 * O * PW * R * 8);
                unsigned char* cb = (unsigned char*)w.copies;
                u64* p0 = (u64*)(cb + (base + (unsigned)(by & 1) * slot_bytes));
                u64* p1 = (u64*)(cb + (base + (unsigned)((by + 1) & 1) * slot_bytes));
                atomicAdd(p0 + R, fx(va));     // band by,   column bx+1
                atomicAdd(p0, fx(vb));         // band by,   column bx
                atomicAdd(p1 + R, fx(vc));     // band by+1, column bx+1
                atomicAdd(p1, fx(vd));         // band by+1, column bx
            } else {
                const int base = bin * PWW + (by + 1) * PW + hcol;
                // reference order per accumulator: (bx+1,by) (bx,by) (bx+1,by+1) (bx,by+1), lanes ascending
                if (va != 0.0f) atomicAdd(&histf[base + 1], va);
                if (vb != 0.0f) atomicAdd(&histf[base], vb);
                if (vc != 0.0f) atomicAdd(&histf[base + PW + 1], vc);
                if (vd != 0.0f) atomicAdd(&histf[base + PW], vd);
            }
            }
        }
        rm2 = rm1; rm1 = r0;
    };
    row_step(0, 0, false);
    row_step(1, 1, false);
    int yrow = 2;
    for (; yrow + 1 < S; yrow += 2) {
        row_step(0, yrow, true);
        row_step(1, yrow + 1, true);
    }
    if (yrow < S) row_step(0, yrow, true);
    if (ACC == ACC_FIXED64 && cur_by != -2) { flush_band(cur_by); flush_band(cur_by + 1); }
    if (ACC == ACC_COLUMNS) {
        *pend_p += pend_v;
        if (prev_by >= 0) fold_band(prev_by);
        if (prev_by + 1 <= C - 1) fold_band(prev_by + 1);      // (cell sizes < 3: the last rows never reach the last band)
    }
    mark(2);   // row loop
    wave_sync();
    mark(3);   // barrier after the row loop

    // ---- per patch (one after the other in PAIR mode: they share the normalisation scratch) ------------------------
    for (int hp = 0; hp < NP; ++hp) {
        if (hp == 1 && !second_valid) break;
        const u64* hfin_p = (const u64*)((unsigned char*)w.hfin + (size_t)hp * a_bytes);
        const float* histf_p = (const float*)((unsigned char*)w.hfin + (size_t)hp * a_bytes);
        float* out_desc = out_row + (long long)(landmark + hp) * lv.P;
        // (FT = float was measured: 2.4 % faster, max deviation from the exact-sum mode 1.2e-7 instead of 9e-8 -- not worth
        // leaving hog.c's double arithmetic)
        if (ACC == ACC_COLUMNS) hog_finish_lean<TO, TC, double>(chist + hp * chist_stride, lds_base, out_desc, lv, lane);
        else hog_finish_patch<ACC, TO, TC>(w, hfin_p, histf_p, out_desc, lv, lane);
        mark(4);   // normalisation / extraction / store
    }
    mark(5);   // output stores
}

template <int ACC, int FASTBIN, int TO, int TC, bool PAIR, bool PROF = false>
__global__ void __launch_bounds__(HF_WAVES * 64)
hog_fast_kernel(ImageSetDev imgs, const int* __restrict__ img_idx, const float* __restrict__ x, int N, int L,
                EyeIdxDev eyes, HogLevelDev lv, float* __restrict__ feat, long long ldf,
                int* __restrict__ idx_out, int* __restrict__ status, size_t lds_per_wave,
                unsigned long long* prof = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = uni(threadIdx.x >> 6);
    // XCD-aware remap (bijective): workgroups that the dispatcher places on XCD b%8 take a contiguous run of patches
    const unsigned nb = gridDim.x, b = blockIdx.x;
    const unsigned q = nb / 8, r = nb % 8, xcd = b % 8;
    const unsigned blk = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
    const long long p = (long long)blk * HF_WAVES + wave;
    const int Lw = PAIR ? (L + 1) / 2 : L;      // wave slots per sample: one per landmark, or one per landmark pair
    const bool valid = p < (long long)N * Lw;
    // (ACC_COLUMNS has one workgroup barrier, behind the shared fold weights: tail waves stay until then, on patch 0)
    if (!valid && ACC != ACC_COLUMNS) return;
    const long long pe = valid ? p : 0;
    const int s = (int)(pe / Lw), iw = (int)(pe - (long long)s * Lw);
    const int i = PAIR ? 2 * iw : iw;
    const bool second_valid = PAIR && (i + 1 < L);
    const int im = img_idx ? img_idx[s] : s;
    const float* xr = x + (long long)s * 2 * L;
    float* row = feat + (long long)s * ldf;
    hog_patch_fast<ACC, FASTBIN, TO, TC, PAIR, PROF>(imgs, im, xr, L, i, second_valid, eyes, lv, smem + (size_t)wave * lds_per_wave,
                                                     row, idx_out ? idx_out + (long long)s * (1 + 2 * L) : nullptr, status, prof,
                                                     (float*)(smem + (size_t)HF_WAVES * lds_per_wave), valid);
    if (!valid) return;
    if (PROF && (threadIdx.x & 63) == 0) atomicAdd(&prof[7], 1ull);
    // bias, adaptive_vlhog.hpp:182-183 (the non-adaptive example transform has none)
    if (lv.fixed_h == 0 && iw == Lw - 1 && (threadIdx.x & 63) == 0) row[(long long)L * lv.P] = 1.0f;
}

// count the (gx, gy) pairs for which the un-normalised arg-max disagrees with the reference arithmetic
__global__ void verify_fast_bins_kernel(HogLevelDev lv, int* __restrict__ mismatches)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 511 * 511) return;
    const float gx = (float)(i % 511 - 255), gy = (float)(i / 511 - 255);
    const float g = sqrtf(gx * gx + gy * gy);
    int a, b, c;
    bin_reference(gx, gy, g, lv, a);
    bin_unnormalised(gx, gy, lv, b);
    bin_sector<0>(gx, gy, lv, lv.O, c);
    const float g2 = gx * gx + gy * gy;
    const int want = __builtin_bit_cast(int, sqrtf(g2));
    const bool sqrt2_ok = __builtin_bit_cast(int, sqrt_int_exact(g2)) == want;
    const bool sqrt1_ok = __builtin_bit_cast(int, sqrt_int_up(g2)) == want;
    // mode 1: un-normalised arg-max + two-sided sqrt;  mode 2: sector count + one-sided sqrt, where a pixel the
    // reference skips (a == -1) may carry any valid bin as long as its magnitude is exactly 0
    bool sector_ok = (a == c) || (a == -1 && g == 0.0f && c >= 0 && c < 2 * lv.O);
    if (lv.O == 4) {
        bool b0, b1, b2;
        bin_sector4_bits(gx, gy, lv, b0, b1, b2);
        sector_ok = sector_ok && ((int)b0 + 2 * (int)b1 + 4 * (int)b2 == c);
    }
    if (a != b || !sqrt2_ok) atomicAdd(mismatches, 1);
    if (!sector_ok || !sqrt1_ok) atomicAdd(mismatches + 1, 1);
    // the packed kernel's raw v_sqrt_f32: acceptable only if it is the correctly rounded root or exactly one ulp below it
    const int raw = __builtin_bit_cast(int, __builtin_amdgcn_sqrtf(g2));
    if (!(raw == want || raw == want - 1)) atomicAdd(mismatches + 2, 1);
    // the packed kernel's octant code on rotated coordinates (4 orientations): its bin must be the reference's
    if (lv.O == 4) {
        const int row = bin_rot4_row(gx, gy);
        int jb = -1;
        for (int j = 0; j < 8; ++j) if ((int)HP_ROW_OF_BIN(j) == row) jb = j;
        if (!((a == jb) || (a == -1 && g == 0.0f))) atomicAdd(mismatches + 3, 1);
    }
}

}  // namespace

bool sdm_hog_fast_supported(const HogLevelDev& lv)
{
    return lv.S >= 4 && lv.S <= 64 && fast_lds_bytes(lv.cell, lv.C, lv.O, lv.D) * HF_WAVES <= 160 * 1024;
}

// two patches per wave: the ROI fits a half wave and the CU still holds at least as many patches in flight as with one
// patch per wave (LDS-limited workgroups per CU x patches per wave)
static bool hog_fast_pair(const HogLevelDev& lv, int fast_bins, bool columns = false)
{
    if (lv.S > 32 || fast_bins != 2) return false;
    const size_t one = fast_wg_lds_bytes(lv.cell, lv.C, lv.O, lv.D, false, columns);
    const size_t two = fast_wg_lds_bytes(lv.cell, lv.C, lv.O, lv.D, true, columns);
    if (two > 160 * 1024) return false;
    const size_t wg_one = (160 * 1024) / one, wg_two = (160 * 1024) / two;
    return 2 * wg_two >= wg_one;
}

void sdm_launch_verify_fast_bins(const HogLevelDev& lv, int* mismatches_dev, hipStream_t stream)
{
    const int n = 511 * 511;
    hipLaunchKernelGGL(verify_fast_bins_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, lv, mismatches_dev);
}

template <int TO, int TC>
static void launch_fast_oc(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                           const EyeIdxDev& eyes, const HogLevelDev& lv, float* feat, long long ldf, int* idx_out,
                           int* status, int acc_mode, int fast_bins, hipStream_t stream)
{
    // column sums need the compile-time geometry (MFMA tile count) and both patches' cell columns in 16 MFMA columns
    const bool columns = acc_mode == ACC_COLUMNS && TO > 0 && TC > 0 && 2 * TC <= 16;
    const bool exact_order = acc_mode == ACC_EXACT_ORDER;
    const bool pair = hog_fast_pair(lv, fast_bins, columns);
    const long long total = (long long)N * (pair ? (L + 1) / 2 : L);
    const size_t per = fast_lds_bytes(lv.cell, lv.C, lv.O, lv.D, pair, columns);
    const unsigned grid = (unsigned)((total + HF_WAVES - 1) / HF_WAVES);
    const dim3 g(grid), b(HF_WAVES * 64);
    const size_t lds = fast_wg_lds_bytes(lv.cell, lv.C, lv.O, lv.D, pair, columns);
    static unsigned long long attr_seen = 0;
    if (sdm_first_use_on_device(attr_seen)) {
#define HATTR(A, B, P) SDM_SET_ATTR((const void*)hog_fast_kernel<A, B, TO, TC, P>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)
        HATTR(ACC_EXACT_ORDER, 0, false); HATTR(ACC_EXACT_ORDER, 1, false); HATTR(ACC_EXACT_ORDER, 2, false);
        HATTR(ACC_FIXED64, 0, false); HATTR(ACC_FIXED64, 1, false); HATTR(ACC_FIXED64, 2, false);
        HATTR(ACC_EXACT_ORDER, 2, true); HATTR(ACC_FIXED64, 2, true);
        if constexpr (TO > 0) { HATTR(ACC_COLUMNS, 0, false); HATTR(ACC_COLUMNS, 1, false); HATTR(ACC_COLUMNS, 2, false); HATTR(ACC_COLUMNS, 2, true); }
#undef HATTR
    }
#define LAUNCH(ACC, FB, P)                                                                                               \
    hipLaunchKernelGGL((hog_fast_kernel<ACC, FB, TO, TC, P>), g, b, lds, stream, imgs, img_idx, x, N, L, eyes, lv, feat, \
                       ldf, idx_out, status, per)
#define LAUNCH_ACC(ACC)                                                                    \
    do {                                                                                   \
        if (pair) LAUNCH(ACC, 2, true);                                                    \
        else if (fast_bins == 2) LAUNCH(ACC, 2, false);                                    \
        else if (fast_bins == 1) LAUNCH(ACC, 1, false);                                    \
        else LAUNCH(ACC, 0, false);                                                        \
    } while (0)
    if (exact_order) LAUNCH_ACC(ACC_EXACT_ORDER);
    else if (columns) { if constexpr (TO > 0) LAUNCH_ACC(ACC_COLUMNS); }
    else LAUNCH_ACC(ACC_FIXED64);
#undef LAUNCH_ACC
#undef LAUNCH
}

// instrumented run (s_memtime per phase, summed over waves): prof[0..5] phase cycles, prof[7] waves
void sdm_launch_hog_fast_profile(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                                 const EyeIdxDev& eyes, const HogLevelDev& lv, float* feat, long long ldf,
                                 int* status, unsigned long long* prof_dev, hipStream_t stream)
{
    const long long total = (long long)N * L;
    if (total <= 0 || !(lv.O == 4 && lv.C == 5)) return;
    const size_t per = fast_lds_bytes(lv.cell, lv.C, lv.O, lv.D, false, true);
    const unsigned grid = (unsigned)((total + HF_WAVES - 1) / HF_WAVES);
    static unsigned long long attr_seen = 0;
    if (sdm_first_use_on_device(attr_seen))
        SDM_SET_ATTR((const void*)hog_fast_kernel<ACC_COLUMNS, 2, 4, 5, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL((hog_fast_kernel<ACC_COLUMNS, 2, 4, 5, false, true>), dim3(grid), dim3(HF_WAVES * 64), per * HF_WAVES + HF_WT_BYTES,
                       stream, imgs, img_idx, x, N, L, eyes, lv, feat, ldf, (int*)nullptr, status, per, prof_dev);
}

void sdm_launch_hog_fast(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                         const EyeIdxDev& eyes, const HogLevelDev& lv, float* feat, long long ldf, int* idx_out,
                         int* status, int acc_mode, int fast_bins, hipStream_t stream)
{
    if ((long long)N * L <= 0) return;
    // specialised instances for the shipped (4 orientations) and the "31-bin" (9 orientations) 5x5-cell geometry
    const bool small_cell = lv.cell <= 13;   // the specialised instances rely on cell^2 * 361 < 2^16 (see fx)
    if (lv.O == 4 && lv.C == 5 && small_cell)
        launch_fast_oc<4, 5>(imgs, img_idx, x, N, L, eyes, lv, feat, ldf, idx_out, status, acc_mode, fast_bins, stream);
    else if (lv.O == 9 && lv.C == 5 && small_cell)
        launch_fast_oc<9, 5>(imgs, img_idx, x, N, L, eyes, lv, feat, ldf, idx_out, status, acc_mode, fast_bins, stream);
    else
        launch_fast_oc<0, 0>(imgs, img_idx, x, N, L, eyes, lv, feat, ldf, idx_out, status, acc_mode, fast_bins, stream);
}
