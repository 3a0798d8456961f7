// sdm_hog_packed.hip -- the lane-packed HOG kernel for gfx950 (hog_packed_kernel: the default pixel kernel of the detect and
// training paths), its normalisation (hog_finish_direct), the per-level tables of resize taps (taps_table_kernel, pair_taps_table_kernel) and their
// launchers sdm_launch_hog_packed / sdm_launch_hog_cells / sdm_launch_taps_table / sdm_launch_pair_taps_table.  The launch plan it walks is built on the
// host by sdm_hog_plan.hip; the device helpers it shares with the one-patch-per-wave family (sdm_hog_fast.hip) are
// sdm_hog_device.h.
//
// Lane-packed kernel (ACC_COLUMNS arithmetic, 4 orientations, 5 x 5 cells): one wave walks a GROUP of patches of one sample
// in passes of 64 pixel columns (HogPlanDev, sdm_kernels.h).  Per group: inter-eye distance, patch half-width, resize
// scale and the per-coordinate tap tables ONCE (they are the same for every landmark of a sample, adaptive_vlhog.hpp:123);
// per pass: every lane fetches the taps of ITS column from the lane that computed that coordinate (ds_bpermute), applies
// its own patch's image borders, and the row loop of hog_patch_fast's two-patch form runs unchanged -- each lane adds
// g * wy to its own pixel column [bin][lane][band slot]; the band folds multiply the 64 columns by the pass's weight
// table (16 registers per lane, loaded per pass) on the matrix cores and ADD the cells to the histograms of the up to
// three patches the pass touches (a patch cut by a pass boundary gets its cells from two passes).  A patch is normalised
// and stored as soon as its last column has been folded; its histogram slot is then free for the patch three further on.
// Same integer decisions and the same f32 operations per accumulator as hog_patch_fast<ACC_COLUMNS>, except that the cells
// of a cut patch are the sum of two partial folds.
#include "sdm_kernels.h"
#include "sdm_hog_device.h"
#include <type_traits>

#pragma clang fp contract(off)

// geometry of the launch
#define HP_WAVES 4                  /* waves per workgroup */
#define HP_ST 66                    /* column-row stride: 64 pixel columns + 2 (2 * 66 = 4 mod 32 dwords: the sixteen bin rows of a fold read fall into 8 banks) */
#define HP_MINW 6                   /* __launch_bounds__ minimum waves per SIMD: <= 80 registers, with 6.6 KB of LDS per wave six waves fit */
#define HP_MINW_CELLS 6             /* the CELLS form needs 5.1 KB of LDS per wave: seven waves per SIMD fit if the registers do (<= 72) */
// Row carry (the CELLS instances specialised on the cell size): where the patch is enlarged, the lower source row of resized row y
// is one of the two rows that row y - 1 already loaded and filtered, so a second row loop loads and filters the UPPER source row
// only and selects the lower one from the two values it holds (a bit-field select, v_bitop3_b32 on gfx950, with a mask from the row table).  Which half-widths
// qualify is decided per (level, h) by taps_table_kernel from the taps themselves; a wave picks its loop once, above the loop.
// Per cell size: whether the instance carries the second loop (it adds 60 - 70 % to the instance's code), by measurement
// (profiles/hog_row_carry.txt): cells 10 / 8 / 6 run 12 / 13 / 8 % faster with it at the shipped levels.  Cell 11 with it: 331.1 us
// per launch against 331.1 without (at relative patch size 1.0, S = 55, 1 % of the faces have an enlarged patch) -- left out.
__host__ __device__ constexpr bool hp_row_carry(int cell) { return cell == 10 || cell == 8 || cell == 6; }
// Pair carry (the CELLS instance of cell 11, where the patch is REDUCED by less than 1.5: S < 2h < 1.5 S): every pixel row d >= 1 is
// a SHIFT row (its lower source row is row d - 1's upper one) or an ORPHAN row (its lower source row is the one after row d - 1's
// upper one: both of its rows are new), and no pair of pixel rows (2p + 1, 2p + 2) holds two orphans.  A third row loop then loads
// THREE source rows per pair of pixel rows instead of four: the upper row of both, and one spare that serves whichever row of the pair
// is the orphan (its address is put out of the buffer's range where the pair has none: nothing is fetched).  The lower row of every
// pixel row is one bit select between the previous upper row and the spare.  Eligibility, the per-row "take the spare" masks and the
// per-pair spare rows come from pair_taps_table_kernel.  Per cell size, by measurement (profiles/hog_pair_carry.txt).
#ifndef HP_PAIR_CARRY_11
#define HP_PAIR_CARRY_11 1
#endif
__host__ __device__ constexpr bool hp_pair_carry(int cell) { return HP_PAIR_CARRY_11 && cell == 11; }
// spare offsets of the pair loop: one int per pair of pixel rows (2p + 1, 2p + 2), per wave, behind the row table
__host__ __device__ constexpr int hp_pair_slots(int cell, int C, bool cells, bool raw) { return cells && raw && hp_pair_carry(cell) ? (C * cell - 1) / 2 : 0; }
// (The ablation switches of rounds 3-6 -- HP_ABL = 1 ... 15: no folds, no read-modify-write, no image loads, conflict-free operand
//  reads, ... -- are scripts/experiments/hog_packed_ablations.patch; scripts/r6_hog_lds_variants.sh applies it to a copy and builds
//  the variants.  Their measurements: profiles/r04_hog_ablations.txt, profiles/r06_hog_lds.txt.)
// (What a band fold costs by part -- no folds, no operand split, no stores, no matrix instructions, no clears -- is
//  scripts/experiments/hog_fold_ablations.patch, measured in profiles/hog_fold_cost.txt.)
// (The settled build switches of rounds 2-6 -- of this file, sdm_hog_fast.hip and sdm_hog_plan.hip; among them the float / double
//  normalisation and the three- / four-product float16 fold that scripts/feature_error.py compared -- are
//  scripts/experiments/hog_settled_switches.patch, which re-adds them to this tree.)

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// (the same with the weight in a vector register: the packed kernel reads it from its per-row table in LDS)
__device__ inline unsigned mul_hi_u24_vv(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

#define HP_ROWS_BYTES(O) ((size_t)2 * (O) * HP_ST * 8)
#define HP_HIST_BYTES(O, CC) ((size_t)2 * (O) * (CC) * 4)
// finish scratch: cell norms, block factors and the clamped undirected values [4][O][CC] of the descriptor pass, staged for the
// texture sums (measured and dropped: recomputing them there, O products per output, instead of staging)
__host__ __device__ inline size_t packed_scratch_bytes(int C, int O = 4)
{
    return al16((size_t)C * C * 4) + al16((size_t)(C + 1) * (C + 1) * 8) + al16((size_t)4 * O * C * C * 8);
}
// per wave: [ column rows | per-row table of the vertical taps, S + 2 entries of 16 bytes | spare offsets of the pair loop | hist_slots histograms ]
// (the finish scratch overlays the column rows, which are all zero between two passes)
// (the generic instance issues its image loads two rows ahead without looking: entries S and S + 1 repeat the last row; the
//  instances specialised on the cell size know at compile time where the ROI ends and keep S entries)
__host__ __device__ inline size_t packed_rowtab_bytes(int S, bool spec = false) { return (size_t)(S + (spec ? 0 : 2)) * 16; }
__host__ __device__ inline size_t packed_lds_bytes(int C, int O, int S, int hist_slots, bool spec = false, int pair_slots = 0)
{
    return al16(HP_ROWS_BYTES(O)) + packed_rowtab_bytes(S, spec) + al16((size_t)pair_slots * 4) + hist_slots * al16(HP_HIST_BYTES(O, C * C));
}
// specialised instances of the feature-row form: the band-slot weights {ws0, ws1} of every pixel row (level constants,
// hog.c:697-704) in ONE table per workgroup behind the waves' regions, read per row with a broadcast 8-byte LDS read straight
// into the register pair the packed multiply-add takes (scalar loads of them cannot stay in SGPRs over an unrolled ROI: the
// compiler spilled them to vector lanes and paid two v_readlane per row)
// (rows 0 and S - 1 have no gradient: the table holds rows 1 .. S - 2)
// The detect instances (raw cells, 4 orientations) have no such table: the pairs are compile-time constants (packed_row_const,
// sdm_kernels.h) that the row loop takes from scalar registers -- HpBandPairs below.
__host__ __device__ constexpr bool hp_const_weights(int O, int cell, bool cells, bool raw) { return cells && raw && O == 4 && cell > 0; }
__host__ __device__ inline size_t packed_wstab_bytes(int S) { return al16((size_t)(S - 2) * 8); }
__host__ __device__ inline size_t packed_wg_lds_bytes(int C, int O, int S, int hist_slots, bool spec, int pair_slots = 0, bool wstab = true)
{
    return packed_lds_bytes(C, O, S, hist_slots, spec, pair_slots) * HP_WAVES + (spec && wstab ? packed_wstab_bytes(S) : 0);
}

// The band-slot weights of a detect instance, sorted out at compile time.  Rows 1 .. S - 2 multiply by the pair {ws0, ws1} of
// packed_row_const (x 8 where the folds are float16: the column sums carry that factor, exactly).
//  * A row with two non-zero weights takes its pair from a PAIR of scalar registers, the operand of the packed multiply-add.  Two
//    rows whose pairs hold the same two bit patterns -- in either slot order: a row of an even band and the matching row of an odd
//    one -- share the registers; `swap` says that the row wants them the other way round, which the instruction's operand
//    selectors do.
//  * A row with ONE non-zero weight -- the half cells at either end, whose other cell row (-1 or C) does not exist, and the centre
//    row of an odd cell -- changes one column sum only: fma(0, g, q) is q for a finite g and a column sum q, which is never -0.  It
//    takes a plain multiply-add on that slot, with ONE scalar register: an element of a pair where the bits are the same, else a
//    register of its own.
// What this is for: the hardware admits a workgroup of four waves by its scalar registers too, in steps of sixteen -- eight per CU up
// to 80, seven up to 96 -- and the compiler's occupancy figure does not know (profiles/hog_row_weights.txt).  Only cell 8 divides
// exactly; at the other cell sizes the fraction of hx is rounded at the magnitude of hx, so the same position in another band is
// often another bit pattern: 14 / 12 / 4 / 9 pairs and 4 / 1 / 0 / 1 single registers at cells 11 / 10 / 8 / 6 (every row a pair: 23 / 19 / 7 /
// 12 pairs, which cost cells 11 and 10 a workgroup per CU and with it the whole gain).
template <int CELL, int C, bool X8>
struct HpBandPairs {
    static constexpr int S = C * CELL;
    int n = 0, n1 = 0;
    float a[S] = {}, b[S] = {};      // pair k as the registers hold it
    float one[S] = {};               // single register k
    int idx[S] = {};                 // row d -> its pair; a row of one weight: the pair it borrows from, or -1 - (its single register)
    bool swap[S] = {};               // row d takes {b, a}; a row of one weight that borrows: element b
    int slot[S] = {};                // row d has one weight, for this slot; -1: two
    constexpr HpBandPairs()
    {
        float w[S][2] = {};
        for (int d = 1; d < S - 1; ++d) {
            const HogRowConst rc = packed_row_const(d, CELL, C);
            w[d][0] = rc.ws0 * (X8 ? 8.0f : 1.0f); w[d][1] = rc.ws1 * (X8 ? 8.0f : 1.0f);
            slot[d] = w[d][1] == 0.0f ? 0 : (w[d][0] == 0.0f ? 1 : -1);
        }
        for (int d = 1; d < S - 1; ++d) {      // (weights are never NaN and never -0: == compares the bits)
            if (slot[d] >= 0) continue;
            int k = 0;
            bool sw = false;
            for (; k < n; ++k) {
                if (a[k] == w[d][0] && b[k] == w[d][1]) break;
                if (a[k] == w[d][1] && b[k] == w[d][0]) { sw = true; break; }
            }
            if (k == n) { a[n] = w[d][0]; b[n] = w[d][1]; ++n; }
            idx[d] = k; swap[d] = sw;
        }
        for (int d = 1; d < S - 1; ++d) {
            if (slot[d] < 0) continue;
            const float v = w[d][slot[d]];
            int k = 0;
            for (; k < n; ++k)
                if (a[k] == v || b[k] == v) break;
            if (k < n) { idx[d] = k; swap[d] = a[k] != v; continue; }
            for (k = 0; k < n1; ++k)
                if (one[k] == v) break;
            if (k == n1) one[n1++] = v;
            idx[d] = -1 - k;
        }
    }
};

// arithmetic type of the packed kernel's normalisation (hog.c:930-1052 computes the block factors and the clamped products in
// double and stores floats).  In float -- v_rsq_f32 for 1 / sqrt, f32 products -- the features differ from the oracle exactly as
// much as before (max 1.8e-7, relative L2 7.5e-8 -> 8.0e-8 over 128 faces x 4 levels, scripts/feature_error.py: the separable
// column sums dominate), and the kernel is 3.7 % faster.  The one-patch-per-wave kernels and the exact modes keep the double path.
__device__ inline float ft_rsqrt(float v) { return __builtin_amdgcn_rsqf(v); }
__device__ inline float ft_min02(float v) { return __builtin_fminf(0.2f, v); }
// hog_finish_lean with the descriptor written straight to the feature row (no staging copy: 2 KB less LDS per wave)
template <int TO, int TC>
__device__ void hog_finish_direct(const float* hist, unsigned char* scratch, float* __restrict__ out_desc,
                                  const HogLevelDev& lv, int lane)
{
    typedef float FT;
    constexpr int O = TO, C = TC, CC = C * C, CB = C + 1;
    float* nrm = (float*)scratch;
    FT* fac = (FT*)(scratch + al16((size_t)CC * 4));
    FT* hcc = (FT*)(scratch + al16((size_t)CC * 4) + al16((size_t)CB * CB * 8));      // [4][O][CC] clamped hc_j
    static_assert(((TC * TC * 4 + 15) / 16 * 16) + (((TC + 1) * (TC + 1) * 8 + 15) / 16 * 16) + 4 * TO * TC * TC * 8 <= 2 * TO * HP_ST * 8,
                  "the finish scratch overlays the column rows");
    for (int c = lane; c < CC; c += 64) {                       // cell norms (hog.c:875-890)
        float n = 0.0f;
        for (int k = 0; k < O; ++k) {
            const float hs = hist[c + k * CC] + hist[c + (k + O) * CC];
            n += hs * hs;
        }
        nrm[c] = n;
    }
    wave_sync();
    for (int t = lane; t < CB * CB; t += 64) {                  // block factors (hog.c:930-981): see hog_finish_patch
        const int byb = t / CB, bxb = t - byb * CB;
        const int xa = bxb - 1 > 0 ? bxb - 1 : 0, xb = bxb < C - 1 ? bxb : C - 1;
        const int ya = byb - 1 > 0 ? byb - 1 : 0, yb = byb < C - 1 ? byb : C - 1;
        const FT na = nrm[xa + ya * C], nb = nrm[xb + ya * C];
        const FT nc = nrm[xa + yb * C], nd = nrm[xb + yb * C];
        fac[t] = ft_rsqrt(na + nb + nc + nd + (FT)1e-4);
    }
    wave_sync();
#define CL02(v) ft_min02(v)
    for (int t = lane; t < O * CC; t += 64) {                   // hog.c:985-1033, Matlab order of adaptive_vlhog.hpp:166-175
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
            out_desc[ct + k * CC] = (float)((FT)0.5 * (ha1 + ha2 + ha3 + ha4));
            out_desc[ct + (k + O) * CC] = (float)((FT)0.5 * (hb1 + hb2 + hb3 + hb4));
            out_desc[ct + (k + 2 * O) * CC] = (float)((FT)0.5 * (hc1 + hc2 + hc3 + hc4));
            // t = k * CC + c: consecutive lanes, consecutive values
            hcc[t] = hc1; hcc[O * CC + t] = hc2; hcc[2 * O * CC + t] = hc3; hcc[3 * O * CC + t] = hc4;
        } else {
            out_desc[ct + k * CC] = (float)hc1;
            out_desc[ct + (k + O) * CC] = (float)hc2;
            out_desc[ct + (k + 2 * O) * CC] = (float)hc3;
            out_desc[ct + (k + 3 * O) * CC] = (float)hc4;
        }
    }
    if (lv.variant == 1) {                                      // texture sums (hog.c:1020-1023, 1047-1052): t_j = sum over k, in order, of the clamped hc_j
        const float tex = 1.0f / sqrtf(18.0f);
        wave_sync();
        for (int t = lane; t < 4 * CC; t += 64) {
            const int j = t / CC, c = t - j * CC;
            const int y = c / C, x = c - y * C, ct = x * C + y;
            FT acc = 0;
#pragma unroll
            for (int k = 0; k < O; ++k) acc += hcc[(j * O + k) * CC + c];
            out_desc[ct + (3 * O + j) * CC] = (float)(tex * acc);
        }
    }
#undef CL02
    wave_sync();
}

// Gradient magnitude of the RAW instances: v_sqrt_f32 as the hardware returns it.  On gfx950 it is the correctly rounded root or
// one ulp below it (15 % of the 511^2 possible gradients, never above, never further: scripts/ubench/sqrt_candidates.hip); the
// four-instruction residual test that repairs the ulp (sqrt_int_up, kept by the one-patch-per-wave kernels and the exact
// modes) costs 4 % of this kernel, and no two-instruction form is exact on all inputs.  The features move by < 3e-8, inside the
// tolerance the separable column sums of this mode have anyway (<= 2e-7 from the oracle); no integer decision depends on it.
//
// CELL > 0: the instance is specialised on the level's cell size: S, the band of every pixel row and
// hence the fold sites, the band slots and every row-table offset are compile-time constants, the row loop is unrolled over
// the S rows -- no per-row scalar loads of the band index, no band compare / branch, no loop counter.  CELL == 0: any cell size
// (the round-2 form of the loop).  RAW: the gradient magnitude is v_sqrt_f32 as the hardware returns it (chosen per level at
// sdm_set_model_geometry, only if the exhaustive check found it exact or one ulp low on all 511^2 gradients).
// CELLS: the launch stops at the raw cell histograms (round 4): every band fold stores its cells straight to HBM,
// cells[sample][landmark][part][cell column][cell row][2O] (a lane stores its four bins of one cell with one 16-byte store; part 0: the pass that sees the patch's first column, part 1: the second pass of a
// patch cut by a pass boundary -- the consumer adds the two), there are no histogram slots in LDS and no normalisation phase in
// this kernel: sdm_desc.hip normalises (hog.c:857-1062) with a lane per cell and either writes the feature rows or multiplies
// the descriptors by the regressor while they are still on the chip.  `feat` is then the cells buffer, `ldf` unused.
template <int TO, int TC, int CELL, bool RAW, bool CELLS = false>
__global__ void __launch_bounds__(HP_WAVES * 64, CELLS ? HP_MINW_CELLS : HP_MINW)
hog_packed_kernel(ImageSetDev imgs, const int* __restrict__ img_idx, const float* __restrict__ x, int N, int L,
                  EyeIdxDev eyes, HogLevelDev lv, HogPlanDev plan, float* __restrict__ feat, long long ldf,
                  int* __restrict__ idx_out, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int O = TO, C = TC, CC = C * C;
    constexpr int ST = HP_ST;
    static_assert(2 * TO <= 32 && SDM_PLAN_MAX_SEG * TC <= 16, "16 x 16 matrix-core tiles: 2O bin rows in one or two tiles, 3 patches x C cell columns");
    constexpr int MT = (2 * TO + 15) / 16;        // row tiles of a band fold: 1 for 4 orientations, 2 for the 18 bin rows of "31-bin" HOG (hog.c:212-215)
    const int lane = threadIdx.x & 63;
    const int wave = uni(threadIdx.x >> 6);
    // XCD-aware remap (bijective): the workgroups the dispatcher places on XCD b % 8 take a contiguous run of groups, so the
    // groups of one sample meet in one L2
    const unsigned nb = gridDim.x, bid = blockIdx.x;
    const unsigned q8 = nb / 8, r8 = nb % 8, xcd = bid % 8;
    const unsigned blk = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
    // work unit of a wave: a group of patches (all its passes), or -- CELLS: the passes share nothing but the group geometry, every
    // fold stores its cells to HBM -- ONE pass: uniform, short waves whose number is a finer multiple of the
    // 6 144 wave slots of the chip (RCR-22 level 1 at 4 096 faces: 20 480 waves of four or two passes = 3.3 rounds of slots
    // became 73 728 waves of one pass = 12.0 rounds)
    // (Round 5, VERDICT r04 item 4a: a wave taking k consecutive passes of its sample -- inter-eye distance, half-width, taps, row
    //  table and the cleared column rows set up once per k passes -- measured 1.141 / 1.158 / 1.165 / 1.169 ms per 4 096 faces for
    //  k = 1 / 2 / 3 / 4, scripts/r5_detect_env_ab.py, profiles/r05_experiments.txt: the finer balance of one pass per wave is worth more
    //  than the set-up it repeats.  One pass per wave stays.)
    constexpr bool SPLIT = CELLS;
    const int gpf = SPLIT ? plan.n_main * plan.P + plan.Pt : plan.n_main + (plan.Gt > 0 ? 1 : 0);      // units per sample
    const long long wid = (long long)blk * HP_WAVES + wave;
    if (wid >= (long long)N * gpf) return;                           // (no workgroup barrier anywhere below)
    const int s = (int)(wid / gpf), u = (int)(wid - (long long)s * gpf);
    const int g = SPLIT ? (u < plan.n_main * plan.P ? u / plan.P : plan.n_main) : u;
    const bool main_group = g < plan.n_main;
    const int lm0 = main_group ? g * plan.G : plan.n_main * plan.G;   // first landmark of the group
    const int t_first = SPLIT ? u - g * plan.P : 0;                   // (tail group: u - n_main P)
    const int npass = SPLIT ? t_first + 1 : (main_group ? plan.P : plan.Pt);
    const int pass0 = main_group ? 0 : plan.P;
    constexpr int SC = TC * CELL;                 // (0 for the generic instance)
    const int S = CELL > 0 ? SC : lv.S;

    const int nslots = CELLS ? 0 : plan.hist_slots;                                   // 2, or 3 for ROIs under 22 columns; none when the cells go to HBM
    constexpr bool SPEC = CELL > 0;
    constexpr bool ROTB = RAW && TO == 4;          // octant code on rotated coordinates (bin_rot4_row); the folds read rows HP_ROW_OF_BIN(bin)
    constexpr int NPAIR = hp_pair_slots(CELL, TC, CELLS, RAW);      // > 0: the instance has the pair loop
    constexpr bool PAIR = NPAIR > 0;
    static_assert(!PAIR || (TC * CELL) % 2 == 1, "pair loop: rows 1 .. S - 1 in pairs");
    unsigned char* lds = smem + (size_t)wave * packed_lds_bytes(C, O, S, nslots, SPEC, NPAIR);
    float* colrows = (float*)lds;                                                    // [2O][ST][2 band slots]
    i32x4* rowtab = (i32x4*)(lds + al16(HP_ROWS_BYTES(O)));                          // [S (+ 2)] {row offset 0, row offset 1, weight 0 << 12, weight 1 << 12}
    int* sptab = (int*)(lds + al16(HP_ROWS_BYTES(O)) + packed_rowtab_bytes(S, SPEC));      // [NPAIR] byte offset of the pair's spare source row (PAIR)
    float* hist = (float*)(lds + al16(HP_ROWS_BYTES(O)) + packed_rowtab_bytes(S, SPEC) + al16((size_t)NPAIR * 4));   // [nslots][2O][CC]
    constexpr bool WCONST = hp_const_weights(TO, CELL, CELLS, RAW);      // the band-slot weights are constants in scalar registers: no table
    f32x2* wstab = (f32x2*)(smem + (size_t)HP_WAVES * packed_lds_bytes(C, O, S, nslots, SPEC, NPAIR));      // [S - 2] per workgroup (SPEC && !WCONST): rows 1 .. S - 2
    constexpr int HSTR = (2 * O * CC * 4 + 15) / 16 * 4;      // floats per histogram slot (16-byte multiple)
    unsigned char* scratch = lds;      // the finish scratch overlays the column rows, which are all zero between two passes
    auto hist_slot = [&](int patch_slot) { return nslots == 2 ? (patch_slot & 1) : patch_slot % 3; };

    const int im = uni(img_idx ? img_idx[s] : s);
    const float* xr = x + (long long)s * 2 * L;
    float* out_row = feat + (long long)s * ldf;
    int* idx_row = idx_out ? idx_out + (long long)s * (1 + 2 * L) : nullptr;

    // ---- CELLS: what depends on (level, pass, lane) only is requested first and arrives under the geometry's arithmetic ------------
    constexpr bool F16F = TO == 4 && CELL > 0;      // band folds on the 16-bit matrix cores (below)
    unsigned desc1 = 0;
    f32x4 wq1[4];
    i32x4 pinfo1 = {0, 0, 0, 0};
    f32x2 wsrow = {0.0f, 0.0f};
    if constexpr (CELLS) {
        const int pt1 = pass0 + t_first;      // the wave's one pass
        desc1 = plan.lane_tab[pt1 * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            wq1[i] = F16F ? ((const f32x4*)(plan.wb16 + ((size_t)pt1 * 64 + lane) * 32))[i] : ((const f32x4*)(plan.wb + ((size_t)pt1 * 64 + lane) * 16))[i];
        pinfo1 = *(const i32x4*)(plan.pass_info + pt1 * 4);      // wave-uniform, 16 bytes
        if (CELL > 0 && !WCONST) wsrow = (f32x2){lv.row_tab[lane][0], lv.row_tab[lane][1]};
    }

    // ---- group geometry (wave-uniform; adaptive_vlhog.hpp:123) ----------------------------------------------------------
    const int h = lv.fixed_h > 0 ? lv.fixed_h : uni((int)round((double)lv.rel * ied_of(xr, L, eyes) / 2));
    const bool empty = h <= 0;
    if (empty && lane == 0) atomicOr(status, SDM_DEV_ERR_EMPTY_PATCH);
    const int sw = empty ? 1 : 2 * h;
    const bool area2 = (sw == 2 * S);
    const uint8_t* img = imgs.base + imgs.offset[im];
    const int iw = imgs.w[im], ih = imgs.h[im], istride = imgs.stride[im];
    const __amdgpu_buffer_rsrc_t img_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)img, 0, ih * istride, 0x00020000);

    // ---- per-coordinate taps of cv::resize: lane d computes coordinate d once (shared by rows and columns, by all patches) ----
    int tab_s, tab_w;                 // unclamped source index floor((d + 0.5) scale - 0.5), 11-bit weights c0 | c1 << 16
    constexpr bool CARRY = CELLS && RAW && CELL > 0 && hp_row_carry(CELL);      // the instance has the one-load row loop
    int carry_mask = 0;               // row d takes its lower source row from row d - 1's upper one (all ones) or lower one (zero)
                                      // (PAIR: from the pair's spare (all ones) or row d - 1's upper one (zero))
    bool carry = false;               // this wave's half-width is one-load (PAIR: pair) eligible (wave-uniform)
    int spare_off = 0;                // PAIR: lane p holds the byte offset of the spare row of pixel rows (2p + 1, 2p + 2)
    i32x4 row_ent;                    // vertical taps of row d as the row loop wants them: byte offsets of the two source rows
                                      // RELATIVE to the patch origin (rows clipped to the patch), the two weights << 12
    if (CELLS && plan.taps && h < SDM_SCALE_TAB) {      // the level's table of taps by half-width (taps_table_kernel): two 16-byte loads
        const i32x4* e = (const i32x4*)(plan.taps + ((size_t)(h > 0 ? h : 0) * 64 + lane) * 8);
        const i32x4 e0 = e[0], e1 = e[1];
        tab_s = e0.x; tab_w = e0.y;
        row_ent = (i32x4){e0.z * istride, e0.w * istride, e1.x, e1.y};
        if (CARRY) { carry_mask = e1.z; carry = uni(e1.w) != 0 && !plan.two_load; }
        if (PAIR && plan.pair_taps) {
            const i32x4 e2 = *(const i32x4*)(plan.pair_taps + ((size_t)(h > 0 ? h : 0) * 64 + lane) * 4);
            carry_mask = e2.x; carry = uni(e2.z) != 0 && !plan.two_load;
            // a pair without an orphan: the address is 2^31 bytes off, outside the buffer's range -- the load returns 0 without a fetch
            // (and whatever it returned, the masks of both rows are zero)
            spare_off = e2.y >= 0 ? e2.y * istride : (int)0x80000000;
        }
    } else {
        const double scale = resize_scale(lv, h, sw);
        const ResizeTaps tp = resize_taps(lane < S ? lane : S - 1, scale, sw, area2);
        tab_s = tp.s0;
        tab_w = (tp.c0 & 0xffff) | (tp.c1 << 16);
        row_ent = (i32x4){tp.sy0 * istride, tp.sy1 * istride, tp.b0 << 12, tp.b1 << 12};
    }
    // (Measured and dropped: the vertical taps as one scalar 16-byte load per row from a per-level table [h][row] in HBM
    // instead of two v_readlane + eight scalar decode instructions -- 1.50 -> 1.58 ms: the scalar cache misses of 24 waves
    // per CU, each streaming the 1 KB of its own half-width, delay every other scalar load of the CU.)

    // ---- clear the column rows and the histogram slots --------------------------------------------------------------------
    {
        const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        constexpr int NZ = (int)((HP_ROWS_BYTES(O) + 15) / 16);      // 16-byte stores at constant offsets, the last trip on its first lanes
#pragma unroll
        for (int k = 0; k < (NZ + 63) / 64; ++k)
            if (64 * k + 63 < NZ || lane < NZ - 64 * k) ((f32x4*)lds)[64 * k + lane] = z4;      // (the histograms are stored before they are added to)
    }
    wave_sync();
    // the per-row table: every lane reads entry y with ONE broadcast LDS read per row (no v_readlane, no scalar decoding);
    // entries S and S + 1 (the row loop issues its loads two rows ahead) repeat the last row
    if (SPEC) {
        // specialised layout: entry e = {offsets of row e + 2, weights of row e}: the row loop wants exactly that pair at row e, in
        // ONE 16-byte broadcast read; the offsets of rows 0 and 1 (issued before the loop) sit in the last two entries
        // (one-load loop: entry e = {offset of the UPPER source row of row e + 2, carry mask of row e, weights of row e})
        if (lane < S) {
            const int eo = lane >= 2 ? lane - 2 : lane + S - 2;
            if ((CARRY || PAIR) && carry) { ((int*)&rowtab[eo])[0] = row_ent.y; ((int*)&rowtab[lane])[1] = carry_mask; }
            else *(i32x2*)&rowtab[eo] = (i32x2){row_ent.x, row_ent.y};
            *((i32x2*)&rowtab[lane] + 1) = (i32x2){row_ent.z, row_ent.w};
        }
        if (PAIR && carry && lane < NPAIR) sptab[lane] = spare_off;
    } else if (lane < S + 2) rowtab[lane] = row_ent;
    // (every wave of the workgroup writes the same values; a wave's own LDS accesses execute in order, so it reads what it -- or
    //  a neighbour, identically -- wrote: no workgroup barrier)
    // 4 orientations, specialised instances: band folds on the 16-bit matrix cores (column sums x 8 and weights x 2^10 as two float16
    // pieces each, all four piece products)
    static_assert(!F16F || CELL * 361 * 8 < 65504, "float16 folds: a band slot's column sum (<= cell x 255 sqrt 2) x 8 must stay a float16 number");      // (column sums carry a factor 8: exact, undone with the weights' 2^10 after the fold)
    if (SPEC && !WCONST && lane >= 1 && lane < S - 1) wstab[lane - 1] = (CELLS ? wsrow : (f32x2){lv.row_tab[lane][0], lv.row_tab[lane][1]}) * (F16F ? 8.0f : 1.0f);
    if (!SPEC && S + 2 > 64 && lane < S + 2 - 64) {
        i32x4 last;
#pragma unroll
        for (int k = 0; k < 4; ++k) last[k] = __builtin_amdgcn_readlane(row_ent[k], 63);
        rowtab[64 + lane] = last;
    }
    wave_sync();

    unsigned spread_sel = HF_SPREAD_SEL;
    asm volatile("" : "+v"(spread_sel));
    // -1 in a scalar register, opaque to the optimiser: fma(half, -1, v) written with the literal is rewritten to a conversion and a
    // subtraction; with the register it stays the one v_fma_mix_f32 of the fold's operand split
    float neg_one = -1.0f;
    if constexpr (CELLS) asm volatile("" : "+s"(neg_one));
    // the band-slot weight pairs of the instance, each pinned in a pair of scalar registers for the whole pass (opaque to the
    // optimiser, as neg_one: a constant the compiler can see through it is free to re-materialise where it is used, two scalar moves
    // of a literal per pixel row), and the single registers of the rows with one weight
    constexpr HpBandPairs<WCONST ? CELL : 1, TC, F16F> BP{};
    f32x2 wpair[BP.n > 0 ? BP.n : 1];
    float wone[BP.n1 > 0 ? BP.n1 : 1];
    if constexpr (WCONST) {
#pragma unroll
        for (int k = 0; k < BP.n; ++k) {
            wpair[k] = (f32x2){BP.a[k], BP.b[k]};
            asm volatile("" : "+s"(wpair[k]));
        }
#pragma unroll
        for (int k = 0; k < BP.n1; ++k) {
            wone[k] = BP.one[k];
            asm volatile("" : "+s"(wone[k]));
        }
    }
    // the column sums of a lane with the magnitude g of pixel row yy added: {q.x + ws0 g, q.y + ws1 g} (yy = 0: no row is pending, q)
    auto add_row = [&](const int yy, const float g, const f32x2 q) __attribute__((always_inline)) -> f32x2 {
        if (yy <= 0) return q;
        if (BP.slot[yy] < 0) {
            const f32x2 p = wpair[BP.idx[yy]];
            return __builtin_elementwise_fma(BP.swap[yy] ? (f32x2){p.y, p.x} : p, (f32x2){g, g}, q);
        }
        const float w = BP.idx[yy] < 0 ? wone[-1 - BP.idx[yy]] : (BP.swap[yy] ? wpair[BP.idx[yy]].y : wpair[BP.idx[yy]].x);
        return BP.slot[yy] == 0 ? (f32x2){__builtin_fmaf(w, g, q.x), q.y} : (f32x2){q.x, __builtin_fmaf(w, g, q.y)};
    };
    const int li = lane & 15, lq = lane >> 4;

    for (int t = t_first; t < npass; ++t) {
        const int pt = pass0 + t;
        // ---- this lane's column in this pass -----------------------------------------------------------------------------
        const unsigned desc = CELLS ? desc1 : plan.lane_tab[pt * 64 + lane];
        const int slot = (int)(desc & 0xffu), col = (int)((desc >> 8) & 0xffu);
        const bool in_use = (desc >> 17) & 1u;
        const int cs = __builtin_amdgcn_ds_bpermute(col * 4, tab_s);
        const int cw = __builtin_amdgcn_ds_bpermute(col * 4, tab_w);
        const int lm = lm0 + slot;                                   // (< L by construction of the plan, also for lanes not in use)
        const int cx = __float2int_rn(xr[lm]), cy = __float2int_rn(xr[lm + L]);      // cvRound, adaptive_vlhog.hpp:132-133
        const int x0 = cx - h, y0 = cy - h;
        int pl; unsigned wpk;
        {
            // horizontal taps: clamped in the table (cv::resize); columns on the black canvas get weight 0
            int sx = cs, a0 = (short)(cw & 0xffff), a1 = cw >> 16;
            if (sx < 0) { sx = 0; a0 = 2048; a1 = 0; }
            if (sx >= sw - 1) { sx = sw - 1; a0 = 2048; a1 = 0; }
            if (area2) { sx = 2 * col; a0 = 1024; a1 = 1024; }
            const int sx1 = (sx + 1 < sw) ? sx + 1 : sx;
            int px0 = x0 + sx, px1 = x0 + sx1;
            if (px0 < 0 || px0 >= iw || empty || !in_use) a0 = 0;
            if (px1 < 0 || px1 >= iw || empty || !in_use) a1 = 0;
            px0 = px0 < 0 ? 0 : (px0 > iw - 1 ? iw - 1 : px0);
            px1 = px1 < 0 ? 0 : (px1 > iw - 1 ? iw - 1 : px1);
            // two live taps are neighbours: ONE 16-bit load; a single live tap is paired with a zero-weight neighbour inside the row
            if (a0 != 0 && a1 != 0) {
                pl = px0; wpk = (unsigned)a0 | ((unsigned)a1 << 16);
            } else {
                const int p1 = a0 != 0 ? px0 : px1;
                const unsigned w1 = (unsigned)(a0 != 0 ? a0 : a1);
                if (p1 + 1 <= iw - 1 || p1 == 0) { pl = p1; wpk = w1; }
                else { pl = p1 - 1; wpk = w1 << 16; }
            }
        }
        const u16x2 wpk2 = __builtin_bit_cast(u16x2, wpk);
        // rows above or below the image fall outside the buffer's num_records: the hardware range check returns 0 (black canvas)
        const int vb = pl + y0 * istride;
        // ---- fold weights of the pass (matrix-core B operand) and the histogram cell column this lane receives ------------------
        f32x4 wq[4];      // (F16F: the same sixteen registers hold the float16 pieces, [k-block][piece] x 8 halfs)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            wq[i] = CELLS ? wq1[i] : (F16F ? ((const f32x4*)(plan.wb16 + ((size_t)pt * 64 + lane) * 32))[i] : ((const f32x4*)(plan.wb + ((size_t)pt * 64 + lane) * 16))[i]);
        // the pass's four words in registers (one 16-byte load, no load per segment), the lane's segment picked by selects
        const i32x4 pinfo = CELLS ? pinfo1 : *(const i32x4*)(plan.pass_info + pt * 4);
        const int sg = li < C ? 0 : (li < 2 * C ? 1 : (li < 3 * C ? 2 : 3));
        const int seg_slot = sg == 0 ? pinfo.x : (sg == 1 ? pinfo.y : (sg == 2 ? pinfo.z : -1));
        // (rows 16 mt + 4 lq + e >= 2O are skipped at the store)
        // CELLS: ... and the cell columns of a cut patch that this pass's weights leave at exact zero are not stored at all (bit 24 of
        // the lane's plan word, known here, once per pass: sdm_hog_plan.hip, plan_cut_columns; sdm_desc.hip does not load them)
        const bool recv = seg_slot >= 0 && (!CELLS || ((desc >> 24) & 1u));
        const int done = pinfo.w;
        const int nkp = (done >> 16) & 0xff;          // k-step pairs (8 lanes each) that hold columns in this pass
        // the first pass that touches a patch STORES its cells, a later one (the patch was cut) adds to them: the histogram
        // slots need no clearing, and the uncut patches no read-modify-write
        const bool first_seen = sg < 3 && ((done >> (24 + sg)) & 1);
        float* hrecv;
        if (CELLS)      // HBM: cells[sample][landmark][part][cell column][cell row][bin]; part 1 = the second pass of a cut patch.  A lane
                        // holds four consecutive bins of one cell: one 16-byte store per fold (band b = cell row b of the lane's column)
            hrecv = feat + ((((long long)s * L + lm0 + (seg_slot >= 0 ? seg_slot : 0)) * 2 + (first_seen ? 0 : 1)) * CC + (li - sg * C) * C) * (2 * O) + 4 * lq;
        else
            hrecv = hist + (seg_slot >= 0 ? hist_slot(seg_slot) : 0) * HSTR + (4 * lq) * CC + (li - sg * C);

        // ---- row loop ----------------------------------------------------------------------------------------------------------
        // the image loads of row y: the two source rows' byte offsets come from the row table (one broadcast 8-byte LDS read)
        auto issue_row = [&](int y, unsigned short& q0, unsigned short& q1) {
            const i32x2 rr = *(const i32x2*)&rowtab[SPEC ? (y >= 2 ? y - 2 : y + S - 2) : y];
            // (the row offset stays in the VECTOR offset: the hardware range check that yields the black canvas covers voffset only)
            q0 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + rr.x, 0, 0);
            q1 = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + rr.y, 0, 0);
        };
        // (the two-load loop's rows keep their low four bits here: vertical() clears them; the one-load loop's filtered() clears them itself)
        auto horizontal = [&](unsigned short q0, unsigned short q1, int& H0, int& H1) {
            H0 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, spread_bytes(q0, spread_sel)), wpk2, 0u, false);
            H1 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, spread_bytes(q1, spread_sel)), wpk2, 0u, false);
        };
        // (`cut`: the low four bits of H0 and H1 are already cleared -- the one-load loop clears them once, when a row is filtered)
        auto vertical = [&](int H0, int H1, int y, const bool cut = false) -> float {
            const i32x2 bb = *((const i32x2*)&rowtab[y] + 1);      // the row's two weights << 12
            const unsigned m = cut ? ~0u : ~15u;
            const int out = (int)((mul_hi_u24_vv((unsigned)bb.x, (unsigned)H0 & m) + mul_hi_u24_vv((unsigned)bb.y, (unsigned)H1 & m) + 2u) >> 2);
            return (float)out;
        };
        // one-load loop: the image load of row y's upper source row, and the filtered rows it carries from pixel row to pixel row
        auto issue_upper = [&](int y, unsigned short& q) {
            q = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + ((const int*)&rowtab[y >= 2 ? y - 2 : y + S - 2])[0], 0, 0);
        };
        auto filtered = [&](unsigned short q) -> int {
            return (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, spread_bytes(q, spread_sel)), wpk2, 0u, false) & ~15u);
        };
        int Hc0 = 0, Hc1 = 0;
        unsigned short qlow = 0;      // the lower source row of row 0: the only row that loads two
        // pair loop: the spare source row of pixel rows (2p + 1, 2p + 2), and what it filters to
        unsigned short qspare = 0;
        int Hsp = 0;
        auto issue_spare = [&](int p) { qspare = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + sptab[p], 0, 0); };
        float rm2 = 0.0f, rm1 = 0.0f;
        constexpr unsigned bin_stride = ST * 8;
        unsigned char* const cbase0 = (unsigned char*)colrows + lane * 8;
        // LDS byte addresses of this lane's column in bin rows 0 and 1, each in a register of its own (opaque to the optimiser:
        // otherwise the select below becomes base + select(offset, 0), one more add per pixel row)
        typedef __attribute__((address_space(3))) unsigned char lds_u8;
        typedef __attribute__((address_space(3))) f32x2 lds_f32x2;
        unsigned cadr0 = (unsigned)(size_t)(lds_u8*)cbase0, cadr1 = cadr0 + bin_stride;
        asm volatile("" : "+v"(cadr0), "+v"(cadr1));
        lds_f32x2* pend_p = (lds_f32x2*)(size_t)cadr0;
        f32x2 pend_v = {0.0f, 0.0f};
        float pend_g = 0.0f;
        int pend_yy = 0;      // WCONST: the pending row (a constant after unrolling) in the place of its weights
        int prev_by = -1;
        // fold band b (slot b & 1): hist[patch of n][bin][b][cell of n] += sum_x col[bin][x] W[x][n], clear the slot
        // `pair` (CELLS, 4 orientations; round 4): bands b and b + 1 in ONE set of products -- the 8 bin rows of band b's slot are the
        // matrix-core rows 0..7, the 8 of band b + 1's slot the rows 8..15 (idle until now) -- used for the last two bands of a pass,
        // which are complete at the same pixel row: four fold events per pass instead of five.
        auto fold_band = [&](const int b, const bool pair = false) __attribute__((always_inline)) {
            const int sl = b & 1;
            wave_sync();
            f32x4 fa0[MT], fa1[MT];
            const float* ap[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                fa0[mt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f}; fa1[mt] = fa0[mt];
                int bin_i = 16 * mt + li < 2 * O ? 16 * mt + li : 2 * O - 1;
                int sl_i = sl;
                if (pair) { bin_i = li & 7; sl_i = (li >> 3) ? (sl ^ 1) : sl; }
                ap[mt] = colrows + ((ROTB ? (int)HP_ROW_OF_BIN(bin_i) : bin_i) * ST + lq) * 2 + sl_i;
            }
            if constexpr (F16F) {
                // 16-bit matrix cores: A[row][k = 32 kb + 8 lq + j] = this lane's row of column sums at eight consecutive pixel columns
                // (stride two floats: the other band slot lies between), split into two float16 pieces; B = the weights' pieces
                typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
                const float* arow = colrows + (ROTB ? (int)HP_ROW_OF_BIN(pair ? (li & 7) : (li < 2 * O ? li : 2 * O - 1)) : (pair ? (li & 7) : (li < 2 * O ? li : 2 * O - 1))) * ST * 2
                                    + ((pair && (li >> 3)) ? (sl ^ 1) : sl) + 16 * lq;
                f32x4 facc = {0.0f, 0.0f, 0.0f, 0.0f};
                // CELLS: an operand is read AND cleared by ONE LDS instruction, an exchange with zero (ds_wrxchg_rtn_b32), instead of a
                // read here and a bank-conflicted clear of the lane's own column below: the sixteen operands of lanes (li < 8, lq) are
                // each entry of the folded slot exactly once (of both slots in a pair fold, where all sixteen li are rows), so the slot is
                // all zero afterwards as after the clears, and a wave's own LDS accesses execute in order.  The clears were the largest
                // separable part of a fold (4 % of the kernel, profiles/hog_fold_cost.txt).  Lanes li >= 8 of a one-band fold would
                // repeat row 7, and which lane of an exchange gets the value of a shared address is not promised: they stay out, and
                // whatever their registers hold feeds matrix rows 8 .. 15, whose results (lanes lq >= 2) nobody stores.
                float vx[2][8];
                if constexpr (CELLS) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) asm volatile("" : "=v"(vx[i >> 3][i & 7]));
                    if (pair || li < 2 * O) {
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            vx[i >> 3][i & 7] = __builtin_bit_cast(float, __hip_atomic_exchange((unsigned*)const_cast<float*>(&arow[64 * (i >> 3) + 2 * (i & 7)]), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
                    }
                }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = CELLS ? vx[kb][j] : arow[64 * kb + 2 * j];
                    unsigned hp_[4], lp_[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // first piece: v cut to float16's eleven significant bits, which is what the conversion toward zero does to a
                        // float16-normal v -- and v is zero or normal: a non-zero column sum is a sum of non-negative terms
                        // magnitude (>= 1 for a non-zero integer gradient) x band-slot weight (>= 1 / (2 cell)) x 8, each
                        // >= 8 / 24 > 2^-14, and the static_assert above bounds it below 65 504.  Second piece: v minus the first,
                        // exact in float32, by one mixed-precision multiply-add (v_fma_mix_f32) per value.  Four vector instructions
                        // per pair of values (six with the piece cut out by a mask first), the same bits.
                        // (The feature-row form keeps the mask: at its 80 registers the shorter split made cells 10 and 8 spill.)
                        if constexpr (CELLS) {
                            const auto hh = __builtin_amdgcn_cvt_pkrtz(v[2 * e], v[2 * e + 1]);
                            hp_[e] = __builtin_bit_cast(unsigned, hh);
                            lp_[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)hh[0], neg_one, v[2 * e]),
                                                                                             __builtin_fmaf((float)hh[1], neg_one, v[2 * e + 1])));
                        } else {
                            const float h0 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v[2 * e]) & 0xffffe000u);
                            const float h1 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v[2 * e + 1]) & 0xffffe000u);
                            hp_[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(h0, h1));
                            lp_[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(v[2 * e] - h0, v[2 * e + 1] - h1));
                        }
                    }
                    typedef unsigned u32x4f __attribute__((ext_vector_type(4)));
                    const f16x8 ah = __builtin_bit_cast(f16x8, (u32x4f){hp_[0], hp_[1], hp_[2], hp_[3]});
                    const f16x8 al = __builtin_bit_cast(f16x8, (u32x4f){lp_[0], lp_[1], lp_[2], lp_[3]});
                    const f16x8 bh = __builtin_bit_cast(f16x8, wq[2 * kb]), bl = __builtin_bit_cast(f16x8, wq[2 * kb + 1]);
                    facc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bl, facc, 0, 0, 0);
                    facc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, facc, 0, 0, 0);
                    facc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, facc, 0, 0, 0);
                    facc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, facc, 0, 0, 0);
                }
                fa0[0] = facc * (1.0f / 8192.0f);      // 8 (column sums) x 2^10 (weights)
                // fa1[0] stays zero: the stores below add the two accumulators
            } else {
            // the operand reads run two k-step pairs ahead of the products (the scheduling barriers keep that order: with the
            // reads serialised behind the products every fold cost eight LDS round trips)
            float a0v[MT][3], a1v[MT][3];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 2; ++i) { a0v[mt][i] = ap[mt][16 * i]; a1v[mt][i] = ap[mt][16 * i + 8]; }
#pragma unroll
            for (int kp = 0; kp < 8; ++kp) {
                if (kp + 2 < 8) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) { a0v[mt][(kp + 2) % 3] = ap[mt][16 * (kp + 2)]; a1v[mt][(kp + 2) % 3] = ap[mt][16 * (kp + 2) + 8]; }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (kp < 6 || kp < nkp) {      // (a 55-column pass leaves the last 8 lanes without a column: 14 products instead of 16)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        fa0[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0v[mt][kp % 3], wq[(2 * kp) >> 2][(2 * kp) & 3], fa0[mt], 0, 0, 0);
                        fa1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[mt][kp % 3], wq[(2 * kp + 1) >> 2][(2 * kp + 1) & 3], fa1[mt], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            }
            // every lane clears the slot(s) of its own pixel column (the LDS unit executes this wave's accesses in order)
            if (CELLS && F16F) { }      // (cleared by the operand exchange above)
            else if (pair) {
#pragma unroll
                for (int k = 0; k < 2 * O; ++k) *(f32x2*)((float*)cbase0 + k * ST * 2) = (f32x2){0.0f, 0.0f};
            } else {
                float* cz = (float*)cbase0 + sl;
#pragma unroll
                for (int k = 0; k < 2 * O; ++k) cz[k * ST * 2] = 0.0f;
            }
            if (CELLS) {
                if (recv) {
                    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(8)));
                    if (pair) {      // rows 4 lq .. 4 lq + 3: bins 4 (lq & 1) .. of band b + (lq >> 1)
                        float* hf = hrecv + (b + (lq >> 1)) * (2 * O) - 4 * lq + 4 * (lq & 1);
                        *(f32x4u*)hf = fa0[0] + fa1[0];
                    } else {
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            float* hf = hrecv + b * (2 * O) + 16 * mt;
                            const int left = 2 * O - (16 * mt + 4 * lq);      // bins from this lane's first one to the last
                            if (left >= 4) *(f32x4u*)hf = fa0[mt] + fa1[mt];
                            else if (left >= 2) *(f32x2*)hf = (f32x2){fa0[mt][0] + fa1[mt][0], fa0[mt][1] + fa1[mt][1]};
                        }
                    }
                }
            } else if (recv) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    float* hf = hrecv + b * C + 16 * mt * CC;
                    if (first_seen) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (16 * mt + 4 * lq + e < 2 * O) hf[e * CC] = fa0[mt][e] + fa1[mt][e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (16 * mt + 4 * lq + e < 2 * O) hf[e * CC] += fa0[mt][e] + fa1[mt][e];
                    }
                }
            }
            wave_sync();
        };
        unsigned short q0[2], q1[2];
        // `loop`: 0 = two loads per pixel row, 1 = one load (row carry), 2 = three loads per two pixel rows (pair carry)
        auto row_step = [&](const int j, const int y, const bool grad, auto loop) __attribute__((always_inline)) {
            int H0, H1;
            constexpr int LOOP = decltype(loop)::value;
            if constexpr (LOOP == 2) {
                // as below; the first row of a pair (odd y) filters the pair's spare and issues the next pair's
                const int Hn = filtered(q1[j]);
                if (y == 0) Hc0 = filtered(qlow);
                else {
                    if (y & 1) {
                        Hsp = filtered(qspare);
                        if (y + 2 < S) issue_spare((y + 2) >> 1);
                    }
                    const unsigned mk = (unsigned)((const int*)&rowtab[y])[1];
                    Hc0 = (int)(((unsigned)Hsp & mk) | ((unsigned)Hc1 & ~mk));
                }
                Hc1 = Hn; H0 = Hc0; H1 = Hc1;
                if (y + 2 < S) issue_upper(y + 2, q1[j]);
            } else if constexpr (LOOP == 1) {
                // no branch, lane read or compare here: the mask comes with the weights in the row's one broadcast LDS read
                const int Hn = filtered(q1[j]);
                if (y == 0) Hc0 = filtered(qlow);
                else {
                    const unsigned mk = (unsigned)((const int*)&rowtab[y])[1];
                    Hc0 = (int)(((unsigned)Hc1 & mk) | ((unsigned)Hc0 & ~mk));
                }
                Hc1 = Hn; H0 = Hc0; H1 = Hc1;
                if (y + 2 < S) issue_upper(y + 2, q1[j]);
            } else {
                horizontal(q0[j], q1[j], H0, H1);
                if (!SPEC || y + 2 < S) issue_row(y + 2, q0[j], q1[j]);      // (generic: past the last row a harmless extra load of the last row)
            }
            f32x2 qv = {0.0f, 0.0f};
            if (grad) qv = *pend_p;
            const float r0 = vertical(H0, H1, y, LOOP != 0);
            if (grad) {
                const int yy = y - 1;                      // gradient of row y - 1 (hog.c:616-672)
                float gx, gy, g2;
                if constexpr (WCONST) {
                    // the two differences and the two squares written as the packed operations they compile to: left to the compiler,
                    // the cell-11 instance with the weights in registers had them unpacked in one of its loops (51 vector instructions)
                    typedef float g_v2 __attribute__((ext_vector_type(2)));
                    const g_v2 gv = (g_v2){from_right(rm1), r0} - (g_v2){from_left(rm1), rm2};
                    const g_v2 gq = gv * gv;
                    gx = gv.x; gy = gv.y; g2 = gq.x + gq.y;
                } else {      // (the feature-row form spills with the packed form: 12 bytes of scratch at cells 11 / 10 / 8)
                    gx = from_right(rm1) - from_left(rm1);
                    gy = r0 - rm2;
                    g2 = gx * gx + gy * gy;
                }
                const float gm = RAW ? __builtin_amdgcn_sqrtf(g2) : sqrt_int_up(g2);
                bool b0 = false, b1 = false, b2 = false;
                int bin_any = 0;
                unsigned rot_ux = 0, rot_uy = 0, rot_uw = 0;
                if constexpr (ROTB) {
                    typedef float v2 __attribute__((ext_vector_type(2)));
                    const v2 rr = __builtin_elementwise_fma((v2){gy, gy}, (v2){HP_ROT_S, HP_ROT_C}, (v2){gx, gx} * (v2){HP_ROT_C, -HP_ROT_S});
                    const float rw = __builtin_fabsf(rr.x) - __builtin_fabsf(rr.y);
                    b0 = rw < 0.0f; b1 = rr.y < 0.0f; b2 = rr.x < 0.0f;      // row = b0 + 2 b1 + 4 b2
                    // (sign bits: -0.0f would differ from "< 0", but x', y' and |x'| - |y'| are never zero for a non-zero integer
                    //  gradient, and a zero gradient adds 0 to whichever row it lands in -- verify_fast_bins_kernel checks the bits)
                    // (scalar copies first: __builtin_bit_cast applied to the vector ELEMENT rr.y reads element 0 with this compiler)
                    const float rx1 = rr.x, ry1 = rr.y;
                    rot_ux = __builtin_bit_cast(unsigned, rx1); rot_uy = __builtin_bit_cast(unsigned, ry1); rot_uw = __builtin_bit_cast(unsigned, rw);
                } else if constexpr (TO == 4) bin_sector4_bits(gx, gy, lv, b0, b1, b2);
                else bin_sector<TO>(gx, gy, lv, TO, bin_any);      // (a zero gradient lands in bin 0 with magnitude 0)
                // column sums by fused multiply-add: one v_pk_fma_f32 instead of a multiply and an add per pixel
                *pend_p = WCONST ? add_row(pend_yy, pend_g, qv) : __builtin_elementwise_fma(pend_v, (f32x2){pend_g, pend_g}, qv);
                const float* rt = lv.row_tab[yy];
                f32x2 wsv;
                if (WCONST) wsv = (f32x2){0.0f, 0.0f};      // (add_row takes the row's weights from the registers)
                else if (SPEC) wsv = wstab[yy - 1];
                else wsv = (f32x2){rt[0], rt[1]};
                const float ws0 = wsv.x, ws1 = wsv.y;
                // (specialised instance: yy and with it the band are constants after unrolling; prev_by folds away)
                const int cby = CELL > 0 ? packed_band_of(yy, CELL) : __builtin_bit_cast(int, rt[2]);
                if (cby != prev_by) {
                    // Detect instances: band C - 2 is not folded where band C - 1's rows begin but together with it, in the closing pair
                    // fold behind the loop -- four fold events per pass, not five.  The rows of band C - 1 leave its slot as it is: their
                    // weight for that slot is the one of cell row C, which does not exist and is zero in the row table (fill_row_tab), and
                    // fma(0, g, q) is q for a finite g and a column sum q, which is never -0.  (The pair fold was written for this; the row
                    // loop folded band C - 2 at the boundary all the same, so the closing call only ever saw band C - 1 alone:
                    // profiles/hog_fold_overlap.txt.)
                    if (CELLS && F16F && cby == C - 1 && prev_by == C - 2) { }
                    else {
                        if (prev_by >= 0) fold_band(prev_by);
                        prev_by = cby;
                    }
                }
                if constexpr (ROTB) {
                    // the octant code straight from the three sign bits (shifts and shift-ors instead of three compares and three selects)
                    // v_alignbit_b32(hi, lo, 31) = (hi << 1) | (lo >> 31): one instruction per further sign bit
                    const unsigned code = __builtin_amdgcn_alignbit(__builtin_amdgcn_alignbit(rot_ux >> 31, rot_uy, 31), rot_uw, 31);
                    pend_p = (lds_f32x2*)(size_t)(cadr0 + code * bin_stride);
                } else if constexpr (TO == 4)
                    pend_p = (lds_f32x2*)(size_t)((b0 ? cadr1 : cadr0) + ((b1 ? 2u * bin_stride : 0u) + (b2 ? 4u * bin_stride : 0u)));
                else
                    pend_p = (lds_f32x2*)(size_t)(cadr0 + (unsigned)bin_any * bin_stride);
                pend_v = (f32x2){ws0, ws1}; pend_g = gm; pend_yy = yy;
            }
            rm2 = rm1; rm1 = r0;
        };
        constexpr std::integral_constant<int, 0> two_loads{};
        auto two_load_rows = [&]() __attribute__((always_inline)) {
            issue_row(0, q0[0], q1[0]);
            issue_row(1, q0[1], q1[1]);
            row_step(0, 0, false, two_loads);
            row_step(1, 1, false, two_loads);
            if constexpr (CELL > 0) {
#pragma unroll
                for (int yrow = 2; yrow < SC; ++yrow) row_step(yrow & 1, yrow, true, two_loads);
            } else {
                int yrow = 2;
                for (; yrow + 1 < S; yrow += 2) {
                    row_step(0, yrow, true, two_loads);
                    row_step(1, yrow + 1, true, two_loads);
                }
                if (yrow < S) row_step(0, yrow, true, two_loads);
            }
        };
        if constexpr (CARRY) {
            if (carry) {      // wave-uniform, once per pass: the loops themselves hold no branch
                constexpr std::integral_constant<int, 1> one_load{};
                qlow = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + __builtin_amdgcn_readlane(row_ent.x, 0), 0, 0);
                issue_upper(0, q1[0]);
                issue_upper(1, q1[1]);
                row_step(0, 0, false, one_load);
                row_step(1, 1, false, one_load);
#pragma unroll
                for (int yrow = 2; yrow < SC; ++yrow) row_step(yrow & 1, yrow, true, one_load);
            } else two_load_rows();
        } else if constexpr (PAIR) {
            if (carry) {      // wave-uniform, once per pass, as above
                constexpr std::integral_constant<int, 2> pair_load{};
                qlow = __builtin_amdgcn_raw_buffer_load_b16(img_rsrc, vb + __builtin_amdgcn_readlane(row_ent.x, 0), 0, 0);
                issue_upper(0, q1[0]);
                issue_upper(1, q1[1]);
                issue_spare(0);
                row_step(0, 0, false, pair_load);
                row_step(1, 1, false, pair_load);
#pragma unroll
                for (int yrow = 2; yrow < SC; ++yrow) row_step(yrow & 1, yrow, true, pair_load);
            } else two_load_rows();
        } else two_load_rows();
        *pend_p = WCONST ? add_row(pend_yy, pend_g, *pend_p) : __builtin_elementwise_fma(pend_v, (f32x2){pend_g, pend_g}, *pend_p);
        if (CELLS && TO == 4 && prev_by >= 0 && prev_by + 1 <= C - 1) fold_band(prev_by, true);
        else {
            if (prev_by >= 0) fold_band(prev_by);
            if (prev_by + 1 <= C - 1) fold_band(prev_by + 1);
        }
        wave_sync();

        // ---- patches whose last column was in this pass: normalise, store, free the histogram slot -----------------------------
        const int dfirst = done & 0xff, dcount = (done >> 8) & 0xff;
        for (int j = 0; j < dcount; ++j) {
            const int ps = dfirst + j, lmp = lm0 + ps;
            if (!CELLS) {
                float* hp = hist + hist_slot(ps) * HSTR;
                hog_finish_direct<TO, TC>(hp, scratch, out_row + (long long)lmp * lv.P, lv, lane);
                // the scratch sat on the column rows, which the next pass expects to be zero
                for (int i = lane; i < (int)(packed_scratch_bytes(C, O) / 16); i += 64) ((f32x4*)scratch)[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            }
            if (idx_row && lane == 0) {
                if (lmp == 0) idx_row[0] = h;
                idx_row[1 + lmp] = __float2int_rn(xr[lmp]);
                idx_row[1 + L + lmp] = __float2int_rn(xr[lmp + L]);
            }
            // bias, adaptive_vlhog.hpp:182-183 (the non-adaptive example transform has none)
            if (!CELLS && lmp == L - 1 && lv.fixed_h == 0 && lane == 0) out_row[(long long)L * lv.P] = 1.0f;
            if (!CELLS) wave_sync();
        }
    }
}

// cv::resize's taps depend on the level and on the patch half-width h only: one table per level, [h < SDM_SCALE_TAB][64 coordinates]
// x {s0, c0 | c1 << 16, sy0, sy1, b0 << 12, b1 << 12, carry mask, one-load eligible}, built once per geometry by the device function the kernels used to call
// per wave (so the bits are the ones they computed).  Round 4: ~80 vector instructions (double-precision coordinate arithmetic,
// conversions, clamps) per wave leave the pixel kernel's set-up -- a third of its instructions outside the row loop at the small levels.
// Row carry: half-width h is one-load eligible when the lower source row sy0 of every resized row d >= 1 is one of the two rows
// (sy0, sy1) of row d - 1 -- decided from the taps as computed here, clamped first row and clipped last rows included; never for an
// empty patch or the exact-2x reduction.  The mask of row d says which: all ones = row d - 1's sy1, zero = its sy0.
__global__ void taps_table_kernel(HogLevelDev lv, int* __restrict__ table)
{
    const int h = blockIdx.x, d = threadIdx.x;
    const int S = lv.S;
    const bool empty = h <= 0;
    const int sw = empty ? 1 : 2 * h;
    const bool area2 = (sw == 2 * S);
    const double scale = resize_scale(lv, h, sw);
    const ResizeTaps tp = resize_taps(d < S ? d : S - 1, scale, sw, area2);
    i32x4* e = (i32x4*)(table + ((size_t)h * 64 + d) * 8);
    e[0] = (i32x4){tp.s0, (tp.c0 & 0xffff) | (tp.c1 << 16), tp.sy0, tp.sy1};
    const int p0 = __shfl_up(tp.sy0, 1), p1 = __shfl_up(tp.sy1, 1);      // (one wave per half-width)
    const bool held = d == 0 || d >= S || tp.sy0 == p0 || tp.sy0 == p1;
    const bool eligible = !empty && !area2 && __ballot(!held) == 0;
    e[1] = (i32x4){tp.b0 << 12, tp.b1 << 12, (d >= 1 && tp.sy0 == p1) ? -1 : 0, eligible ? 1 : 0};
}

// Pair carry: per (level, h) a table of its own, [h < SDM_SCALE_TAB][64] x {take-the-spare mask of row d, source row of the spare of
// pair d = pixel rows (2d + 1, 2d + 2) or -1 where the pair has no orphan, half-width is pair eligible, orphan rows of the patch}, from
// the same taps.  Row d >= 1 is a shift row when sy0 equals row d - 1's sy1, an orphan row when it is the row after that; h is pair
// eligible when the patch is neither empty nor the exact-2x reduction, every row d >= 1 is one of the two, no pair (2p + 1, 2p + 2)
// holds two orphans and a last row without a partner (even S) is a shift row.  Row 0 loads its two rows itself.
__global__ void pair_taps_table_kernel(HogLevelDev lv, int* __restrict__ table)
{
    const int h = blockIdx.x, d = threadIdx.x;
    const int S = lv.S;
    const bool empty = h <= 0;
    const int sw = empty ? 1 : 2 * h;
    const bool area2 = (sw == 2 * S);
    const double scale = resize_scale(lv, h, sw);
    const ResizeTaps tp = resize_taps(d < S ? d : S - 1, scale, sw, area2);
    const int p1 = __shfl_up(tp.sy1, 1);      // (one wave per half-width)
    const bool row = d >= 1 && d < S;
    const bool orphan = row && tp.sy0 == p1 + 1;
    const bool shift = row && tp.sy0 == p1;
    const int npairs = (S - 1) / 2;
    const unsigned long long orphans = __ballot(orphan);
    const bool two = (d & 1) && d <= 2 * npairs && orphan && ((orphans >> (d + 1)) & 1);      // both rows of pair (d, d + 1)
    const bool bad = (row && !shift && !orphan) || two || (d > 2 * npairs && d < S && !shift);
    const bool eligible = !empty && !area2 && __ballot(bad) == 0;
    // lane p: the spare of pixel rows (2p + 1, 2p + 2)
    const int ra = __shfl(tp.sy0, (2 * d + 1) & 63), rb = __shfl(tp.sy0, (2 * d + 2) & 63);
    int spare = -1;
    if (d < npairs) spare = ((orphans >> (2 * d + 1)) & 1) ? ra : (((orphans >> (2 * d + 2)) & 1) ? rb : -1);
    ((i32x4*)table)[(size_t)h * 64 + d] = (i32x4){orphan ? -1 : 0, spare, eligible ? 1 : 0, (int)__popcll(orphans)};
}

}  // namespace

template <bool CELLS>
static void launch_hog_packed(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                              const EyeIdxDev& eyes, const HogLevelDev& lv, const HogPlanDev& plan, float* feat, long long ldf,
                              int* idx_out, int* status, hipStream_t stream)
{
    const int gpf = CELLS ? plan.n_main * plan.P + plan.Pt : plan.n_main + (plan.Gt > 0 ? 1 : 0);
    const long long total = (long long)N * gpf;
    if (total <= 0) return;
    const unsigned grid = (unsigned)((total + HP_WAVES - 1) / HP_WAVES);
#define HP_LAUNCH_O(TO, CELL, RAW)                                                                                              \
    hipLaunchKernelGGL((hog_packed_kernel<TO, 5, CELL, RAW, CELLS>), dim3(grid), dim3(HP_WAVES * 64),                              \
                       packed_wg_lds_bytes(5, TO, lv.S, CELLS ? 0 : plan.hist_slots, CELL > 0, hp_pair_slots(CELL, 5, CELLS, RAW), !hp_const_weights(TO, CELL, CELLS, RAW)), stream, imgs, img_idx, x, N, L,  \
                       eyes, lv, plan, feat, ldf, idx_out, status)
#define HP_LAUNCH(CELL, RAW) HP_LAUNCH_O(4, CELL, RAW)
    if (lv.O == 9) {      // "31-bin" HOG (9 orientations, hog.c:212-215): 18 bin rows = two matrix-core row tiles per band fold
        static unsigned long long attr9 = 0;
        if (sdm_first_use_on_device(attr9)) {
            SDM_SET_ATTR((const void*)hog_packed_kernel<9, 5, 0, true, CELLS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            SDM_SET_ATTR((const void*)hog_packed_kernel<9, 5, 0, false, CELLS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        }
        if (plan.raw_sqrt) HP_LAUNCH_O(9, 0, true); else HP_LAUNCH_O(9, 0, false);
        return;
    }
    // instances specialised on the shipped cell sizes (apps/rcr/rcr-train.cpp:447: 11, 10, 8, 6); any other cell size or a level
    // whose fast-arithmetic verdict is negative run the generic instance
    if (!plan.raw_sqrt) { HP_LAUNCH(0, false); return; }
    switch (lv.cell) {
    case 11: HP_LAUNCH(11, true); break;
    case 10: HP_LAUNCH(10, true); break;
    case 8: HP_LAUNCH(8, true); break;
    case 6: HP_LAUNCH(6, true); break;
    default: HP_LAUNCH(0, true); break;
    }
#undef HP_LAUNCH
#undef HP_LAUNCH_O
}

void sdm_launch_hog_packed(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                           const EyeIdxDev& eyes, const HogLevelDev& lv, const HogPlanDev& plan, float* feat, long long ldf,
                           int* idx_out, int* status, hipStream_t stream)
{
    launch_hog_packed<false>(imgs, img_idx, x, N, L, eyes, lv, plan, feat, ldf, idx_out, status, stream);
}

// the same launch stopping at the raw cell histograms: cells[N][L][2 parts][C*C][2O] floats (see hog_packed_kernel, CELLS)
void sdm_launch_hog_cells(const ImageSetDev& imgs, const int* img_idx, const float* x, int N, int L,
                          const EyeIdxDev& eyes, const HogLevelDev& lv, const HogPlanDev& plan, float* cells,
                          int* idx_out, int* status, hipStream_t stream)
{
    launch_hog_packed<true>(imgs, img_idx, x, N, L, eyes, lv, plan, cells, 0, idx_out, status, stream);
}

// whether sdm_launch_hog_cells runs this level on an instance that holds the one-load row loop (the dispatch above)
bool sdm_hog_cells_row_carry(const HogLevelDev& lv, const HogPlanDev& plan)
{
    return lv.O == 4 && plan.raw_sqrt && plan.taps && hp_row_carry(lv.cell);
}

void sdm_launch_taps_table(const HogLevelDev& lv, int* table, hipStream_t stream)
{
    hipLaunchKernelGGL(taps_table_kernel, dim3(SDM_SCALE_TAB), dim3(64), 0, stream, lv, table);
}

// whether sdm_launch_hog_cells runs this level on an instance that holds the pair loop
bool sdm_hog_cells_pair_carry(const HogLevelDev& lv, const HogPlanDev& plan)
{
    return lv.O == 4 && lv.C == 5 && plan.raw_sqrt && plan.taps && plan.pair_taps && hp_pair_carry(lv.cell);
}

void sdm_launch_pair_taps_table(const HogLevelDev& lv, int* table, hipStream_t stream)
{
    hipLaunchKernelGGL(pair_taps_table_kernel, dim3(SDM_SCALE_TAB), dim3(64), 0, stream, lv, table);
}
