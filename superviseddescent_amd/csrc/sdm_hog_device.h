// sdm_hog_device.h -- device helpers shared by the two HOG pixel-kernel families: the one-patch-per-wave kernels
// (sdm_hog_fast.hip) and the lane-packed kernel (sdm_hog_packed.hip).  Inter-eye distance, cv::resize's tap arithmetic, the
// wavefront shifts, the integer-domain square roots, the orientation binning forms that sdm_launch_verify_fast_bins compares,
// and the wave-level synchronisation.  Everything here has internal linkage: each of the two translation units compiles its
// own copy, as when they were one file.
#pragma once
#include "sdm_kernels.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline double ied_of(const float* __restrict__ xr, int L, const EyeIdxDev& e)
{
    float rx = 0.0f, ry = 0.0f, lx = 0.0f, ly = 0.0f;
    for (int i = 0; i < e.nre; ++i) { rx += xr[e.re[i]]; ry += xr[e.re[i] + L]; }
    // (helpers.hpp:143-157 divides the f32 sums by the count; for a power of two that is exactly this multiplication)
    if (e.inv_nre != 0.0f) { rx *= e.inv_nre; ry *= e.inv_nre; } else { rx /= (float)e.nre; ry /= (float)e.nre; }
    for (int i = 0; i < e.nle; ++i) { lx += xr[e.le[i]]; ly += xr[e.le[i] + L]; }
    if (e.inv_nle != 0.0f) { lx *= e.inv_nle; ly *= e.inv_nle; } else { lx /= (float)e.nle; ly /= (float)e.nle; }
    float dxf = rx - lx, dyf = ry - ly;
    double dx = dxf, dy = dyf;
    return sqrt(dx * dx + dy * dy);
}

__device__ inline int sat_short_f(float v)
{
    int i = __float2int_rn(v);
    return i > 32767 ? 32767 : (i < -32768 ? -32768 : i);
}

__device__ inline int vl_floor(float x)
{
    int xi = (int)x;
    if (x >= 0 || (float)xi == x) return xi;
    return xi - 1;
}

// lane i <- lane i-1 / lane i+1 (DPP wavefront shifts; lane 0 / lane 63 receive 0)
__device__ inline float from_left(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ inline float from_right(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

// Correctly rounded sqrt for the values that occur here (sums of two squared u8 differences: integers <= 130050):
// the hardware approximation (<= 1 ulp) corrected by one residual test on each neighbour, without the denormal
// scaling of the general-purpose sqrtf.  Used only after sdm_verify_fast_bins found it bit-identical to sqrtf on
// every possible input.
__device__ inline float sqrt_int_exact(float x)
{
    const float r = __builtin_amdgcn_sqrtf(x);
    const float rm = __builtin_bit_cast(float, __builtin_bit_cast(int, r) - 1);
    const float rp = __builtin_bit_cast(float, __builtin_bit_cast(int, r) + 1);
    const float em = __builtin_fmaf(-rm, r, x);
    const float ep = __builtin_fmaf(-rp, r, x);
    float y = (em <= 0.0f) ? rm : r;
    y = (ep > 0.0f) ? rp : y;
    return y;
}

// One-sided form: on gfx950 v_sqrt_f32 is never above the correctly rounded root for these inputs (it is exact or one
// ulp low: scripts/ubench/sqrt_domain.hip), so only the upper neighbour is tested.  Like everything else here it is
// used only after the exhaustive on-device comparison with sqrtf.
__device__ inline float sqrt_int_up(float x)
{
    const float r = __builtin_amdgcn_sqrtf(x);
    const float rp = __builtin_bit_cast(float, __builtin_bit_cast(int, r) + 1);
    const float ep = __builtin_fmaf(-rp, r, x);
    return (ep > 0.0f) ? rp : r;
}

// reference arithmetic, hog.c:637-672 (identical to sdm_hog.hip::gradient_bin)
__device__ inline void bin_reference(float gx, float gy, float g, const HogLevelDev& lv, int& bin)
{
    float nx = g > 0.0f ? gx / g : 0.0f;
    float ny = g > 0.0f ? gy / g : 0.0f;
    float best = 0.0f;
    bin = -1;
    for (int k = 0; k < lv.O; ++k) {
        float s = nx * lv.ox[k] + ny * lv.oy[k];
        int b = k;
        if (s < 0) { s = -s; b += lv.O; }
        if (s > best) { best = s; bin = b; }
    }
}

// shortcut: same arg-max on the un-normalised gradient (verified exhaustively per level, see
// sdm_verify_fast_bins); the scores only need to ORDER correctly, so FMA is fine here.
__device__ inline void bin_unnormalised(float gx, float gy, const HogLevelDev& lv, int& bin)
{
    float best = 0.0f;
    bin = -1;
    for (int k = 0; k < lv.O; ++k) {
        float s = __builtin_fmaf(gx, lv.ox[k], gy * lv.oy[k]);
        int b = s < 0 ? k + lv.O : k;
        s = __builtin_fabsf(s);
        if (s > best) { best = s; bin = b; }
    }
}

// Sector method: fold the gradient into the half plane gy > 0 (or gy == 0, gx > 0), count how many of the floor(O/2)
// sector boundaries tan((2j+1)pi/2O) the slope |gy|/|gx| exceeds -> index m of the nearest orientation in the first
// quadrant, then unfold (second quadrant: O - m; flipped half plane: + O).  ~3 instructions per boundary instead of
// ~6 per orientation; used only after the exhaustive on-device comparison with the reference arithmetic.
template <int TO>
__device__ inline void bin_sector(float gx, float gy, const HogLevelDev& lv, int O, int& bin)
{
    // (gy == 0, gx < 0) needs no fold: m = 0 and the second-quadrant rule already yields O.  A zero gradient yields
    // bin 0 here where the reference selects nothing: its magnitude is 0, so it contributes exact zeros either way.
    const bool flip = gy < 0.0f;
    const float fx = flip ? -gx : gx;
    const float a = __builtin_fabsf(gx), b = __builtin_fabsf(gy);
    int m = 0;
#pragma unroll
    for (int j = 0; j < (TO ? TO / 2 : SDM_MAX_ORIENT / 2); ++j) {
        if (TO == 0 && j >= lv.n_sector) break;
        m += (b > a * lv.sector_t[j]) ? 1 : 0;
    }
    int d = (fx >= 0.0f) ? m : O - m;
    d += flip ? O : 0;
    if (TO > 0 && ((2 * TO) & (2 * TO - 1)) == 0) bin = d & (2 * TO - 1);      // d <= 2O: the wrap is a mask for 2O = 2^k
    else bin = d >= 2 * O ? d - 2 * O : d;
}

// The same for 4 orientations, as the three bits of the directed bin (8 bins of 45 degrees).  With A = |gy| > |gx| t0,
// B = |gy| > |gx| t1 (B implies A: m = A + B), X = gx < 0, Y = gy < 0 and s = X xor Y (= fx < 0 above whenever it matters:
// for gx == 0 both boundaries are exceeded, m = 2, and d = 2 either way):  d = s ? 4 - m : m has bit0 = A & ~B,
// bit1 = (bit0 & s) | B, bit2 = s & ~A, and bin = (d + 4 Y) mod 8 only flips bit2.  Checked against bin_sector for all
// 511 x 511 gradients by verify_fast_bins_kernel.
__device__ inline void bin_sector4_bits(float gx, float gy, const HogLevelDev& lv, bool& b0, bool& b1, bool& b2)
{
    const float a = __builtin_fabsf(gx), b = __builtin_fabsf(gy);
    const bool A = b > a * lv.sector_t[0], B = b > a * lv.sector_t[1];
    const bool X = gx < 0.0f, Y = gy < 0.0f;
    const bool s = X != Y;
    b0 = A != B;
    b1 = (b0 && s) || B;
    b2 = (s && !A) != Y;
}

// Round 4: the same eight sectors on coordinates rotated by -22.5 degrees, where the sector boundaries are the two axes and the
// two diagonals: octant code = 4 [x' < 0] + 2 [y' < 0] + [|x'| < |y'|] -- three sign tests, no scalar boolean chain (the three
// bits above cost five scalar instructions per pixel row, and every scalar instruction takes an issue slot beside the vector
// ones).  The code is NOT the bin: bin j lives in column-sum row HP_ROW_OF_BIN(j), and the band folds read their matrix-core
// rows through that permutation, so the histograms come out in bin order.  Used only when verify_fast_bins_kernel found the
// code's bin equal to the reference's on all 511 x 511 gradients (counter 3).
#define HP_ROT_C 0.92387953251128674f      /* cos(pi / 8) */
#define HP_ROT_S 0.38268343236508977f      /* sin(pi / 8) */
#define HP_ROW_OF_BIN(j) ((0x37645102u >> (4 * (j))) & 7u)      /* bins 0..7 -> rows 2 0 1 5 4 6 7 3 */
__device__ inline int bin_rot4_row(float gx, float gy)
{
    typedef float v2 __attribute__((ext_vector_type(2)));
    const v2 r = __builtin_elementwise_fma((v2){gy, gy}, (v2){HP_ROT_S, HP_ROT_C}, (v2){gx, gx} * (v2){HP_ROT_C, -HP_ROT_S});
    const float w = __builtin_fabsf(r.x) - __builtin_fabsf(r.y);
    // the kernel takes the SIGN BITS (a -0.0f would count as negative): checked here in that form
    // (scalar copies first: __builtin_bit_cast applied to the vector ELEMENT r.y reads element 0 with this compiler)
    const float rx1 = r.x, ry1 = r.y;
    return (int)((((__builtin_bit_cast(unsigned, rx1) >> 31) << 1 | (__builtin_bit_cast(unsigned, ry1) >> 31)) << 1) | (__builtin_bit_cast(unsigned, w) >> 31));
}

__host__ __device__ inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// Every LDS region belongs to one wave, and the LDS unit executes one wave's instructions in issue order, so the
// phases of a patch only need the compiler to keep that order: a wavefront-scope fence, no workgroup barrier (the
// four waves of a workgroup never wait for each other).
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// the two source bytes of a 16-bit load -> the two 16-bit halves of a register {b0, 0, b1, 0} (v_perm_b32 reads the loaded
// register as it is: no zero-extension instruction), ready for v_dot2_u32_u16 with the packed tap weights
#define HF_SPREAD_SEL 0x0c010c00u
__device__ inline unsigned spread_bytes(unsigned short v, unsigned sel)
{
    unsigned r;
    u16x2 t;            // (the upper half stays undefined on purpose: a 16 -> 32 bit conversion would cost a v_and)
    t.x = v;
    asm("v_perm_b32 %0, 0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(unsigned, t)), "v"(sel));
    return r;
}

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// cv::resize's taps of destination coordinate d for a 2h x 2h -> S x S bilinear 8-bit resize (resize.cpp, restated in
// SURVEY.md row a-2r): unclamped source index s0 = floor((d + 0.5) scale - 0.5), the 11-bit weights c0, c1 of s0 and s0 + 1,
// and the vertical form (rows clipped to the patch, the fraction kept; the exact-2x reduction as weights 1024 on rows 2d, 2d+1).
struct ResizeTaps { int s0, c0, c1, sy0, sy1, b0, b1; };
__device__ inline ResizeTaps resize_taps(int d, double scale, int sw, bool area2)
{
    ResizeTaps t;
    float f = (float)((d + 0.5) * scale - 0.5);
    t.s0 = (int)floorf(f);
    f -= (float)t.s0;
    t.c0 = sat_short_f((1.f - f) * 2048.0f);
    t.c1 = sat_short_f(f * 2048.0f);
    t.sy0 = t.s0 < 0 ? 0 : (t.s0 > sw - 1 ? sw - 1 : t.s0);
    t.sy1 = t.s0 + 1 < 0 ? 0 : (t.s0 + 1 > sw - 1 ? sw - 1 : t.s0 + 1);
    t.b0 = t.c0; t.b1 = t.c1;
    if (area2) { t.sy0 = 2 * d; t.sy1 = 2 * d + 1; t.b0 = 1024; t.b1 = 1024; }
    return t;
}
__device__ inline double resize_scale(const HogLevelDev& lv, int h, int sw)
{
    return (h < SDM_SCALE_TAB) ? lv.scale_tab[h > 0 ? h : 0] : 1.0 / ((double)lv.S / (double)sw);
}

}  // namespace
