// sdm_track_motion_device.h -- the arithmetic of the tracker's motion-compensated initialisation (include/sdm.h, "Tracking,
// motion-compensated"): per slot a 32 x 32 reference chip of block means around the face, and before the next step's cascade a
// block-matching search for the translation that takes the chip into the new frame.  Integer throughout, except the grid's cell
// size and centre, which come from the row's float32 bounds.
// Plain C++ behind TRACK_MOTION_HD: the device code of track_motion_store_kernel and track_motion_search_kernel
// (csrc/sdm_track_motion.hip) and, compiled for the host, of tests/cpp/track_motion_host.cpp, which runs it under the host sanitizers
// on frames, chips and column sums in heap blocks of exactly their bytes.
//
// A grid of cells is built in two phases per cell row: `lanes` lanes write the column sums of its k pixel rows, one pixel column per
// lane and turn, so that consecutive lanes read consecutive bytes of a frame row; then four lanes per cell add k column sums each.
// The kernels run the phases with the 256 lanes of a workgroup and a barrier between them; a host program runs the lanes one after
// the other.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRACK_MOTION_HD __device__ __forceinline__
#else
#define TRACK_MOTION_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define TRACK_MOTION_C 32               // the chip's side in cells
#define TRACK_MOTION_MAX_S 16           // the search reach in cells
#define TRACK_MOTION_MAX_K 64           // the cell's side in pixels
#define TRACK_MOTION_MAX_POS 1048576.0f // 2^20: the clamp of the centre (the upright tracker's rule)
#define TRACK_MOTION_PARTS 4            // lanes per cell in the second phase

// one gray image: its first byte, pixels, rows, bytes per row
struct TrackMotionImage {
    const uint8_t* p;
    int w, h, stride;
};

struct TrackMotionGrid {
    int k, ox, oy;
};

// cells of a search window's side, and the bytes of one of its rows in memory: nine aligned words from any start column stay inside
TRACK_MOTION_HD int track_motion_window(int S) { return TRACK_MOTION_C + 2 * S; }
TRACK_MOTION_HD int track_motion_pitch(int S) { return ((track_motion_window(S) + 3) & ~3) + 4; }

// the grid of a row whose enclosing box is [x0, x1] x [y0, y1]
TRACK_MOTION_HD TrackMotionGrid track_motion_grid(float x0, float x1, float y0, float y1, float scale)
{
    const float side = fmaxf(x1 - x0, y1 - y0) * scale;
    const float q = ceilf(side / 32.0f);
    TrackMotionGrid g;
    g.k = q >= (float)TRACK_MOTION_MAX_K ? TRACK_MOTION_MAX_K : (q >= 1.0f ? (int)q : 1);      // (a NaN gives 1)
    const float cx = fminf(fmaxf((x0 + x1) * 0.5f, -TRACK_MOTION_MAX_POS), TRACK_MOTION_MAX_POS);
    const float cy = fminf(fmaxf((y0 + y1) * 0.5f, -TRACK_MOTION_MAX_POS), TRACK_MOTION_MAX_POS);
    g.ox = (int)floorf(cx) - 16 * g.k;
    g.oy = (int)floorf(cy) - 16 * g.k;
    return g;
}

// first phase, a lane's share: colsum[x] = the sum of the k taps (X0 + x, Y0 .. Y0 + k - 1) for x = lane, lane + lanes, ... < npx.
// Every tap is guarded by the image's own width and height; a tap outside reads 0.
TRACK_MOTION_HD void track_motion_columns(const TrackMotionImage& im, int X0, int Y0, int k, int npx, int lane, int lanes, int* colsum)
{
    for (int x = lane; x < npx; x += lanes) {
        const int X = X0 + x;
        int sum = 0;
        if (X >= 0 && X < im.w)
            for (int v = 0; v < k; ++v) {
                const int Y = Y0 + v;
                if (Y >= 0 && Y < im.h) sum += im.p[(long long)Y * im.stride + X];
            }
        colsum[x] = sum;
    }
}

// second phase: part q of cell c, the column sums c k + q, c k + q + 4, ...; the four parts added are the cell's block sum
TRACK_MOTION_HD int track_motion_cell_part(const int* colsum, int c, int q, int k)
{
    int sum = 0;
    for (int u = q; u < k; u += TRACK_MOTION_PARTS) sum += colsum[c * k + u];
    return sum;
}

// the cell's byte: the rounded mean of its k x k taps
TRACK_MOTION_HD uint8_t track_motion_mean(int block_sum, int k)
{
    const int kk = k * k;
    return (uint8_t)((block_sum + kk / 2) / kk);
}

// |a - b| of four bytes each, added to acc
TRACK_MOTION_HD uint32_t track_motion_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int e = 0; e < 4; ++e) {
        const int d = (int)((a >> (8 * e)) & 255u) - (int)((b >> (8 * e)) & 255u);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

// bytes sh .. sh + 3 of the eight bytes lo, hi (sh in 0 .. 3)
TRACK_MOTION_HD uint32_t track_motion_align(uint32_t hi, uint32_t lo, int sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#else
    return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
#endif
}

// SAD(dx, dy) of the reference chip (32 rows of 8 words) against the window cur (words, track_motion_pitch(S) bytes per row)
TRACK_MOTION_HD int track_motion_sad(const uint32_t* cur, const uint32_t* ref, int S, int dx, int dy)
{
    const int pw = track_motion_pitch(S) / 4;
    const int c0 = S + dx, w0 = c0 >> 2, sh = c0 & 3;
    uint32_t acc = 0;
#if defined(__HIPCC__)
#pragma unroll 2                        // (unrolled whole, the 256 words of the chip are kept in registers: one wave per SIMD)
#endif
    for (int j = 0; j < TRACK_MOTION_C; ++j) {
        const uint32_t* row = cur + (S + dy + j) * pw + w0;
        const uint32_t* rr = ref + j * (TRACK_MOTION_C / 4);
        uint32_t lo = row[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int m = 0; m < TRACK_MOTION_C / 4; ++m) {
            const uint32_t hi = row[m + 1];
            acc = track_motion_sad4(track_motion_align(hi, lo, sh), rr[m], acc);
            lo = hi;
        }
    }
    return (int)acc;
}

// the search key: the lexicographic order of (SAD, dx^2 + dy^2, dy, dx) as the order of one integer -- SAD < 2^18, the squared
// distance <= 512, dy + 16 and dx + 16 in 0 .. 32
TRACK_MOTION_HD unsigned long long track_motion_key(int sad, int dx, int dy)
{
    return ((unsigned long long)(unsigned)sad << 22) | ((unsigned long long)(unsigned)(dx * dx + dy * dy) << 12) |
           ((unsigned long long)(unsigned)(dy + TRACK_MOTION_MAX_S) << 6) | (unsigned long long)(unsigned)(dx + TRACK_MOTION_MAX_S);
}
TRACK_MOTION_HD int track_motion_key_sad(unsigned long long key) { return (int)(key >> 22); }
TRACK_MOTION_HD int track_motion_key_dx(unsigned long long key) { return (int)(key & 63u) - TRACK_MOTION_MAX_S; }
TRACK_MOTION_HD int track_motion_key_dy(unsigned long long key) { return (int)((key >> 6) & 63u) - TRACK_MOTION_MAX_S; }

// a lane's share of the search: the smallest key of the offsets o = lane, lane + lanes, ... < (2S + 1)^2, o = (dy + S)(2S + 1) + dx + S;
// the lane that holds the offset (0, 0) leaves its SAD in *sad_zero
TRACK_MOTION_HD unsigned long long track_motion_search(const uint32_t* cur, const uint32_t* ref, int S, int lane, int lanes, int* sad_zero)
{
    const int n = 2 * S + 1;
    unsigned long long best = ~0ull;
    for (int o = lane; o < n * n; o += lanes) {
        const int dy = o / n - S, dx = o - (dy + S) * n - S;
        const int sad = track_motion_sad(cur, ref, S, dx, dy);
        if (dx == 0 && dy == 0) *sad_zero = sad;
        const unsigned long long key = track_motion_key(sad, dx, dy);
        best = key < best ? key : best;
    }
    return best;
}

// the acceptance rule: the best offset is taken when it beats staying in place by min_gain / 256 of the latter's SAD
TRACK_MOTION_HD bool track_motion_accept(int sad_best, int sad_zero, int min_gain) { return sad_best * 256 <= sad_zero * (256 - min_gain); }
