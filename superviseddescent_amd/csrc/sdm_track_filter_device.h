// sdm_track_filter_device.h -- the arithmetic of the tracker's temporal landmark filter (include/sdm.h, "Tracking, filtered"): the
// One-Euro filter of Casiez et al. 2012, a first-order low-pass whose cut-off rises with the filtered speed, the speed measured in
// units of the face's own size.  Per slot three rows of 2L floats -- r the previous raw row, d the filtered derivative, f the
// previous filtered row -- and one int, primed.
// Plain C++ behind TRACK_FILTER_HD: the device code of track_filter_kernel (csrc/sdm_track_filter.hip) and, compiled for the host,
// of tests/cpp/track_filter_host.cpp, which runs it under the host sanitizers on state rows of exactly 2L floats.
//
// A row is worked on by `stride` lanes; lane k holds the coordinates k, k + stride, ...  The kernel runs it with the 64 lanes of a
// wave and reduces the lanes' bounds with __shfl_xor; a host program runs the lanes one after the other.
//
// float32 throughout; every operation is rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off
// elsewhere).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TRACK_FILTER_HD __device__ __forceinline__
#else
#define TRACK_FILTER_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

struct TrackFilterParams {
    float min_cutoff, beta, d_cutoff;      // Hz, Hz per face size per second, Hz
};

// what a row does in this step
#define TRACK_FILTER_PASS 0                // lost: out = x, the slot's state is dropped
#define TRACK_FILTER_PRIME 1               // first filtered step since start / restart / configure: r = x, d = 0, f = x, out = x
#define TRACK_FILTER_RUN 2

TRACK_FILTER_HD int track_filter_action(int mask, int primed)
{
    return mask != 0 ? TRACK_FILTER_PASS : (primed ? TRACK_FILTER_RUN : TRACK_FILTER_PRIME);
}

// the smoothing factor of a cut-off fc (Hz) at a step of dt seconds
TRACK_FILTER_HD float track_filter_alpha(float fc, float dt)
{
    return 1.0f / (1.0f + (1.0f / (6.2831855f * fc)) / dt);
}

// a lane's share of the row's enclosing box: min / max of its x and of its y coordinates (+-INFINITY where it holds none)
TRACK_FILTER_HD void track_filter_bounds(const float* x, int L, int lane, int stride, float& x0, float& x1, float& y0, float& y1)
{
    x0 = INFINITY; x1 = -INFINITY; y0 = INFINITY; y1 = -INFINITY;
    for (int j = lane; j < L; j += stride) {
        const float vx = x[j], vy = x[L + j];
        x0 = fminf(x0, vx); x1 = fmaxf(x1, vx);
        y0 = fminf(y0, vy); y1 = fmaxf(y1, vy);
    }
}

// the speed weight of a row whose enclosing box is [x0, x1] x [y0, y1]: beta per face size s, 0 for a face without size
TRACK_FILTER_HD float track_filter_weight(float beta, float x0, float x1, float y0, float y1)
{
    const float s = fmaxf(x1 - x0, y1 - y0);
    return s > 0.0f ? beta / s : 0.0f;
}

// one coordinate of a primed row: the state moves on, the filtered value is returned
TRACK_FILTER_HD float track_filter_coordinate(float x, float dt, float ad, float min_cutoff, float w, float& r, float& d, float& f)
{
    const float v = (x - r) / dt;
    float dn = (ad * v) + ((1.0f - ad) * d);
    if (!isfinite(dn)) dn = 0.0f;
    const float a = track_filter_alpha(min_cutoff + w * fabsf(dn), dt);
    float fn = (a * x) + ((1.0f - a) * f);
    if (!isfinite(fn)) fn = x;
    r = x; d = dn; f = fn;
    return fn;
}

// a lane's share of one row: x (2L, raw in, filtered out), the slot's r, d, f (2L each); w from the whole row's bounds
TRACK_FILTER_HD void track_filter_row(float* x, float* r, float* d, float* f, int M, int lane, int stride, int action, float dt, float w,
                                      const TrackFilterParams& p)
{
    if (action == TRACK_FILTER_PASS) return;
    if (action == TRACK_FILTER_PRIME) {
        for (int j = lane; j < M; j += stride) {
            const float v = x[j];
            r[j] = v; d[j] = 0.0f; f[j] = v;
        }
        return;
    }
    const float ad = track_filter_alpha(p.d_cutoff, dt);
    for (int j = lane; j < M; j += stride) {
        float rj = r[j], dj = d[j], fj = f[j];
        x[j] = track_filter_coordinate(x[j], dt, ad, p.min_cutoff, w, rj, dj, fj);
        r[j] = rj; d[j] = dj; f[j] = fj;
    }
}
