// sdm_align_paste_area_device.h -- what the filtered paste (include/sdm.h, "Pasting crops back, filtered") adds to
// csrc/sdm_align_paste_device.h: S of a row from its W and the row's working footprint (paste_area_prepare_row), the footprint test
// (paste_area_holds), the pixel of a row with S > 1 -- the average of S x S sub-samples' unrounded sums (paste_area_taps) -- and the
// shape for the ownership rule (PasteRigidArea).  S, the offsets and the average are csrc/sdm_align_area_device.h's, the taps, the
// blend and the ownership rule csrc/sdm_paste_device.h's.  Plain C++ behind ALIGN_HD: the device code of csrc/sdm_align_paste.hip and,
// compiled for the host, tests/cpp/align_paste_area_host.cpp.  No float contraction.
#pragma once
#include "sdm_align_area_device.h"
#include "sdm_align_paste_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// what the prepare stage keeps beside a row's PasteRow
struct PasteAreaRow {
    int S;                      // sub-samples per axis, 1 ... 16
    float du, dv;               // S > 1: how far the pixel CENTRE's position may lie outside [-1, cw] x [-1, ch]; < 0: the box alone decides
    int pad;
};

// paste_prepare_row, then S from the float32 W (align_area_samples on W00, W10) and, for S > 1, the working footprint: the box one
// frame pixel wider on each side (an empty box stays empty: its own margin of a whole pixel already holds the offsets' half), and the
// reach du, dv.  A sub-sample lies less than half a frame pixel from the centre, (|W00| + |W01|) / 2 crop pixels in u; both positions are
// float32 sums of magnitude <= mag = |W00| (fw + 1) + |W01| (fh + 1) + |W02|, four roundings each: 2^-21 mag bounds either's error.  A
// sub-sample has a tap in the crop only from -1 - 1/64 up to cw, and 1/4 more covers the roundings of the test itself.  Beyond
// mag = 2^20 or a reach of 2^15 no bound is claimed, and the box alone decides.
ALIGN_HD void paste_area_prepare_row(const float m[6], int flags_in, int frame, int fw, int fh, int cw, int ch, int mode, int max_samples,
                                     float min2, PasteRow& r, PasteAreaRow& ar)
{
    paste_prepare_row(m, flags_in, frame, fw, fh, cw, ch, r);
    ar.S = align_area_samples(r.w, r.flags, mode, max_samples, min2);
    ar.du = ar.dv = -1.0f;
    ar.pad = 0;
    if (ar.S == 1 || r.x1 <= r.x0) return;
    r.x0 = r.x0 > 0 ? r.x0 - 1 : 0; r.y0 = r.y0 > 0 ? r.y0 - 1 : 0;
    r.x1 = r.x1 < fw ? r.x1 + 1 : fw; r.y1 = r.y1 < fh ? r.y1 + 1 : fh;
    const double mu = fabs((double)r.w[0]) * (fw + 1.0) + fabs((double)r.w[1]) * (fh + 1.0) + fabs((double)r.w[2]);
    const double mv = fabs((double)r.w[3]) * (fw + 1.0) + fabs((double)r.w[4]) * (fh + 1.0) + fabs((double)r.w[5]);
    const double du = (fabs((double)r.w[0]) + fabs((double)r.w[1])) * 0.5 + mu * (2.0 / 2097152.0) + 0.28125;
    const double dv = (fabs((double)r.w[3]) + fabs((double)r.w[4])) * 0.5 + mv * (2.0 / 2097152.0) + 0.28125;
    if (!(mu < 1048576.0 && mv < 1048576.0 && du < 32768.0 && dv < 32768.0)) return;
    ar.du = (float)du; ar.dv = (float)dv;
}

// The working footprint: S == 1 -- paste_footprint, at q; S > 1 -- the pixel lies in the row's box and its centre's float32 position
// within (du, dv) of the crop and its one-pixel rim.  It holds every pixel for which the contract's formula gives a != 0; it is the one
// predicate behind "an earlier row owns this pixel" and "this row is applied here".
ALIGN_HD bool paste_area_holds(const PasteRow& r, const PasteAreaRow& ar, int cw, int ch, int X, int Y, AlignPos& q)
{
    if (ar.S == 1) return paste_footprint(r, cw, ch, X, Y, q);
    q.x0 = q.fx = q.y0 = q.fy = 0;
    if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) return false;
    if (ar.du < 0.0f) return true;
    const float fx = (float)X, fy = (float)Y;
    const float u = (r.w[0] * fx + r.w[1] * fy) + r.w[2];
    const float v = (r.w[3] * fx + r.w[4] * fy) + r.w[5];
    return u >= -1.0f - ar.du && u <= (float)cw + ar.du && v >= -1.0f - ar.dv && v <= (float)ch + ar.dv;
}

// the four weighted taps of row n's crop at the quantised position q ADDED to the unrounded sums: per tensor channel, the taps clamped
// into the crop, and the opacity, a tap outside the crop reading 0.  (paste_sample_taps's loop without its rounding; that function
// written on top of this one computes the same and moves the registers of both unfiltered paste kernels, which stay as they are.)
ALIGN_HD void paste_area_tap_sums(const PasteCropDev& c, int n, const AlignPos& q, uint32_t sum[3], uint32_t& asum)
{
    const uint32_t wt[4] = {(uint32_t)((32 - q.fx) * (32 - q.fy)), (uint32_t)(q.fx * (32 - q.fy)), (uint32_t)((32 - q.fx) * q.fy),
                            (uint32_t)(q.fx * q.fy)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = q.x0 + (k & 1), y = q.y0 + (k >> 1);
        const bool in = x >= 0 && x < c.cw && y >= 0 && y < c.ch;
        const int xc = x < 0 ? 0 : (x > c.cw - 1 ? c.cw - 1 : x), yc = y < 0 ? 0 : (y > c.ch - 1 ? c.ch - 1 : y);
        if (in) asum += wt[k] * (c.alpha ? (uint32_t)c.alpha[(long long)n * c.an + (long long)yc * c.cw + xc] : 255u);
        const long long e = (long long)n * c.sn + (long long)yc * c.sy + (long long)xc * c.sx;
        if (c.channels == 3) {
#pragma unroll
            for (int t = 0; t < 3; ++t) sum[t] += wt[k] * paste_decode(c, e + (long long)t * c.sc, t);
        } else {
            sum[0] += wt[k] * paste_decode(c, e, 0);
        }
    }
}

// frame pixel (X, Y) under row n with S > 1: the S x S sub-samples' unrounded colour and opacity sums, averaged; then the channel order
// as at S == 1.  a = 0 when a sub-sample is refused by the 2^20 rule: the row does not touch the pixel.
ALIGN_HD void paste_area_taps(const PasteCropDev& c, int n, const PasteRow& r, int S, int X, int Y, uint32_t bgr[3], uint32_t& a)
{
    const float* o = align_area_offsets.o + S * (S - 1) / 2;
    uint32_t sum[3] = {0u, 0u, 0u}, asum = 0u;
    bool ok = true;
    for (int v = 0; v < S; ++v) {
        const float fy = (float)Y + o[v];
        const float ax = r.w[1] * fy, ay = r.w[4] * fy;
        for (int u = 0; u < S; ++u) {
            const float fx = (float)X + o[u];
            const float pu = (r.w[0] * fx + ax) + r.w[2];
            const float pv = (r.w[3] * fx + ay) + r.w[5];
            AlignPos q;
            if (!align_quantise(pu, pv, q)) { ok = false; continue; }
            paste_area_tap_sums(c, n, q, sum, asum);
        }
    }
    a = 0u;
    bgr[0] = bgr[1] = bgr[2] = 0u;
    if (!ok) return;
    const uint32_t k = (uint32_t)(S * S), rcp = align_area_reciprocal(k);
    a = align_area_average(asum, k, rcp);
    if (c.channels == 3) {
        const bool rgb = c.t.order == SDM_ALIGN_ORDER_RGB;
        const uint32_t t0 = align_area_average(sum[0], k, rcp), t1 = align_area_average(sum[1], k, rcp), t2 = align_area_average(sum[2], k, rcp);
        bgr[0] = rgb ? t2 : t0; bgr[1] = t1; bgr[2] = rgb ? t0 : t2;
    } else {
        bgr[0] = bgr[1] = bgr[2] = align_area_average(sum[0], k, rcp);
    }
}

// the filtered paste's shape for paste_owned: all rows' records and what the prepare stage kept beside them
struct PasteRigidArea {
    const PasteRow* rows;
    const PasteAreaRow* area;
};

ALIGN_HD bool paste_holds(const PasteRigidArea& p, int n, const PasteCropDev& c, int X, int Y, AlignPos& q)
{
    return paste_area_holds(p.rows[n], p.area[n], c.cw, c.ch, X, Y, q);
}

ALIGN_HD void paste_taps(const PasteRigidArea& p, const PasteCropDev& c, int n, int X, int Y, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    const int S = p.area[n].S;
    if (S == 1) paste_sample_taps<false>(c, n, q, nullptr, bgr, a);
    else paste_area_taps(c, n, p.rows[n], S, X, Y, bgr, a);
}

// paste_pixel of the filtered paste
template <bool PLANAR = true>
ALIGN_HD void paste_area_pixel(const PasteFrameDev& f, const PasteRow* rows, const PasteAreaRow* area, const int* list, int k,
                               const PasteCropDev& c, int X, int Y)
{
    AlignPos q;
    const int n = list[k];
    if (paste_area_holds(rows[n], area[n], c.cw, c.ch, X, Y, q)) paste_owned<PLANAR>(f, PasteRigidArea{rows, area}, list, k, c, X, Y, q);
}
