// sdm_align_paste_device.h -- the arithmetic of the paste-back of crop tensors into frames (include/sdm.h, "Pasting crops back"): a row's
// inverse map, flags and box (paste_prepare_row), the footprint test, the decoded taps, the integer bilinear colour and opacity
// (paste_sample), the blend, the pixel's load / apply / store, and paste_pixel -- what one frame pixel's owner does from the ownership
// test to its one store.  The quantisation, the weights, the gray rule and the element formula are sdm_align_tensor_device.h's.  Plain
// C++ behind one macro, so the same text is the device code of csrc/sdm_align_paste.hip and -- compiled for the host,
// tests/cpp/align_paste_host.cpp -- a program that runs under the host sanitizers on frames, tensors and opacity maps of exactly the
// bytes they own.
//
// Every float operation is rounded on its own (no contraction: the pragma below under clang, -ffp-contract=off elsewhere); everything
// else is int32 / uint32 arithmetic, every offset 64-bit.
#pragma once
#include "sdm_align_tensor_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// one destination frame and its rows: entries row_begin ... row_end - 1 of the row list, ascending
struct PasteFrameDev {
    uint8_t* p;
    long long stride;
    int w, h, format;           // SDM_FRAME_GRAY ... SDM_FRAME_RGBA
    int row_begin, row_end;
    int pad;
};

// one row, as the prepare stage leaves it
struct PasteRow {
    float w[6];                 // frame -> crop: W00 W01 W02 W10 W11 W12
    int flags;                  // SDM_ALIGN_*
    int frame;
    int x0, y0, x1, y1;         // the footprint's box in the frame, [x0, x1) x [y0, y1); empty for a row that pastes nothing
};

// the decode and gray constants (AlignTensorDev's of csrc/sdm_kernels.h, which host code cannot include)
struct PasteTensorDev {
    float scale[3], bias[3];    // per TENSOR channel
    int order;                  // SDM_ALIGN_ORDER_*
    int wb, wg, wr, gray_shift;
};

// the tensor and the opacity maps of a call
struct PasteCropDev {
    const void* in;             // the tensor
    const uint8_t* alpha;       // null: 255 inside the crop
    long long sn;               // elements from row n to row n + 1
    int sc, sy, sx;             // elements from channel to channel, crop row to crop row, column to column
    long long an;               // bytes from row n's opacity map to row n + 1's (0: one map for all rows)
    int cw, ch;                 // the crop
    int dtype, channels;        // SDM_ALIGN_U8 | F16 | F32; 1 | 3
    PasteTensorDev t;
};

// W (frame -> crop) of a float32 M (crop -> frame): in double, each of the six entries rounded once to float32; returns d
ALIGN_HD double paste_inverse(const float m[6], float w[6])
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const double d = m00 * m11 - m01 * m10;
    const double w00 = m11 / d, w01 = -m01 / d, w10 = -m10 / d, w11 = m00 / d;
    const double w02 = -(w00 * m02 + w01 * m12), w12 = -(w10 * m02 + w11 * m12);
    w[0] = (float)w00; w[1] = (float)w01; w[2] = (float)w02;
    w[3] = (float)w10; w[4] = (float)w11; w[5] = (float)w12;
    return d;
}

// M00 M01 M02 M10 M11 M12 (float32, crop -> frame) of a row in a frame of fw x fh pixels: W, the flags and the box.  flags_in: the
// fit's flags, or -1 -- then PARTIAL is the fit's rule evaluated here, on the corner pixel centres of the crop.
ALIGN_HD void paste_prepare_row(const float m[6], int flags_in, int frame, int fw, int fh, int cw, int ch, PasteRow& r)
{
    r.frame = frame;
    r.x0 = r.y0 = r.x1 = r.y1 = 0;
    bool finite = true;
    for (int e = 0; e < 6; ++e) finite = finite && isfinite(m[e]);
    int flags = flags_in < 0 ? 0 : flags_in;
    if (flags_in < 0 && finite) {
        const float cj[2] = {0.0f, (float)(cw - 1)}, ci[2] = {0.0f, (float)(ch - 1)};
        for (int u = 0; u < 2; ++u)
            for (int v = 0; v < 2; ++v) {
                const float sx = (m[0] * cj[u] + m[1] * ci[v]) + m[2];
                const float sy = (m[3] * cj[u] + m[4] * ci[v]) + m[5];
                if (!(sx >= 0.0f && sx <= (float)(fw - 1) && sy >= 0.0f && sy <= (float)(fh - 1))) flags = SDM_ALIGN_PARTIAL;
            }
    }
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const double d = paste_inverse(m, r.w);
    bool ok = finite && !(flags & SDM_ALIGN_DEGENERATE) && d != 0.0;
    for (int e = 0; e < 6; ++e) ok = ok && isfinite(r.w[e]);
    if (!ok) {
        r.flags = finite ? flags | SDM_ALIGN_DEGENERATE : SDM_ALIGN_DEGENERATE;       // (as the fit: no other bit beside a non-finite M)
        return;
    }
    r.flags = flags;
    // the box: the crop corners (-1, -1) ... (cw, ch) through M, widened by what the float32 W and positions can move a footprint
    // pixel against the exact inverse.  A position has three rounded products and sums of magnitude <= |W..| fw + |W..| fh + |W.2|,
    // each W entry is rounded once: 2^-21 of that magnitude bounds the error in crop pixels, 1/32 more covers the quantisation; a
    // crop pixel is |M00| + |M01| (|M10| + |M11|) frame pixels wide (high); one frame pixel more for the floor and the ceiling.
    const double eu = (fabs((double)r.w[0]) * fw + fabs((double)r.w[1]) * fh + fabs((double)r.w[2]) + 1.0) * (1.0 / 2097152.0) + 0.03125;
    const double ev = (fabs((double)r.w[3]) * fw + fabs((double)r.w[4]) * fh + fabs((double)r.w[5]) + 1.0) * (1.0 / 2097152.0) + 0.03125;
    const double e = eu > ev ? eu : ev;
    const double mx = (fabs(m00) + fabs(m01)) * e + 1.0, my = (fabs(m10) + fabs(m11)) * e + 1.0;
    double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double u = (k & 1) ? (double)cw : -1.0, v = (k & 2) ? (double)ch : -1.0;
        const double x = (m00 * u + m01 * v) + m02, y = (m10 * u + m11 * v) + m12;
        if (k == 0 || x < xlo) xlo = x;
        if (k == 0 || x > xhi) xhi = x;
        if (k == 0 || y < ylo) ylo = y;
        if (k == 0 || y > yhi) yhi = y;
    }
    xlo = floor(xlo - mx); xhi = ceil(xhi + mx) + 1.0; ylo = floor(ylo - my); yhi = ceil(yhi + my) + 1.0;
    // clipped to the frame while still double: nothing beyond int reaches the conversion
    r.x0 = xlo > 0.0 ? (xlo < (double)fw ? (int)xlo : fw) : 0;
    r.y0 = ylo > 0.0 ? (ylo < (double)fh ? (int)ylo : fh) : 0;
    r.x1 = xhi < (double)fw ? (xhi > 0.0 ? (int)xhi : 0) : fw;
    r.y1 = yhi < (double)fh ? (yhi > 0.0 ? (int)yhi : 0) : fh;
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r.x0 = r.y0 = r.x1 = r.y1 = 0;
}

// frame pixel (X, Y) in the footprint of r: inside its box, the position accepted by the 2^20 rule, and at least one tap in the crop
ALIGN_HD bool paste_footprint(const PasteRow& r, int cw, int ch, int X, int Y, AlignPos& q)
{
    if (X < r.x0 || X >= r.x1 || Y < r.y0 || Y >= r.y1) return false;
    const float fx = (float)X, fy = (float)Y;
    const float u = (r.w[0] * fx + r.w[1] * fy) + r.w[2];
    const float v = (r.w[3] * fx + r.w[4] * fy) + r.w[5];
    if (!align_quantise(u, v, q)) return false;
    return q.x0 >= -1 && q.x0 <= cw - 1 && q.y0 >= -1 && q.y0 <= ch - 1;
}

ALIGN_HD float paste_half(uint16_t h)
{
#if defined(__HIPCC__) || defined(__FLT16_MAX__)
    _Float16 f;
    memcpy(&f, &h, 2);
    return (float)f;
#else
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t b;
    if (e == 31u) b = s | 0x7f800000u | (m << 13);
    else if (e != 0u) b = s | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) b = s;
    else {
        int k = 0;
        uint32_t mm = m;
        while (!(mm & 1024u)) { mm <<= 1; ++k; }
        b = s | ((uint32_t)(113 - k) << 23) | ((mm & 1023u) << 13);
    }
    float f;
    memcpy(&f, &b, 4);
    return f;
#endif
}

// tensor element e of channel c decoded to 0 ... 255: the byte; or e * scale[c] + bias[c], 0 for a NaN, clamped, rounded to even
ALIGN_HD uint32_t paste_decode(const PasteCropDev& c, long long e, int ch)
{
    if (c.dtype == SDM_ALIGN_U8) return ((const uint8_t*)c.in)[e];
    float x;
    if (c.dtype == SDM_ALIGN_F32) memcpy(&x, (const uint8_t*)c.in + 4 * e, 4);
    else { uint16_t h; memcpy(&h, (const uint8_t*)c.in + 2 * e, 2); x = paste_half(h); }
    const float s = x * c.t.scale[ch];                              // align_element's convention: the product rounded, then the sum
    const float f = s + c.t.bias[ch];
    if (f != f) return 0u;
    return (uint32_t)rintf(fminf(fmaxf(f, 0.0f), 255.0f));
}

// the sampled (B, G, R) and opacity of row n's crop at the quantised position q (inside the footprint).  LABELLED (the piecewise-affine
// paste, csrc/sdm_warp_paste_device.h): a tap whose crop pixel has label 255 in `labels` (crop_height x crop_width bytes) reads opacity 0
template <bool LABELLED>
ALIGN_HD void paste_sample_taps(const PasteCropDev& c, int n, const AlignPos& q, const uint8_t* labels, uint32_t bgr[3], uint32_t& a)
{
    const uint32_t wt[4] = {(uint32_t)((32 - q.fx) * (32 - q.fy)), (uint32_t)(q.fx * (32 - q.fy)), (uint32_t)((32 - q.fx) * q.fy),
                            (uint32_t)(q.fx * q.fy)};
    uint32_t sum[3] = {0u, 0u, 0u}, asum = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = q.x0 + (k & 1), y = q.y0 + (k >> 1);
        const bool in = x >= 0 && x < c.cw && y >= 0 && y < c.ch;
        const int xc = x < 0 ? 0 : (x > c.cw - 1 ? c.cw - 1 : x), yc = y < 0 ? 0 : (y > c.ch - 1 ? c.ch - 1 : y);
        if (in && (!LABELLED || labels[(long long)yc * c.cw + xc] != 255u))
            asum += wt[k] * (c.alpha ? (uint32_t)c.alpha[(long long)n * c.an + (long long)yc * c.cw + xc] : 255u);
        const long long e = (long long)n * c.sn + (long long)yc * c.sy + (long long)xc * c.sx;
        if (c.channels == 3) {
#pragma unroll
            for (int t = 0; t < 3; ++t) sum[t] += wt[k] * paste_decode(c, e + (long long)t * c.sc, t);
        } else {
            sum[0] += wt[k] * paste_decode(c, e, 0);
        }
    }
    a = (asum + 512u) >> 10;
    if (c.channels == 3) {
        const bool rgb = c.t.order == SDM_ALIGN_ORDER_RGB;
        const uint32_t t0 = (sum[0] + 512u) >> 10, t1 = (sum[1] + 512u) >> 10, t2 = (sum[2] + 512u) >> 10;
        bgr[0] = rgb ? t2 : t0; bgr[1] = t1; bgr[2] = rgb ? t0 : t2;
    } else {
        bgr[0] = bgr[1] = bgr[2] = (sum[0] + 512u) >> 10;
    }
}

ALIGN_HD void paste_sample(const PasteCropDev& c, int n, const AlignPos& q, uint32_t bgr[3], uint32_t& a)
{
    paste_sample_taps<false>(c, n, q, nullptr, bgr, a);
}

ALIGN_HD uint32_t paste_blend(uint32_t a, uint32_t q, uint32_t o) { return (a * q + (255u - a) * o + 127u) / 255u; }

// One frame pixel in its owner's registers: the old colour bytes loaded once (paste_load), every row's sample blended in (paste_apply),
// the colour bytes stored once, byte by byte, if any opacity was not 0 (paste_store).  Shared by both pastes.
struct PastePixel {
    uint8_t* p;
    uint32_t o[3];
    int nb;                     // colour bytes: 1 | 3 (the alpha byte is neither read nor written)
    bool swap, any;
};

ALIGN_HD void paste_load(const PasteFrameDev& f, int X, int Y, PastePixel& s)
{
    const int bpp = f.format == SDM_FRAME_GRAY ? 1 : (f.format == SDM_FRAME_BGR || f.format == SDM_FRAME_RGB) ? 3 : 4;
    s.nb = bpp == 1 ? 1 : 3;
    s.p = f.p + ((long long)Y * f.stride + (long long)X * bpp);
    s.o[0] = s.o[1] = s.o[2] = 0u;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < s.nb) s.o[b] = s.p[b];
    s.swap = f.format == SDM_FRAME_RGB || f.format == SDM_FRAME_RGBA;
    s.any = false;
}

ALIGN_HD void paste_apply(const PasteCropDev& c, const uint32_t bgr[3], uint32_t a, PastePixel& s)
{
    if (a == 0u) return;
    s.any = true;
    if (s.nb == 1) {
        const uint32_t g = c.channels == 3 ? (bgr[0] * c.t.wb + bgr[1] * c.t.wg + bgr[2] * c.t.wr + (1u << (c.t.gray_shift - 1))) >> c.t.gray_shift
                                           : bgr[0];
        s.o[0] = paste_blend(a, g, s.o[0]);
    } else {
#pragma unroll
        for (int b = 0; b < 3; ++b) s.o[b] = paste_blend(a, bgr[s.swap ? 2 - b : b], s.o[b]);
    }
}

ALIGN_HD void paste_store(const PastePixel& s)
{
    if (!s.any) return;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < s.nb) s.p[b] = (uint8_t)s.o[b];
}

// Frame pixel (X, Y) as seen by entry k of its frame's row list: nothing unless the pixel is in that row's footprint and in no earlier
// entry's -- then this is the pixel's one reader and writer: the old bytes once, every later entry of the list that holds the pixel
// applied in order, the colour bytes stored once if any opacity was not 0.  rows: all rows' records; list: the row lists.
ALIGN_HD void paste_pixel(const PasteFrameDev& f, const PasteRow* rows, const int* list, int k, const PasteCropDev& c, int X, int Y)
{
    AlignPos q;
    if (!paste_footprint(rows[list[k]], c.cw, c.ch, X, Y, q)) return;
    for (int j = f.row_begin; j < k; ++j) {
        AlignPos qj;
        if (paste_footprint(rows[list[j]], c.cw, c.ch, X, Y, qj)) return;
    }
    PastePixel s;
    paste_load(f, X, Y, s);
    for (int j = k; j < f.row_end; ++j) {
        const int n = list[j];
        if (j > k && !paste_footprint(rows[n], c.cw, c.ch, X, Y, q)) continue;
        uint32_t bgr[3], a;
        paste_sample(c, n, q, bgr, a);
        paste_apply(c, bgr, a, s);
    }
    paste_store(s);
}
