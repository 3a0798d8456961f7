// sdm_paste_device.h -- what the two pastes of tensors back into frames share (include/sdm.h, "Pasting crops back" and "Pasting warped
// faces back"): the frame and crop records, the inverse map, a frame pixel's position in the crop (paste_position), the decoded taps,
// the integer bilinear colour and opacity, the blend, the pixel's load / apply / store, and paste_owned -- the one text of the ownership
// rule, which a paste calls with its shape (PasteRigid of csrc/sdm_align_paste_device.h, PasteRigidArea of
// csrc/sdm_align_paste_area_device.h, PasteMesh of csrc/sdm_warp_paste_device.h).
// Plain C++ behind ALIGN_HD: the device code of both kernels and, compiled for the host, of the two programs of tests/cpp that run it
// under the host sanitizers on frames, tensors and opacity maps of exactly the bytes they own.
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

// the tensor and the opacity maps of a call
struct PasteCropDev {
    const void* in;             // the tensor
    const uint8_t* alpha;       // null: 255 inside the crop
    long long sn;               // elements from row n to row n + 1
    int sc, sy, sx;             // elements from channel to channel, crop row to crop row, column to column
    long long an;               // bytes from row n's opacity map to row n + 1's (0: one map for all rows)
    int cw, ch;                 // the crop
    int dtype, channels;        // SDM_ALIGN_U8 | F16 | F32; 1 | 3
    AlignTensorDev t;           // the decode and gray constants
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

// frame pixel (X, Y) through W into a crop of cw x ch pixels: the position accepted by the 2^20 rule, and at least one tap in the crop
ALIGN_HD bool paste_position(const float w[6], int cw, int ch, int X, int Y, AlignPos& q)
{
    const float fx = (float)X, fy = (float)Y;
    const float u = (w[0] * fx + w[1] * fy) + w[2];
    const float v = (w[3] * fx + w[4] * fy) + w[5];
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
// paste): a tap whose crop pixel has label 255 in `labels` (crop_height x crop_width bytes) reads opacity 0
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

ALIGN_HD uint32_t paste_blend(uint32_t a, uint32_t q, uint32_t o) { return (a * q + (255u - a) * o + 127u) / 255u; }

// One frame pixel in its owner's registers: the old colour bytes loaded once (paste_load), every row's sample blended in (paste_apply),
// the colour bytes stored once, byte by byte, if any opacity was not 0 (paste_store).
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

// The ownership rule.  Frame pixel (X, Y) lies in the footprint of entry k of its frame's row list at position q: nothing if an earlier
// entry's footprint holds it too -- else this is the pixel's one reader and writer: the old bytes once, entry k and every later entry
// that holds the pixel applied in order, the colour bytes stored once if any opacity was not 0.  list: the row lists.  Shape: the paste's
// rows, with paste_holds(shape, n, crop, X, Y, q) -- row n's footprint holds the pixel, at q -- and paste_taps(shape, crop, n, X, Y, q,
// bgr, a): row n's colour and opacity for the pixel (a == 0: the row leaves it alone)
template <class Shape>
ALIGN_HD void paste_owned(const PasteFrameDev& f, const Shape& shape, const int* list, int k, const PasteCropDev& c, int X, int Y, AlignPos q)
{
    for (int j = f.row_begin; j < k; ++j) {
        AlignPos qj;
        if (paste_holds(shape, list[j], c, X, Y, qj)) return;
    }
    PastePixel s;
    paste_load(f, X, Y, s);
    for (int j = k; j < f.row_end; ++j) {
        const int n = list[j];
        if (j > k && !paste_holds(shape, n, c, X, Y, q)) continue;
        uint32_t bgr[3], a;
        paste_taps(shape, c, n, X, Y, q, bgr, a);
        paste_apply(c, bgr, a, s);
    }
    paste_store(s);
}
