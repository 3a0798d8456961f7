// sdm_paste_device.h -- what the two pastes of tensors back into frames share (include/sdm.h, "Pasting crops back" and "Pasting warped
// faces back"): the frame and crop records, the inverse map, a frame pixel's position in the crop (paste_position), the decoded taps,
// the integer bilinear colour and opacity, the blend, the pixel's load / apply / store, and paste_owned -- the one text of the ownership
// rule, which a paste calls with its shape (PasteRigid of csrc/sdm_align_paste_device.h, PasteRigidArea of
// csrc/sdm_align_paste_area_device.h, PasteMesh of csrc/sdm_warp_paste_device.h) -- and, for NV12 destinations ("Pasting crops back
// into NV12 frames"), its sibling paste_owned_block with the 2 x 2 block's load / luma / chroma / store.
// Plain C++ behind ALIGN_HD: the device code of both kernels and, compiled for the host, of the programs of tests/cpp that run it
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
    long long plane;            // planar colour: bytes from plane c to plane c + 1, of any sign (0 otherwise)
    int w, h, format;           // SDM_FRAME_GRAY ... SDM_FRAME_RGBA, SDM_FRAME_NV12 with its matrix and range bits (the block path), SDM_FRAME_*_PLANAR
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

// sn, sc, sy, sx and an of a tensor of cw x ch x channels in `layout` (SDM_ALIGN_NCHW | SDM_ALIGN_NHWC), one opacity map per row or one
// for all.  Host code: the C-ABI fills the record with it, and so do the host programs of tests/cpp.
static inline void paste_crop_layout(PasteCropDev& c, int layout, bool alpha_per_row)
{
    c.sn = (long long)c.channels * c.cw * c.ch;
    if (layout == SDM_ALIGN_NCHW) { c.sc = c.cw * c.ch; c.sy = c.cw; c.sx = 1; }
    else { c.sc = 1; c.sy = c.cw * c.channels; c.sx = c.channels; }
    c.an = alpha_per_row ? (long long)c.cw * c.ch : 0;
}

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
    long long pd;               // planar colour: colour byte b is p[b * pd]; 0: the bytes are p[0 ... nb - 1]
    uint32_t o[3];
    int nb;                     // colour bytes: 1 | 3 (the alpha byte is neither read nor written)
    bool swap, any;
};

// PLANAR false: an instance for frame lists that hold no planar frame -- the planar case is not in its code (the kernels choose at the
// launch; the host programs and every caller that names nothing take the general text)
template <bool PLANAR = true>
ALIGN_HD void paste_load(const PasteFrameDev& f, int X, int Y, PastePixel& s)
{
    const bool planar = PLANAR && align_planar(f.format);
    const int bpp = f.format == SDM_FRAME_GRAY || planar ? 1 : (f.format == SDM_FRAME_BGR || f.format == SDM_FRAME_RGB) ? 3 : 4;
    s.nb = f.format == SDM_FRAME_GRAY ? 1 : 3;
    s.p = f.p + ((long long)Y * f.stride + (long long)X * bpp);
    s.pd = planar ? f.plane : 0;
    s.o[0] = s.o[1] = s.o[2] = 0u;
    if (planar) {                                                   // one byte of each plane
        s.o[0] = s.p[0]; s.o[1] = s.p[s.pd]; s.o[2] = s.p[s.pd + s.pd];
    } else {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b < s.nb) s.o[b] = s.p[b];
    }
    s.swap = align_red_first(f.format);
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

template <bool PLANAR = true>
ALIGN_HD void paste_store(const PastePixel& s)
{
    if (!s.any) return;
    if (PLANAR && s.pd != 0) {
        s.p[0] = (uint8_t)s.o[0]; s.p[s.pd] = (uint8_t)s.o[1]; s.p[s.pd + s.pd] = (uint8_t)s.o[2];
        return;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < s.nb) s.p[b] = (uint8_t)s.o[b];
}

// The ownership rule.  Frame pixel (X, Y) lies in the footprint of entry k of its frame's row list at position q: nothing if an earlier
// entry's footprint holds it too -- else this is the pixel's one reader and writer: the old bytes once, entry k and every later entry
// that holds the pixel applied in order, the colour bytes stored once if any opacity was not 0.  list: the row lists.  Shape: the paste's
// rows, with paste_holds(shape, n, crop, X, Y, q) -- row n's footprint holds the pixel, at q -- and paste_taps(shape, crop, n, X, Y, q,
// bgr, a): row n's colour and opacity for the pixel (a == 0: the row leaves it alone)
template <bool PLANAR = true, class Shape>
ALIGN_HD void paste_owned(const PasteFrameDev& f, const Shape& shape, const int* list, int k, const PasteCropDev& c, int X, int Y, AlignPos q)
{
    for (int j = f.row_begin; j < k; ++j) {
        AlignPos qj;
        if (paste_holds(shape, list[j], c, X, Y, qj)) return;
    }
    PastePixel s;
    paste_load<PLANAR>(f, X, Y, s);
    for (int j = k; j < f.row_end; ++j) {
        const int n = list[j];
        if (j > k && !paste_holds(shape, n, c, X, Y, q)) continue;
        uint32_t bgr[3], a;
        paste_taps(shape, c, n, X, Y, q, bgr, a);
        paste_apply(c, bgr, a, s);
    }
    paste_store<PLANAR>(s);
}

// NV12 destinations (include/sdm.h, "Pasting crops back into NV12 frames").  The unit is the 2 x 2 block of luma pixels that share one
// (U, V) pair: block (BX, BY) holds the pixels X in {2 BX, 2 BX + 1}, Y in {2 BY, 2 BY + 1} that lie inside the frame, pixel i at
// (2 BX + (i & 1), 2 BY + (i >> 1)).  BT.601 limited range in Q20, the counterpart of align_nv12_to_bgr.
ALIGN_HD uint32_t paste_nv12_luma(const uint32_t bgr[3])
{
    return (269484u * bgr[2] + 528482u * bgr[1] + 102760u * bgr[0] + (16u << 20) + (1u << 19)) >> 20;
}

ALIGN_HD void paste_nv12_chroma(const uint32_t m[3], uint32_t& u, uint32_t& v)
{
    const int b = (int)m[0], g = (int)m[1], r = (int)m[2];
    const int uq = (460324 * b - 305135 * g - 155188 * r + (128 << 20) + (1 << 19)) >> 20;
    const int vq = (460324 * r - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20;
    u = (uint32_t)(uq < 0 ? 0 : (uq > 255 ? 255 : uq));
    v = (uint32_t)(vq < 0 ? 0 : (vq > 255 ? 255 : vq));
}

// One block in its owner's registers: the up-to-four luma bytes (packed, pixel i at bits 8 i) and the UV pair loaded once
// (paste_block_load), every row applied (paste_block_luma per pixel, paste_block_chroma per row), the changed bytes stored once
struct PasteBlock {
    uint8_t* y;                 // the luma byte of pixel 0
    uint8_t* uv;                // the (U, V) pair; null: a 1-channel tensor, the UV plane is neither read nor written
    long long stride;
    uint32_t luma, u, v;
    int in;                     // bit i: pixel i lies inside the frame
    int wrote;                  // bit i: a row's opacity was not 0 on pixel i; bit 4: some a_c was not 0
    uint32_t cnt;               // the pixels inside the frame: 4 | 2 | 1
};

ALIGN_HD void paste_block_load(const PasteFrameDev& f, uint8_t* chroma, const PasteCropDev& c, int BX, int BY, PasteBlock& s)
{
    const int X = 2 * BX, Y = 2 * BY;
    s.stride = f.stride;
    s.y = f.p + ((long long)Y * f.stride + X);
    s.in = 1 | (X + 1 < f.w ? 2 : 0) | (Y + 1 < f.h ? 4 : 0) | (X + 1 < f.w && Y + 1 < f.h ? 8 : 0);
    s.cnt = (X + 1 < f.w ? 2u : 1u) * (Y + 1 < f.h ? 2u : 1u);
    s.luma = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (s.in >> i & 1) s.luma |= (uint32_t)s.y[(long long)(i >> 1) * s.stride + (i & 1)] << (8 * i);
    s.uv = c.channels == 3 ? chroma + ((long long)BY * f.stride + 2 * (long long)BX) : nullptr;
    s.u = s.v = 0u;
    if (s.uv) { s.u = s.uv[0]; s.v = s.uv[1]; }
    s.wrote = 0;
}

// a row's colour and opacity (a != 0) on pixel i: the luma blend; the opacity-weighted colour sums of the row's chroma rule.
// YUV false: every NV12 frame of the call is value 5, the constants are in the code as they always were; YUV true: a frame of the call
// carries a colour description ("YUV colour description and 10-bit surfaces"), the constants are enc, the frame's table row (value 5's
// included)
template <bool YUV = false>
ALIGN_HD void paste_block_luma(const PasteCropDev& c, const uint32_t bgr[3], uint32_t a, int i, PasteBlock& s, uint32_t sum[3], uint32_t& A,
                               const YuvEncode* enc = nullptr)
{
    uint32_t yq;
    if constexpr (YUV) yq = c.channels == 3 ? yuv_luma(*enc, bgr) : bgr[0];
    else yq = c.channels == 3 ? paste_nv12_luma(bgr) : bgr[0];
    const uint32_t o = s.luma >> (8 * i) & 255u;
    s.luma = (s.luma & ~(255u << (8 * i))) | paste_blend(a, yq, o) << (8 * i);
    s.wrote |= 1 << i;
    A += a;
#pragma unroll
    for (int t = 0; t < 3; ++t) sum[t] += a * bgr[t];
}

// a row's chroma: the opacity-weighted mean colour of the block's pixels, converted, blended with the mean opacity over cnt
template <bool YUV = false>
ALIGN_HD void paste_block_chroma(const uint32_t sum[3], uint32_t A, PasteBlock& s, const YuvEncode* enc = nullptr)
{
    if (!s.uv || A == 0u) return;
    const uint32_t m[3] = {(sum[0] + A / 2u) / A, (sum[1] + A / 2u) / A, (sum[2] + A / 2u) / A};
    const uint32_t ac = (A + s.cnt / 2u) / s.cnt;
    if (ac == 0u) return;
    uint32_t uq, vq;
    if constexpr (YUV) yuv_chroma(*enc, m, uq, vq);
    else paste_nv12_chroma(m, uq, vq);
    s.u = paste_blend(ac, uq, s.u);
    s.v = paste_blend(ac, vq, s.v);
    s.wrote |= 16;
}

ALIGN_HD void paste_block_store(const PasteBlock& s)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (s.wrote >> i & 1) s.y[(long long)(i >> 1) * s.stride + (i & 1)] = (uint8_t)(s.luma >> (8 * i));
    if (s.wrote & 16) { s.uv[0] = (uint8_t)s.u; s.uv[1] = (uint8_t)s.v; }
}

// the pixels of block (BX, BY) that row n's footprint holds, as bits
template <class Shape>
ALIGN_HD int paste_block_holds(const PasteFrameDev& f, const Shape& shape, int n, const PasteCropDev& c, int BX, int BY)
{
    int held = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int X = 2 * BX + (i & 1), Y = 2 * BY + (i >> 1);
        AlignPos q;
        if (X < f.w && Y < f.h && paste_holds(shape, n, c, X, Y, q)) held |= 1 << i;
    }
    return held;
}

// The ownership rule on an NV12 frame: paste_owned with the block as its unit.  Block (BX, BY) as entry k of its frame's row list sees
// it: nothing unless entry k's footprint holds one of its pixels and no earlier entry's does -- else this is the one reader and writer of
// the block's luma bytes and of its UV pair: loaded once, entry k and every later entry applied in order (per pixel the taps and the luma
// blend, then the row's chroma), stored once.  chroma: the frame's UV plane.  The pixel loop is kept rolled: one pixel's taps are live
// at a time, the block's state is five registers.
// paste_owned_block_state: the rule up to the store -- false: not this entry's block; true: s is the block as it is to be stored (what the
// host program of tests/cpp reads the written bytes from).
template <bool YUV = false, class Shape>
ALIGN_HD bool paste_owned_block_state(const PasteFrameDev& f, uint8_t* chroma, const Shape& shape, const int* list, int k, const PasteCropDev& c,
                                      int BX, int BY, PasteBlock& s)
{
    if (!paste_block_holds(f, shape, list[k], c, BX, BY)) return false;
    for (int j = f.row_begin; j < k; ++j)
        if (paste_block_holds(f, shape, list[j], c, BX, BY)) return false;
    paste_block_load(f, chroma, c, BX, BY, s);
    const YuvEncode* const enc = YUV ? &yuv_tables.enc[yuv_encode_row(f.format)] : nullptr;
    for (int j = k; j < f.row_end; ++j) {
        const int n = list[j];
        uint32_t sum[3] = {0u, 0u, 0u}, A = 0u;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int X = 2 * BX + (i & 1), Y = 2 * BY + (i >> 1);
            AlignPos q;
            if (!(s.in >> i & 1) || !paste_holds(shape, n, c, X, Y, q)) continue;
            uint32_t bgr[3], a;
            paste_taps(shape, c, n, X, Y, q, bgr, a);
            if (a != 0u) paste_block_luma<YUV>(c, bgr, a, i, s, sum, A, enc);
        }
        paste_block_chroma<YUV>(sum, A, s, enc);
    }
    return true;
}

template <bool YUV = false, class Shape>
ALIGN_HD void paste_owned_block(const PasteFrameDev& f, uint8_t* chroma, const Shape& shape, const int* list, int k, const PasteCropDev& c,
                                int BX, int BY)
{
    PasteBlock s;
    if (paste_owned_block_state<YUV>(f, chroma, shape, list, k, c, BX, BY, s)) paste_block_store(s);
}
