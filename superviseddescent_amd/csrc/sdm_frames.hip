// sdm_frames.hip -- colour frames that are already on the device -> the context's gray images (sdm_set_frames_device, include/sdm.h).
// One launch converts every colour frame of a call: interleaved BGR / RGB / BGRA / RGBA, planar BGR / RGB (three planes of one byte
// per pixel, any signed distance apart) and the luma plane of P010 (16-bit words, gray = min(255, ((word >> 6) + 2) >> 2): include/sdm.h,
// "YUV colour description and 10-bit surfaces") of any size, pitch and pointer alignment into gray images the context owns, with the
// arithmetic of bgr2gray_kernel (sdm_apply.hip; cv::cvtColor's fixed-point weights, adaptive_vlhog.hpp:114-120).  The source is
// only read.
#include "sdm_kernels.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// the source pointers come out of the descriptor table: named as global memory, or the loads would be flat ones
typedef const __attribute__((address_space(1))) uint8_t* gbytes;
// a 16-byte access that is only known to be 4-byte aligned (global_load_dwordx4 asks for dword alignment, not for 16 bytes)
struct __attribute__((packed, aligned(4))) Quad { u32x4 v; };

__device__ __forceinline__ unsigned gray_of(unsigned p0, unsigned p1, unsigned p2, int c0, int c1, int c2, int half, int shift)
{
    // bgr2gray_kernel's sum; every product and the sum stay below 2^24 (255 * 2^shift + half), so the 24-bit multiplier gives the same bits
    return (__umul24(p0, (unsigned)c0) + __umul24(p1, (unsigned)c1) + __umul24(p2, (unsigned)c2) + (unsigned)half) >> shift;
}

// four 3-byte pixels in three dwords -> four gray bytes in one dword (the unpacking of bgr2gray_kernel)
__device__ __forceinline__ unsigned gray4_of_12(unsigned w0, unsigned w1, unsigned w2, int c0, int c1, int c2, int half, int shift)
{
    return gray_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, c0, c1, c2, half, shift) |
           gray_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, c0, c1, c2, half, shift) << 8 |
           gray_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, c0, c1, c2, half, shift) << 16 |
           gray_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, c0, c1, c2, half, shift) << 24;
}

// four 4-byte pixels (the fourth byte, alpha, is not used) -> four gray bytes
__device__ __forceinline__ unsigned gray4_of_16(u32x4 q, int c0, int c1, int c2, int half, int shift)
{
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) out |= gray_of(q[k] & 255u, (q[k] >> 8) & 255u, (q[k] >> 16) & 255u, c0, c1, c2, half, shift) << (8 * k);
    return out;
}

// Work unit of a lane: a CHUNK of 16 consecutive pixels of one row (48 or 64 source bytes, 16 gray bytes).  The chunks of a frame
// are numbered row by row (chunks_per_row = ceil(w / 16)); a workgroup takes 256 consecutive chunks of ONE frame (block0 of the
// descriptors: the frame's first workgroup), so the frame's descriptor is wave-uniform and comes through scalar loads.
//   wide path   the row starts on a 4-byte boundary (decoder pitches, torch rows) and the chunk is complete: three (BGR) or four
//               (BGRA) 16-byte loads -- a chunk starts 48 c or 64 c bytes into its row, so it is as aligned as the row is
//   byte path   the last, incomplete chunk of a row, and every chunk of a row that does not start on a 4-byte boundary: one byte
//               load per channel, only of pixels that exist
// A planar frame's chunk is 16 bytes of each plane: one 16-byte load per plane when the chunk is complete and the row start and the
// plane distance are multiples of 4 (so all three row starts are 4-byte aligned), the byte path otherwise.
// Either way the lane stores ONE 16-byte word: the owned gray images start on 16-byte boundaries with a row stride that is a
// multiple of 16 (sdm_frames_gray_stride), so the store is aligned and the bytes behind the last pixel of a row land in that
// row's own padding (written as zero, never read as pixels: the pixel kernels take w and the stride from the image table).
__global__ void __launch_bounds__(256) frames_to_gray_kernel(const FrameConvDev* __restrict__ frames, int n_frames, uint8_t* __restrict__ gray,
                                                             int cb, int cg, int cr, int shift)
{
    // the frame of this workgroup: the last descriptor with block0 <= blockIdx.x (uniform binary search, scalar loads)
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frames[mid].block0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const FrameConvDev f = frames[lo];
    const unsigned cpr = ((unsigned)f.w + 15u) >> 4;
    const unsigned id = (blockIdx.x - f.block0) * 256u + threadIdx.x;      // (< 2^31: checked by the host)
    const unsigned row = id / cpr, c = id - row * cpr;
    if (row >= (unsigned)f.h) return;
    const int c0 = f.swap_rb ? cr : cb, c1 = cg, c2 = f.swap_rb ? cb : cr;      // weights of byte 0, 1, 2 of a pixel
    const int half = 1 << (shift - 1);
    gbytes rowp = (gbytes)f.src + (long long)row * f.pitch;
    const int npx = min(16, f.w - (int)(c * 16u));
    u32x4 out = {0u, 0u, 0u, 0u};
    if (f.bpp == 1) {
        // planar: the chunk is 16 bytes of each plane, f.plane bytes apart (64-bit, any sign); as aligned as the three row starts are
        gbytes p0 = rowp + (size_t)c * 16, p1 = p0 + f.plane, p2 = p1 + f.plane;
        if (npx == 16 && (((size_t)rowp | (size_t)f.plane) & 3) == 0) {
            const u32x4 a = ((const __attribute__((address_space(1))) Quad*)p0)->v, b = ((const __attribute__((address_space(1))) Quad*)p1)->v,
                        d = ((const __attribute__((address_space(1))) Quad*)p2)->v;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int s = 8 * (k & 3);
                out[k >> 2] |= gray_of((a[k >> 2] >> s) & 255u, (b[k >> 2] >> s) & 255u, (d[k >> 2] >> s) & 255u, c0, c1, c2, half, shift) << s;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < npx) out[k >> 2] |= gray_of(p0[k], p1[k], p2[k], c0, c1, c2, half, shift) << (8 * (k & 3));
        }
    } else if (f.bpp == 2) {
        // P010 luma: 16 words of 16 bits, the sample in bits 15..6; gray = min(255, ((word >> 6) + 2) >> 2).  The UV plane is not read.
        gbytes p = rowp + (size_t)c * 32;
        if (npx == 16 && ((size_t)rowp & 3) == 0) {
            const __attribute__((address_space(1))) Quad* q = (const __attribute__((address_space(1))) Quad*)p;
            const u32x4 a = q[0].v, b = q[1].v;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned pair = k < 8 ? a[k >> 1] : b[(k - 8) >> 1];
                const unsigned word = (k & 1) ? pair >> 16 : pair & 0xffffu;
                out[k >> 2] |= min(255u, ((word >> 6) + 2u) >> 2) << (8 * (k & 3));
            }
        } else {
            const __attribute__((address_space(1))) uint16_t* w16 = (const __attribute__((address_space(1))) uint16_t*)p;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < npx) out[k >> 2] |= min(255u, (((unsigned)w16[k] >> 6) + 2u) >> 2) << (8 * (k & 3));
        }
    } else if (npx == 16 && ((size_t)rowp & 3) == 0) {
        if (f.bpp == 3) {
            const __attribute__((address_space(1))) Quad* q = (const __attribute__((address_space(1))) Quad*)(rowp + (size_t)c * 48);
            const u32x4 a = q[0].v, b = q[1].v, d = q[2].v;
            out[0] = gray4_of_12(a[0], a[1], a[2], c0, c1, c2, half, shift);
            out[1] = gray4_of_12(a[3], b[0], b[1], c0, c1, c2, half, shift);
            out[2] = gray4_of_12(b[2], b[3], d[0], c0, c1, c2, half, shift);
            out[3] = gray4_of_12(d[1], d[2], d[3], c0, c1, c2, half, shift);
        } else {
            const __attribute__((address_space(1))) Quad* q = (const __attribute__((address_space(1))) Quad*)(rowp + (size_t)c * 64);
            const u32x4 a = q[0].v, b = q[1].v, d = q[2].v, e = q[3].v;
            out[0] = gray4_of_16(a, c0, c1, c2, half, shift);
            out[1] = gray4_of_16(b, c0, c1, c2, half, shift);
            out[2] = gray4_of_16(d, c0, c1, c2, half, shift);
            out[3] = gray4_of_16(e, c0, c1, c2, half, shift);
        }
    } else {
        gbytes p = rowp + (size_t)c * 16 * f.bpp;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < npx) {
                gbytes s = p + k * f.bpp;
                out[k >> 2] |= gray_of(s[0], s[1], s[2], c0, c1, c2, half, shift) << (8 * (k & 3));
            }
        }
    }
    *(u32x4*)(gray + f.dst_off + (long long)row * f.gstride + (size_t)c * 16) = out;
}

}  // namespace

void sdm_launch_frames_to_gray(const FrameConvDev* frames_dev, int n_frames, unsigned n_blocks, uint8_t* gray, int shift, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
    const int cb = shift == 15 ? 3735 : 1868, cg = shift == 15 ? 19235 : 9617, cr = shift == 15 ? 9798 : 4899;      // (sdm_launch_bgr2gray's)
    hipLaunchKernelGGL(frames_to_gray_kernel, dim3(n_blocks), dim3(256), 0, stream, frames_dev, n_frames, gray, cb, cg, cr, shift);
}
