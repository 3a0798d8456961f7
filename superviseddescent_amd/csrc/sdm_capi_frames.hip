// sdm_capi_frames.hip -- frames that are already on the device as the context's image set: gray and NV12 luma in place, colour
// converted into context-owned gray images by one launch (sdm_frames.hip) (C-ABI of include/sdm.h; shared declarations: sdm_capi_internal.h)
#include "sdm_capi_internal.h"

#include <limits.h>

// 0: not a format -- an unknown base; a matrix or range bit on a base that is not NV12 or P010; a matrix field above BT.2020; any other
// set bit ("YUV colour description and 10-bit surfaces")
int sdm_capi::frame_bpp(int format)
{
    const int base = SDM_FRAME_BASE(format);
    if (format < 0 || (format & ~(0xff | 0xf00 | SDM_FRAME_YUV_FULL))) return 0;
    if ((format & ~0xff) && base != SDM_FRAME_NV12 && base != SDM_FRAME_P010) return 0;
    if ((format & 0xf00) > SDM_FRAME_YUV_BT2020) return 0;
    switch (base) {
    case SDM_FRAME_GRAY: case SDM_FRAME_NV12: case SDM_FRAME_BGR_PLANAR: case SDM_FRAME_RGB_PLANAR: return 1;
    case SDM_FRAME_P010: return 2;
    case SDM_FRAME_BGR: case SDM_FRAME_RGB: return 3;
    case SDM_FRAME_BGRA: case SDM_FRAME_RGBA: return 4;
    default: return 0;
    }
}

bool sdm_capi::frame_planar(int format) { return format == SDM_FRAME_BGR_PLANAR || format == SDM_FRAME_RGB_PLANAR; }

bool sdm_capi::frame_in_place(int format) { const int b = SDM_FRAME_BASE(format); return b == SDM_FRAME_GRAY || b == SDM_FRAME_NV12; }

int sdm_capi::check_frame_uv(int i, const sdm_frame& f, const void* uv)
{
    const std::string at = "frame " + std::to_string(i) + ": ";
    const int base = SDM_FRAME_BASE(f.format);
    if (base == SDM_FRAME_NV12 && (long long)f.stride_bytes < 2ll * ((f.width + 1) / 2))
        return fail(SDM_ERR_INVALID, at + "an NV12 frame needs stride_bytes >= 2 * ((width + 1) / 2)");
    if (base == SDM_FRAME_P010) {
        if ((long long)f.stride_bytes < 4ll * ((f.width + 1) / 2))
            return fail(SDM_ERR_INVALID, at + "a P010 frame needs stride_bytes >= 4 * ((width + 1) / 2)");
        if ((uintptr_t)uv & 1) return fail(SDM_ERR_INVALID, at + "the UV plane of a P010 frame must be 2-byte aligned");
    }
    return SDM_OK;
}

int sdm_capi::frame_plane_distance(int i, const sdm_frame& f, const void* second, long long& D)
{
    D = second ? (long long)((intptr_t)second - (intptr_t)f.data) : (long long)f.height * f.stride_bytes;
    if (D == 0) return fail(SDM_ERR_INVALID, "frame " + std::to_string(i) + ": the second plane of a planar frame lies on the first");
    return SDM_OK;
}

int sdm_capi::check_frame(int i, const sdm_frame& f, bool allow_nv12)
{
    const std::string at = "frame " + std::to_string(i) + ": ";
    const int bpp = frame_bpp(f.format);
    if (!allow_nv12 && bpp && SDM_FRAME_BASE(f.format) == SDM_FRAME_NV12) return fail(SDM_ERR_INVALID, at + "an NV12 frame cannot be pasted into");
    if (!bpp) return fail(SDM_ERR_INVALID, at + "unknown format");
    if (!f.data) return fail(SDM_ERR_INVALID, at + "null pointer");
    if (f.width < 1 || f.height < 1) return fail(SDM_ERR_INVALID, at + "width and height must be >= 1");
    if ((long long)f.stride_bytes < (long long)f.width * bpp) return fail(SDM_ERR_INVALID, at + "stride_bytes < width * bytes per pixel");
    if (SDM_FRAME_BASE(f.format) == SDM_FRAME_P010 && ((((uintptr_t)f.data) | (uintptr_t)(unsigned)f.stride_bytes) & 1))
        return fail(SDM_ERR_INVALID, at + "the pointer and stride_bytes of a P010 frame must be even");
    return SDM_OK;
}

// sdm_set_frames_device (planes null) and sdm_set_frames_device_planes
static int set_frames_device(sdm_ctx* c, const sdm_frame* frames, const void* const* planes, int n, int gray_shift)
{
    if (!c || !frames || n < 1) return fail(SDM_ERR_INVALID, "bad frame list");
    if (gray_shift != 14 && gray_shift != 15) return fail(SDM_ERR_INVALID, "gray_shift must be 14 (OpenCV 2.4 - 3.x) or 15");
    // ---- every argument is checked before anything is allocated, copied or launched ----
    std::vector<FrameConvDev> conv;
    long long owned = 0, blocks = 0;
    int rc;
    for (int i = 0; i < n; ++i) {
        const sdm_frame& f = frames[i];
        if ((rc = check_frame(i, f, true))) return rc;
        const int bpp = frame_bpp(f.format);
        if (frame_in_place(f.format)) continue;
        FrameConvDev d{};
        if (frame_planar(f.format) && (rc = frame_plane_distance(i, f, planes ? planes[i] : nullptr, d.plane))) return rc;
        d.src = (const uint8_t*)f.data; d.dst_off = owned; d.w = f.width; d.h = f.height; d.pitch = f.stride_bytes;
        d.gstride = sdm_frames_gray_stride(f.width); d.bpp = bpp;
        d.swap_rb = f.format == SDM_FRAME_RGB || f.format == SDM_FRAME_RGBA || f.format == SDM_FRAME_RGB_PLANAR;
        d.block0 = (unsigned)blocks;
        // (a lane numbers its chunk within the frame in 32 bits, the launch its workgroups in 31)
        if (sdm_frames_blocks(f.width, f.height) * 256 > (long long)INT_MAX || blocks + sdm_frames_blocks(f.width, f.height) > (long long)INT_MAX)
            return fail(SDM_ERR_INVALID, "frame " + std::to_string(i) + ": more than 2^31 pixel chunks in one call");
        blocks += sdm_frames_blocks(f.width, f.height);
        owned += (long long)d.gstride * f.height;      // (a multiple of 16: the next image starts aligned)
        conv.push_back(d);
    }
    HIP_TRY(hipSetDevice(c->device));
    if (!conv.empty() && ((rc = c->frames.gray.ensure((size_t)owned)) || (rc = c->frames.desc.ensure(conv.size())))) return rc;
    if ((rc = c->img_off.ensure(n)) || (rc = c->img_w.ensure(n)) || (rc = c->img_h.ensure(n)) || (rc = c->img_stride.ensure(n)))
        return rc;
    // ---- the one table: in-place images at their own addresses, owned ones inside frames.gray; base = the lowest address ----
    std::vector<const uint8_t*> addr(n);
    std::vector<int> vw(n), vh(n), vs(n);
    bool narrow = false;
    for (int i = 0, k = 0; i < n; ++i) {
        const sdm_frame& f = frames[i];
        vw[i] = f.width; vh[i] = f.height;
        if (frame_in_place(f.format)) { addr[i] = (const uint8_t*)f.data; vs[i] = f.stride_bytes; }
        else { addr[i] = c->frames.gray.p + conv[k].dst_off; vs[i] = conv[k].gstride; ++k; }
        narrow = narrow || image_needs_generic(f.width, f.height, vs[i]);      // (the rule of every image entry point)
    }
    const uint8_t* base = addr[0];
    for (int i = 1; i < n; ++i) if (addr[i] < base) base = addr[i];
    std::vector<long long> off(n);
    for (int i = 0; i < n; ++i) off[i] = (long long)(addr[i] - base);
    HIP_TRY(hipMemcpyAsync(c->img_off.p, off.data(), n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->img_w.p, vw.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->img_h.p, vh.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->img_stride.p, vs.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (!conv.empty()) {
        HIP_TRY(hipMemcpyAsync(c->frames.desc.p, conv.data(), conv.size() * sizeof(FrameConvDev), hipMemcpyHostToDevice, c->stream));
        sdm_launch_frames_to_gray(c->frames.desc.p, (int)conv.size(), (unsigned)blocks, c->frames.gray.p, gray_shift, c->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->img_base = base;
    c->n_images = n;
    c->img_w_host.swap(vw); c->img_h_host.swap(vh);
    c->narrow_images = narrow;
    return SDM_OK;
}

extern "C" {

int sdm_set_frames_device(sdm_ctx* c, const sdm_frame* frames, int n, int gray_shift)
{
    return set_frames_device(c, frames, nullptr, n, gray_shift);
}

int sdm_set_frames_device_planes(sdm_ctx* c, const sdm_frame* frames, const void* const* planes, int n, int gray_shift)
{
    return set_frames_device(c, frames, planes, n, gray_shift);
}

int sdm_debug_download_image(sdm_ctx* c, int i, uint8_t* out)
{
    if (!c || !out || !c->img_base || i < 0 || i >= c->n_images) return fail(SDM_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    long long off = 0;
    int stride = 0;
    HIP_TRY(hipMemcpyAsync(&off, c->img_off.p + i, sizeof(off), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&stride, c->img_stride.p + i, sizeof(stride), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int w = c->img_w_host[i], h = c->img_h_host[i];
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)w, c->img_base + off, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

}  // extern "C"
