// sdm_capi_align.hip -- C-ABI of the aligned face crops (include/sdm.h, sdm_align_*): the source of the taps in sdm_ctx::align, and a
// call that fits every current row's similarity and warps its image into a crop (csrc/sdm_align.hip).  Every argument is checked
// before anything is launched; the landmark state, the images and the tracker's slots are only read.  sdm_align_set_source_frames and
// sdm_align_crops_tensor (csrc/sdm_align_tensor.hip): a frame list used in place as the source, and the crops as a network's input tensor;
// sdm_align_crops_tensor_filtered (csrc/sdm_align_area.hip): that tensor with a minifying row's pixels averaged over their footprint.
// The way back, sdm_align_paste_tensor, is csrc/sdm_capi_paste.hip; it shares the checks and the fit below.
#include "sdm_capi_internal.h"

#include <cmath>
#include <limits.h>

// what sdm_align_crops and sdm_align_crops_tensor check alike, before anything is launched: geometry, rows, indices, template, crop
// size, and that the source covers every row's image with that image's size
int sdm_capi::align_check_call(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h)
{
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    if (c->N < 1) return fail(SDM_ERR_INVALID, "no current rows (sdm_set_x, sdm_detect_batch or sdm_track_step first)");
    if (!lm || !tmpl) return fail(SDM_ERR_INVALID, "no landmark indices or template");
    int rc;
    if ((rc = check_landmark_subset(c, lm, tmpl, K, 2))) return rc;
    bool spread = false;
    for (int k = 1; k < K && !spread; ++k) spread = tmpl[2 * k] != tmpl[0] || tmpl[2 * k + 1] != tmpl[1];
    if (!spread) return fail(SDM_ERR_INVALID, "the K template points coincide");
    if (out_w < 1 || out_w > 1024 || out_h < 1 || out_h > 1024) return fail(SDM_ERR_INVALID, "crop width and height must be in [1, 1024]");
    return SDM_OK;
}

int sdm_capi::check_landmark_subset(const sdm_ctx* c, const int* lm, const float* tmpl, int K, int Kmin)
{
    const int L = c->L;
    if (K < Kmin || K > L) return fail(SDM_ERR_INVALID, "K must be in [" + std::to_string(Kmin) + ", L]");
    std::vector<char> seen(L, 0);
    for (int k = 0; k < K; ++k) {
        if (lm[k] < 0 || lm[k] >= L) return fail(SDM_ERR_INVALID, "landmark index " + std::to_string(lm[k]) + " out of range");
        if (seen[lm[k]]) return fail(SDM_ERR_INVALID, "landmark index " + std::to_string(lm[k]) + " named twice");
        seen[lm[k]] = 1;
    }
    for (int k = 0; k < 2 * K; ++k)
        if (!std::isfinite(tmpl[k])) return fail(SDM_ERR_INVALID, "a template point is not finite");
    return SDM_OK;
}

// what sdm_align_crops_tensor refuses of its specification and of its output (sdm_warp_crops_tensor refuses the same)
int sdm_capi::align_check_spec(const sdm_align_tensor* spec)
{
    if (!spec) return fail(SDM_ERR_INVALID, "no tensor specification");
    if (spec->dtype != SDM_ALIGN_U8 && spec->dtype != SDM_ALIGN_F16 && spec->dtype != SDM_ALIGN_F32) return fail(SDM_ERR_INVALID, "unknown dtype");
    if (spec->layout != SDM_ALIGN_NHWC && spec->layout != SDM_ALIGN_NCHW) return fail(SDM_ERR_INVALID, "unknown layout");
    if (spec->order != SDM_ALIGN_ORDER_BGR && spec->order != SDM_ALIGN_ORDER_RGB) return fail(SDM_ERR_INVALID, "unknown channel order");
    if (spec->channels != 1 && spec->channels != 3) return fail(SDM_ERR_INVALID, "channels must be 1 or 3");
    if (spec->gray_shift != 14 && spec->gray_shift != 15) return fail(SDM_ERR_INVALID, "gray_shift must be 14 (OpenCV 2.4 - 3.x) or 15");
    if (spec->dtype != SDM_ALIGN_U8)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(spec->scale[k]) || !std::isfinite(spec->bias[k])) return fail(SDM_ERR_INVALID, "a scale or bias is not finite");
    return SDM_OK;
}

int sdm_capi::align_check_out(const void* out_dev)
{
    if (!out_dev) return fail(SDM_ERR_INVALID, "no output");
    if ((uintptr_t)out_dev % 16 != 0) return fail(SDM_ERR_INVALID, "the output must be 16-byte aligned");
    return SDM_OK;
}

AlignTensorDev sdm_capi::align_tensor_dev(const sdm_align_tensor* spec)
{
    AlignTensorDev t{};
    for (int k = 0; k < 3; ++k) { t.scale[k] = spec->scale[k]; t.bias[k] = spec->bias[k]; }
    t.order = spec->order;
    align_gray_weights(spec->gray_shift, t);
    return t;
}

AlignSourceDev sdm_capi::align_source_dev(const sdm_ctx* c)
{
    const sdm_ctx::Align& a = c->align;
    AlignSourceDev src{};
    if (a.base) {
        src.ctx.base = nullptr;
        src.width = a.w; src.height = a.h; src.stride = a.stride;
    } else {
        src.ctx = image_set(c);          // (a frame list: sizes from the context's images, which are the frames'; the rest from the table)
    }
    return src;
}

AlignTapSource sdm_capi::align_tap_source(const sdm_ctx* c)
{
    const sdm_ctx::Align& a = c->align;
    const bool external = a.base != nullptr;
    return {external ? a.base : c->img_base, a.fr.empty() ? nullptr : a.fr_dev.p,
            !external ? SDM_FRAME_GRAY : a.C == 1 ? SDM_FRAME_GRAY : a.C == 3 ? SDM_FRAME_BGR : SDM_FRAME_BGRA};
}

int sdm_capi::align_check_rows(sdm_ctx* c)
{
    const sdm_ctx::Align& a = c->align;
    const int N = c->N;
    const bool external = a.base != nullptr, list = !a.fr.empty();
    // every row's image: in the context's set, and -- external stack or frame list -- in the source with that image's size
    if (!c->img_base || c->n_images < 1) return fail(SDM_ERR_INVALID, "no images set");
    const int n_src = external ? std::min(a.n, c->n_images) : list ? std::min((int)a.fr.size(), c->n_images) : c->n_images;
    if (c->idx_identity && N > n_src) return fail(SDM_ERR_INVALID, "more rows than source images and no sample->image index set");
    if (!c->idx_identity && N > c->n_idx) return fail(SDM_ERR_INVALID, "sample->image index is shorter than the rows");
    for (int r = 0; r < N; ++r) {
        const int im = c->idx_identity ? r : c->img_idx_host[r];
        if (im >= n_src) return fail(SDM_ERR_INVALID, "row " + std::to_string(r) + " maps to image " + std::to_string(im) + ", beyond the source");
        if (external && (c->img_w_host[im] != a.w || c->img_h_host[im] != a.h))
            return fail(SDM_ERR_INVALID, "the source stack's image size differs from image " + std::to_string(im) + " of the context");
        if (list && (c->img_w_host[im] != a.fr[im].width || c->img_h_host[im] != a.fr[im].height))
            return fail(SDM_ERR_INVALID, "frame " + std::to_string(im) + " of the source differs in size from image " + std::to_string(im) + " of the context");
    }
    return SDM_OK;
}

// the K indices and the template in, the fit of every row into a.faces (the buffers are there)
int sdm_capi::align_fit_rows(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h)
{
    sdm_ctx::Align& a = c->align;
    std::vector<int> in((size_t)3 * K);
    memcpy(in.data(), lm, (size_t)K * sizeof(int));
    memcpy(in.data() + K, tmpl, (size_t)2 * K * sizeof(float));
    HIP_TRY(hipMemcpyAsync(a.in.p, in.data(), in.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    sdm_launch_align_fit(c->x[c->cur].p, c->N, c->L, a.in.p, (const float*)(a.in.p + K), K, align_source_dev(c),
                         c->idx_identity ? nullptr : c->img_idx.p, out_w, out_h, a.faces.p, c->stream);
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

int sdm_capi::align_check_filter(const sdm_align_filter* filter)
{
    if (!filter) return fail(SDM_ERR_INVALID, "no filter");
    if (filter->mode != SDM_ALIGN_FILTER_BILINEAR && filter->mode != SDM_ALIGN_FILTER_AREA) return fail(SDM_ERR_INVALID, "unknown filter mode");
    if (filter->max_samples < 1 || filter->max_samples > 16) return fail(SDM_ERR_INVALID, "max_samples must be in [1, 16]");
    if (!std::isfinite(filter->min_scale) || filter->min_scale < 1.0f) return fail(SDM_ERR_INVALID, "min_scale must be finite and >= 1");
    return SDM_OK;
}

AlignAreaDev sdm_capi::align_area_dev(const sdm_align_filter* filter)
{
    AlignAreaDev area{};
    area.mode = filter->mode; area.max_samples = filter->max_samples;
    area.min2 = filter->min_scale * filter->min_scale;                              // (float32, rounded once; may be inf: then every S is 1)
    return area;
}

size_t sdm_capi::align_face_records(int N, bool with_samples)
{
    return (size_t)N + (with_samples ? ((size_t)N * sizeof(int) + sizeof(AlignFace) - 1) / sizeof(AlignFace) : 0);
}

// the records -- and, behind them in the same buffer, the rows' S when `samples_host` is given -- in one copy, one synchronise
int sdm_capi::align_fetch_rows(sdm_ctx* c, int N, float* matrices_host, int* flags_host, int* samples_host)
{
    const size_t rec = (size_t)N * sizeof(AlignFace), bytes = rec + (samples_host ? (size_t)N * sizeof(int) : 0);
    std::vector<unsigned char> host;
    if (matrices_host || flags_host || samples_host) {
        host.resize(bytes);
        HIP_TRY(hipMemcpyAsync(host.data(), c->align.faces.p, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (host.empty()) return SDM_OK;
    const AlignFace* faces = (const AlignFace*)host.data();
    for (int r = 0; r < N; ++r) {
        if (matrices_host) memcpy(matrices_host + (size_t)6 * r, faces[r].m, 6 * sizeof(float));
        if (flags_host) flags_host[r] = faces[r].flags;
    }
    if (samples_host) memcpy(samples_host, host.data() + rec, (size_t)N * sizeof(int));
    return SDM_OK;
}

// sdm_align_crops_tensor (filter null) and sdm_align_crops_tensor_filtered: the same checks, the same fit, one launch behind it
static int align_tensor_call(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h, const sdm_align_tensor* spec,
                             const sdm_align_filter* filter, bool filtered, void* out_dev, float* matrices_host, int* flags_host,
                             int* samples_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = align_check_call(c, lm, tmpl, K, out_w, out_h))) return rc;
    if ((rc = align_check_spec(spec))) return rc;
    if (filtered && (rc = align_check_filter(filter))) return rc;
    if ((rc = align_check_out(out_dev))) return rc;
    if ((rc = align_check_rows(c))) return rc;
    const int N = c->N;
    sdm_ctx::Align& a = c->align;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = a.in.ensure((size_t)3 * K)) || (rc = a.faces.ensure(align_face_records(N, filtered)))) return rc;
    if ((rc = align_fit_rows(c, lm, tmpl, K, out_w, out_h))) return rc;
    const AlignTensorDev t = align_tensor_dev(spec);
    const AlignTapSource src = align_tap_source(c);
    const int* img_idx = c->idx_identity ? nullptr : c->img_idx.p;
    if (!filtered) {
        sdm_launch_align_tensor(src.base, a.faces.p, src.frames, img_idx, src.stack_format, N, out_w, out_h, spec->dtype, spec->layout,
                                spec->channels, t, out_dev, c->stream);
        HIP_TRY(hipGetLastError());
        return align_fetch_rows(c, N, matrices_host, flags_host, nullptr);
    }
    sdm_launch_align_area(src.base, a.faces.p, src.frames, img_idx, src.stack_format, N, out_w, out_h, spec->dtype, spec->layout,
                          spec->channels, t, align_area_dev(filter), (int*)(a.faces.p + N), out_dev, c->stream);
    HIP_TRY(hipGetLastError());
    return align_fetch_rows(c, N, matrices_host, flags_host, samples_host);
}

extern "C" {

int sdm_align_set_source(sdm_ctx* c, const uint8_t* base, int n_images, int width, int height, int stride_bytes, int channels,
                         int on_device)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    sdm_ctx::Align& a = c->align;
    if (!base) { a.base = nullptr; a.n = 0; a.C = 1; a.fr.clear(); return SDM_OK; }          // the context's images
    if (n_images < 1 || width < 1 || height < 1) return fail(SDM_ERR_INVALID, "an image stack needs n_images, width and height >= 1");
    if (channels != 1 && channels != 3 && channels != 4) return fail(SDM_ERR_INVALID, "channels must be 1, 3 or 4");
    if ((long long)stride_bytes < (long long)width * channels) return fail(SDM_ERR_INVALID, "stride_bytes < width * channels");
    HIP_TRY(hipSetDevice(c->device));
    const uint8_t* dev = base;
    if (!on_device) {
        // the bytes the warp can reach: up to the last pixel of the last row (a caller's row padding behind it need not exist)
        const size_t bytes = ((size_t)n_images * height - 1) * (size_t)stride_bytes + (size_t)width * channels;
        if (a.base == a.owned.p) { a.base = nullptr; a.n = 0; a.C = 1; }   // (the copy may be reallocated below: never left dangling)
        int rc = a.owned.ensure(bytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(a.owned.p, base, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        dev = a.owned.p;
    }
    a.base = dev; a.n = n_images; a.w = width; a.h = height; a.stride = stride_bytes; a.C = channels;
    a.fr.clear();                                                             // (a stack replaces a frame list)
    return SDM_OK;
}

int sdm_align_set_source_frames(sdm_ctx* c, const sdm_frame* frames, const void* const* chroma, int n)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    sdm_ctx::Align& a = c->align;
    if (n < 0) return fail(SDM_ERR_INVALID, "bad frame list");
    if (!frames || n == 0) { a.base = nullptr; a.n = 0; a.C = 1; a.fr.clear(); return SDM_OK; }     // the context's images
    // ---- every argument is checked before anything is allocated or copied ----
    std::vector<AlignFrameDev> tab((size_t)n);
    int bpp_all = -1, rc;
    const uint8_t* lowest = nullptr;
    for (int i = 0; i < n; ++i) {
        const sdm_frame& f = frames[i];
        if ((rc = check_frame(i, f, true))) return rc;
        const int bpp = frame_bpp(f.format);
        AlignFrameDev& d = tab[i];
        d.p0 = (const uint8_t*)f.data; d.p1 = nullptr; d.stride = f.stride_bytes; d.cstride = 0; d.format = f.format; d.pad = 0;
        const int fbase = SDM_FRAME_BASE(f.format);
        if (fbase == SDM_FRAME_NV12 || fbase == SDM_FRAME_P010) {
            const void* uv = chroma ? chroma[i] : nullptr;
            d.p1 = uv ? (const uint8_t*)uv : (const uint8_t*)f.data + (size_t)f.height * (size_t)f.stride_bytes;
            if ((rc = check_frame_uv(i, f, d.p1))) return rc;
            d.cstride = f.stride_bytes;
        }
        if (frame_planar(f.format)) {
            long long D;
            if ((rc = frame_plane_distance(i, f, chroma ? chroma[i] : nullptr, D))) return rc;
            d.p1 = (const uint8_t*)f.data + D;
        }
        const int kind = fbase == SDM_FRAME_NV12 || fbase == SDM_FRAME_P010 || frame_planar(f.format) ? 0 : bpp;
        bpp_all = bpp_all < 0 ? kind : (bpp_all == kind ? kind : 0);
        if (!lowest || d.p0 < lowest) lowest = d.p0;
    }
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = a.fr_dev.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpyAsync(a.fr_dev.p, tab.data(), (size_t)n * sizeof(AlignFrameDev), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    a.base = nullptr; a.n = 0; a.C = bpp_all > 0 ? bpp_all : 1;                // (a frame list replaces a stack)
    a.fr.assign(frames, frames + n);
    a.fr_base = lowest; a.fr_bpp = bpp_all;
    return SDM_OK;
}

int sdm_align_crops(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h, uint8_t* out, int out_on_device,
                    float* matrices_host, int* flags_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = align_check_call(c, lm, tmpl, K, out_w, out_h))) return rc;
    const int N = c->N;
    sdm_ctx::Align& a = c->align;
    const bool external = a.base != nullptr, list = !a.fr.empty();
    if (list && a.fr_bpp == 0)
        return fail(SDM_ERR_INVALID, "the frame-list source holds NV12, P010 or planar frames or frames of different pixel sizes: use sdm_align_crops_tensor");
    const int C = external ? a.C : list ? a.fr_bpp : 1;
    if (!out) return fail(SDM_ERR_INVALID, "no output");
    if (out_on_device && ((uintptr_t)out % (C == 4 ? 16 : 4)) != 0)
        return fail(SDM_ERR_INVALID, "a device output must be 4-byte aligned (16 when C = 4)");
    if ((rc = align_check_rows(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t crop_bytes = (size_t)N * out_w * out_h * C;
    if ((rc = a.in.ensure((size_t)3 * K)) || (rc = a.faces.ensure((size_t)N)) || (!out_on_device && (rc = a.crops.ensure(crop_bytes))))
        return rc;
    if ((rc = align_fit_rows(c, lm, tmpl, K, out_w, out_h))) return rc;
    const uint8_t* img = external ? a.base : c->img_base;
    if (list) {
        img = a.fr_base;
        sdm_launch_align_frame_rows(a.faces.p, a.fr_dev.p, c->idx_identity ? nullptr : c->img_idx.p, img, N, c->stream);
        HIP_TRY(hipGetLastError());
    }
    uint8_t* dst = out_on_device ? out : a.crops.p;
    sdm_launch_align_warp(img, a.faces.p, N, out_w, out_h, C, dst, c->stream);
    HIP_TRY(hipGetLastError());
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, a.crops.p, crop_bytes, hipMemcpyDeviceToHost, c->stream));
    return align_fetch_rows(c, N, matrices_host, flags_host, nullptr);
}

int sdm_align_crops_tensor(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h, const sdm_align_tensor* spec,
                           void* out_dev, float* matrices_host, int* flags_host)
{
    return align_tensor_call(c, lm, tmpl, K, out_w, out_h, spec, nullptr, false, out_dev, matrices_host, flags_host, nullptr);
}

int sdm_align_crops_tensor_filtered(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h, const sdm_align_tensor* spec,
                                    const sdm_align_filter* filter, void* out_dev, float* matrices_host, int* flags_host, int* samples_host)
{
    return align_tensor_call(c, lm, tmpl, K, out_w, out_h, spec, filter, true, out_dev, matrices_host, flags_host, samples_host);
}

}  // extern "C"
