// sdm_capi_align.hip -- C-ABI of the aligned face crops (include/sdm.h, sdm_align_*): the source of the taps in sdm_ctx::align, and a
// call that fits every current row's similarity and warps its image into a crop (csrc/sdm_align.hip).  Every argument is checked
// before anything is launched; the landmark state, the images and the tracker's slots are only read.
#include "sdm_capi_internal.h"

#include <cmath>

extern "C" {

int sdm_align_set_source(sdm_ctx* c, const uint8_t* base, int n_images, int width, int height, int stride_bytes, int channels,
                         int on_device)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    sdm_ctx::Align& a = c->align;
    if (!base) { a.base = nullptr; a.n = 0; a.C = 1; return SDM_OK; }          // the context's images
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
    return SDM_OK;
}

int sdm_align_crops(sdm_ctx* c, const int* lm, const float* tmpl, int K, int out_w, int out_h, uint8_t* out, int out_on_device,
                    float* matrices_host, int* flags_host)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    const int L = c->L, N = c->N;
    if (N < 1) return fail(SDM_ERR_INVALID, "no current rows (sdm_set_x, sdm_detect_batch or sdm_track_step first)");
    if (!lm || !tmpl) return fail(SDM_ERR_INVALID, "no landmark indices or template");
    if (K < 2 || K > L) return fail(SDM_ERR_INVALID, "K must be in [2, L]");
    std::vector<char> seen(L, 0);
    for (int k = 0; k < K; ++k) {
        if (lm[k] < 0 || lm[k] >= L) return fail(SDM_ERR_INVALID, "landmark index " + std::to_string(lm[k]) + " out of range");
        if (seen[lm[k]]) return fail(SDM_ERR_INVALID, "landmark index " + std::to_string(lm[k]) + " named twice");
        seen[lm[k]] = 1;
    }
    bool spread = false;
    for (int k = 0; k < 2 * K; ++k)
        if (!std::isfinite(tmpl[k])) return fail(SDM_ERR_INVALID, "a template point is not finite");
    for (int k = 1; k < K && !spread; ++k) spread = tmpl[2 * k] != tmpl[0] || tmpl[2 * k + 1] != tmpl[1];
    if (!spread) return fail(SDM_ERR_INVALID, "the K template points coincide");
    if (out_w < 1 || out_w > 1024 || out_h < 1 || out_h > 1024) return fail(SDM_ERR_INVALID, "crop width and height must be in [1, 1024]");
    sdm_ctx::Align& a = c->align;
    const bool external = a.base != nullptr;
    const int C = external ? a.C : 1;
    if (!out) return fail(SDM_ERR_INVALID, "no output");
    if (out_on_device && ((uintptr_t)out % (C == 4 ? 16 : 4)) != 0)
        return fail(SDM_ERR_INVALID, "a device output must be 4-byte aligned (16 when C = 4)");
    // every row's image: in the context's set, and -- external stack -- in the stack with that image's size
    if (!c->img_base || c->n_images < 1) return fail(SDM_ERR_INVALID, "no images set");
    const int n_src = external ? std::min(a.n, c->n_images) : c->n_images;
    if (c->idx_identity && N > n_src) return fail(SDM_ERR_INVALID, "more rows than source images and no sample->image index set");
    if (!c->idx_identity && N > c->n_idx) return fail(SDM_ERR_INVALID, "sample->image index is shorter than the rows");
    for (int r = 0; r < N; ++r) {
        const int im = c->idx_identity ? r : c->img_idx_host[r];
        if (im >= n_src) return fail(SDM_ERR_INVALID, "row " + std::to_string(r) + " maps to image " + std::to_string(im) + ", beyond the source");
        if (external && (c->img_w_host[im] != a.w || c->img_h_host[im] != a.h))
            return fail(SDM_ERR_INVALID, "the source stack's image size differs from image " + std::to_string(im) + " of the context");
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t crop_bytes = (size_t)N * out_w * out_h * C;
    int rc;
    if ((rc = a.in.ensure((size_t)3 * K)) || (rc = a.faces.ensure((size_t)N)) || (!out_on_device && (rc = a.crops.ensure(crop_bytes))))
        return rc;
    std::vector<int> in((size_t)3 * K);
    memcpy(in.data(), lm, (size_t)K * sizeof(int));
    memcpy(in.data() + K, tmpl, (size_t)2 * K * sizeof(float));
    HIP_TRY(hipMemcpyAsync(a.in.p, in.data(), in.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    AlignSourceDev src{};
    const uint8_t* img;
    if (external) {
        src.ctx.base = nullptr;
        src.width = a.w; src.height = a.h; src.stride = a.stride;
        img = a.base;
    } else {
        src.ctx = image_set(c);
        img = c->img_base;
    }
    sdm_launch_align_fit(c->x[c->cur].p, N, L, a.in.p, (const float*)(a.in.p + K), K, src, c->idx_identity ? nullptr : c->img_idx.p,
                         out_w, out_h, a.faces.p, c->stream);
    HIP_TRY(hipGetLastError());
    uint8_t* dst = out_on_device ? out : a.crops.p;
    sdm_launch_align_warp(img, a.faces.p, N, out_w, out_h, C, dst, c->stream);
    HIP_TRY(hipGetLastError());
    std::vector<AlignFace> faces;
    if (matrices_host || flags_host) {
        faces.resize((size_t)N);
        HIP_TRY(hipMemcpyAsync(faces.data(), a.faces.p, (size_t)N * sizeof(AlignFace), hipMemcpyDeviceToHost, c->stream));
    }
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, a.crops.p, crop_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int r = 0; r < (int)faces.size(); ++r) {
        if (matrices_host) memcpy(matrices_host + (size_t)6 * r, faces[r].m, 6 * sizeof(float));
        if (flags_host) flags_host[r] = faces[r].flags;
    }
    return SDM_OK;
}

}  // extern "C"
