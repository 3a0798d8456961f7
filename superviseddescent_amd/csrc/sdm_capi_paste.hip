// sdm_capi_paste.hip -- C-ABI of the paste-back of crop tensors into frames (include/sdm.h, "Pasting crops back" and "Pasting warped
// faces back"): the entry points check every argument before anything is launched or changed, build the frame table and the rows-of-frame lists on the host from the
// image index they already hold, and enqueue -- fit form -- sdm_align_crops' fit, then the prepare kernel and the one paste launch
// (csrc/sdm_align_paste.hip: paste_kernel_t<NV12, AREA>), the filtered forms behind that file's filtered prepare kernel, the NV12 forms
// with the frames' UV planes as a device array of their own; the piecewise-affine forms enqueue warp_fit_kernel, their prepare kernel and their paste launch
// (csrc/sdm_warp_paste.hip: warp_paste_kernel_t<NV12, AREA>) on the mesh of sdm_warp_set_mesh, their NV12 forms with the same array of UV
// planes, their filtered forms the counts stage ahead of it.  Nothing waits between
// them; the one synchronise of a call brings the matrices and flags back.  The landmark state, the images, the crop source and the
// tracker's slots are only read; the frames' colour bytes are written in place.
#include "sdm_capi_internal.h"
#include "sdm_paste.h"

#include <cmath>

namespace {

// what both forms refuse of the tensor, the opacity maps and the destination frames
int paste_check_args(const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, bool nv12 = false,
                     void* const* dst_chroma = nullptr)
{
    if (!in_dev) return fail(SDM_ERR_INVALID, "no tensor");
    if ((uintptr_t)in_dev % 16 != 0) return fail(SDM_ERR_INVALID, "the tensor must be 16-byte aligned");
    if (!paste) return fail(SDM_ERR_INVALID, "no paste options");
    if (paste->alpha_per_row != 0 && paste->alpha_per_row != 1) return fail(SDM_ERR_INVALID, "alpha_per_row must be 0 or 1");
    if (!frames || n_frames < 1) return fail(SDM_ERR_INVALID, "bad frame list");
    int rc;
    for (int i = 0; i < n_frames; ++i) {
        if ((rc = check_frame(i, frames[i], nv12))) return rc;
        if (SDM_FRAME_BASE(frames[i].format) == SDM_FRAME_P010)
            return fail(SDM_ERR_INVALID, "frame " + std::to_string(i) + ": a P010 frame cannot be pasted into (10-bit destinations are not implemented)");
    }
    for (int i = 0; i < n_frames; ++i)                               // (the UV plane's row: (width + 1) / 2 byte pairs)
        if (SDM_FRAME_BASE(frames[i].format) == SDM_FRAME_NV12 && (long long)frames[i].stride_bytes < 2LL * ((frames[i].width + 1) / 2))
            return fail(SDM_ERR_INVALID, "frame " + std::to_string(i) + ": stride_bytes < 2 * ((width + 1) / 2) of an NV12 frame");
    long long D;
    for (int i = 0; i < n_frames; ++i)                               // (a planar frame's second plane: not on the first)
        if (frame_planar(frames[i].format) && (rc = frame_plane_distance(i, frames[i], dst_chroma ? dst_chroma[i] : nullptr, D))) return rc;
    return SDM_OK;
}

// the fit forms' row -> frame map: every current row's image, which must be among the frames and of its frame's size
int paste_frames_of_rows(const sdm_ctx* c, const sdm_frame* frames, int n_frames, std::vector<int>& frame_of_row)
{
    frame_of_row.resize((size_t)c->N);
    for (int r = 0; r < c->N; ++r) {
        const int im = c->idx_identity ? r : c->img_idx_host[r];
        if (im < 0 || im >= n_frames) return fail(SDM_ERR_INVALID, "row " + std::to_string(r) + " maps to image " + std::to_string(im) + ", beyond the frames");
        if (frames[im].width != c->img_w_host[im] || frames[im].height != c->img_h_host[im])
            return fail(SDM_ERR_INVALID, "frame " + std::to_string(im) + " differs in size from image " + std::to_string(im) + " of the context");
        frame_of_row[r] = im;
    }
    return SDM_OK;
}

// the _at forms' row -> frame map: image_index (null: row r pastes into frame r), every entry among the frames
int paste_frames_of_index(const int* image_index, int n_rows, int n_frames, std::vector<int>& frame_of_row)
{
    frame_of_row.resize((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const int im = image_index ? image_index[r] : r;
        if (im < 0 || im >= n_frames) return fail(SDM_ERR_INVALID, "row " + std::to_string(r) + " maps to frame " + std::to_string(im) + ", outside the list");
        frame_of_row[r] = im;
    }
    return SDM_OK;
}

// the device tables of a call in align.paste_tab: the frame table, the row -> frame index, the rows of every frame in ascending order,
// and every row's place among them (enqueued; nothing waits: `blob`, the host side of the copy, lives until the call's synchronise);
// for the NV12 calls the frames' UV planes behind them, 8-byte aligned -- an array of its own; a planar frame's plane distance (from
// its dst_chroma entry, the second plane, or the default) is in the frame table
struct PasteTables {
    const PasteFrameDev* frames;
    uint8_t* const* chroma;
    const int* of_row;
    const int* list;
    const int* entry;
    bool planar;                    // a planar colour frame is among the frames: the kernels' instances with that case
    bool yuv;                       // an NV12 frame with a colour description is among them: the instances that read its table row
    std::vector<unsigned char> blob;
};

int paste_tables(sdm_ctx* c, const std::vector<int>& frame_of_row, const sdm_frame* frames, int n_frames, PasteTables& out, bool nv12 = false,
                 void* const* dst_chroma = nullptr)
{
    sdm_ctx::Align& a = c->align;
    const int N = (int)frame_of_row.size();
    const size_t tab_bytes = (size_t)n_frames * sizeof(PasteFrameDev), uv_at = (tab_bytes + (size_t)3 * N * sizeof(int) + 7) / 8 * 8;
    const size_t bytes = nv12 ? uv_at + (size_t)n_frames * sizeof(uint8_t*) : tab_bytes + (size_t)3 * N * sizeof(int);
    std::vector<unsigned char>& blob = out.blob;
    blob.assign(bytes, 0);
    out.planar = false;
    out.yuv = false;
    PasteFrameDev* tab = (PasteFrameDev*)blob.data();
    int* of_row = (int*)(blob.data() + tab_bytes);
    int* list = of_row + N;
    int* entry = list + N;
    std::vector<int> count((size_t)n_frames + 1, 0);
    for (int r = 0; r < N; ++r) { of_row[r] = frame_of_row[r]; ++count[(size_t)frame_of_row[r] + 1]; }
    for (int i = 0; i < n_frames; ++i) count[(size_t)i + 1] += count[i];
    for (int i = 0; i < n_frames; ++i) {
        const sdm_frame& f = frames[i];
        PasteFrameDev& d = tab[i];
        d.p = (uint8_t*)const_cast<void*>(f.data);                 // (sdm_frame is the read-only view of the crop calls: written here)
        d.stride = f.stride_bytes; d.w = f.width; d.h = f.height; d.format = f.format;
        d.row_begin = count[i]; d.row_end = count[(size_t)i + 1]; d.pad = 0;
        d.plane = 0;
        out.planar = out.planar || frame_planar(f.format);
        out.yuv = out.yuv || (SDM_FRAME_BASE(f.format) == SDM_FRAME_NV12 && f.format != SDM_FRAME_NV12);
        if (frame_planar(f.format)) frame_plane_distance(i, f, dst_chroma ? dst_chroma[i] : nullptr, d.plane);      // (checked: not 0)
    }
    if (nv12) {
        uint8_t** uv = (uint8_t**)(blob.data() + uv_at);
        for (int i = 0; i < n_frames; ++i) {
            const sdm_frame& f = frames[i];
            uv[i] = SDM_FRAME_BASE(f.format) != SDM_FRAME_NV12 ? nullptr
                    : dst_chroma && dst_chroma[i] ? (uint8_t*)dst_chroma[i]
                                                  : (uint8_t*)const_cast<void*>(f.data) + (size_t)f.height * (size_t)f.stride_bytes;
        }
    }
    std::vector<int> fill(count.begin(), count.end() - 1);
    for (int r = 0; r < N; ++r) { const int at = fill[frame_of_row[r]]++; list[at] = r; entry[r] = at; }
    int rc;
    if ((rc = a.paste_tab.ensure(bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(a.paste_tab.p, blob.data(), bytes, hipMemcpyHostToDevice, c->stream));
    out.frames = (const PasteFrameDev*)a.paste_tab.p;
    out.of_row = (const int*)(a.paste_tab.p + tab_bytes);
    out.list = out.of_row + N; out.entry = out.of_row + 2 * N;
    out.chroma = nv12 ? (uint8_t* const*)(a.paste_tab.p + uv_at) : nullptr;
    return SDM_OK;
}

// the tensor and the opacity maps of a call as the pixel code reads them
PasteCropDev paste_crop_dev(const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste, int cw, int ch)
{
    PasteCropDev crop{};
    crop.in = in_dev; crop.alpha = paste->alpha_dev;
    crop.cw = cw; crop.ch = ch; crop.dtype = spec->dtype; crop.channels = spec->channels;
    paste_crop_layout(crop, spec->layout, paste->alpha_per_row != 0);
    crop.t = align_tensor_dev(spec);
    return crop;
}

// behind the checks: `faces` holds N records with M (fitted: and the fit's flags).  frame_of_row: N checked indices.  filter: null --
// the unfiltered calls --, or the checked filter of the filtered ones: their prepare stage and their kernel, S behind the records.
// nv12: the calls that take NV12 destinations -- the same prepare stages, then paste_kernel_t<true, ...> with the UV planes (dst_chroma:
// the caller's, or null); without a filter their S is 1 for every row
int paste_run(sdm_ctx* c, bool fitted, const std::vector<int>& frame_of_row, int cw, int ch, const sdm_align_tensor* spec, const void* in_dev,
              const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, float* matrices_host, int* flags_host,
              const sdm_align_filter* filter, int* samples_host, bool nv12 = false, void* const* dst_chroma = nullptr)
{
    sdm_ctx::Align& a = c->align;
    const int N = (int)frame_of_row.size();
    int rc;
    PasteTables tab;
    const size_t rows_bytes = (size_t)N * sizeof(PasteRow);
    if ((rc = a.paste_rows.ensure(rows_bytes + (filter ? (size_t)N * sizeof(PasteAreaRow) : 0))) ||
        (rc = paste_tables(c, frame_of_row, frames, n_frames, tab, nv12, dst_chroma)))
        return rc;
    PasteRow* rows_dev = (PasteRow*)a.paste_rows.p;
    const PasteCropDev crop = paste_crop_dev(spec, in_dev, paste, cw, ch);
    PasteAreaRow* area_dev = filter ? (PasteAreaRow*)(a.paste_rows.p + rows_bytes) : nullptr;
    if (!filter)
        sdm_launch_paste_prepare(a.faces.p, tab.of_row, tab.frames, N, cw, ch, fitted, rows_dev, c->stream);
    else
        sdm_launch_paste_area_prepare(a.faces.p, tab.of_row, tab.frames, N, cw, ch, fitted, align_area_dev(filter), rows_dev, area_dev,
                                      (int*)(a.faces.p + N), c->stream);
    HIP_TRY(hipGetLastError());
    sdm_launch_paste(tab.frames, tab.chroma, rows_dev, area_dev, tab.list, tab.entry, N, crop, tab.planar, tab.yuv, c->stream);   // (tab.chroma: null unless nv12)
    HIP_TRY(hipGetLastError());
    if (samples_host && !filter) {                                                      // (an NV12 call without a filter: plain bilinear)
        for (int r = 0; r < N; ++r) samples_host[r] = 1;
        samples_host = nullptr;
    }
    return align_fetch_rows(c, N, matrices_host, flags_host, samples_host);
}

// The piecewise-affine paste behind its checks.  x: N x 2L on the device (the landmark state, or the uploaded points in its layout);
// src, img_idx: what warp_fit_kernel takes for its own record (the prepare kernel takes FOLDED from it and evaluates PARTIAL against the destination frames).
// nv12: the calls that take NV12 destinations -- the same two kernels, then warp_paste_kernel_t<true, false> with the UV planes (dst_chroma: the caller's, or null).
// filter: null -- the unfiltered calls --, or the checked filter of the filtered ones (nv12 is true for them): the counts stage behind the
// prepare kernel, then warp_paste_kernel_t<true, true>; the N x T x 2 counts stand directly behind the rows' records,
// so that they come back in the flags' copy, and the packed counts behind the triangle records
int warp_paste_run(sdm_ctx* c, const float* x, const AlignSourceDev& src, const int* img_idx, const std::vector<int>& frame_of_row,
                   const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames, int n_frames,
                   float* matrices_host, int* flags_host, bool nv12, void* const* dst_chroma, const sdm_align_filter* filter = nullptr,
                   int* samples_host = nullptr)
{
    sdm_ctx::Warp& w = c->warp;
    const int N = (int)frame_of_row.size(), T = w.T;
    int rc;
    const size_t rec = (size_t)N * sizeof(WarpFace), mat = (size_t)N * T * 6 * sizeof(float);
    const size_t rows_bytes = (size_t)N * sizeof(WarpPasteRow), tris_bytes = (size_t)N * T * sizeof(WarpPasteTri);
    const size_t samples_bytes = filter ? (size_t)N * T * 2 * sizeof(int) : 0, counts_bytes = filter ? (size_t)N * T * sizeof(uint16_t) : 0;
    PasteTables tab;
    if ((rc = w.rows.ensure(rec + mat)) || (rc = w.paste.ensure(rows_bytes + samples_bytes + tris_bytes + counts_bytes)) ||
        (rc = paste_tables(c, frame_of_row, frames, n_frames, tab, nv12, dst_chroma)))
        return rc;
    WarpFace* faces = (WarpFace*)w.rows.p;
    float* matrices = (float*)(w.rows.p + rec);
    WarpPasteRow* rows_dev = (WarpPasteRow*)w.paste.p;
    int* samples_dev = (int*)(w.paste.p + rows_bytes);
    WarpPasteTri* tris_dev = (WarpPasteTri*)(w.paste.p + rows_bytes + samples_bytes);
    uint16_t* counts_dev = filter ? (uint16_t*)(w.paste.p + rows_bytes + samples_bytes + tris_bytes) : nullptr;
    sdm_launch_warp_fit(x, N, w.L, w.lm.p, w.K, (const WarpTri*)w.tri.p, T, src, img_idx, faces, matrices, c->stream);
    HIP_TRY(hipGetLastError());
    sdm_launch_warp_paste_prepare(x, N, w.L, w.lm.p, w.K, (const WarpTri*)w.tri.p, T, faces, matrices, tab.of_row, tab.frames, rows_dev,
                                  tris_dev, c->stream);
    HIP_TRY(hipGetLastError());
    const PasteCropDev crop = paste_crop_dev(spec, in_dev, paste, w.out_w, w.out_h);
    if (filter) {
        sdm_launch_warp_paste_area_counts(rows_dev, tris_dev, N, T, align_area_dev(filter), counts_dev, samples_dev, c->stream);
        HIP_TRY(hipGetLastError());
    }
    sdm_launch_warp_paste(tab.frames, tab.chroma, rows_dev, tris_dev, counts_dev, T, tab.list, tab.entry, N, w.labels.p, crop, tab.planar, tab.yuv, c->stream);   // (tab.chroma: null unless nv12)
    HIP_TRY(hipGetLastError());
    // the matrices and the rows' records (a filtered call: with the counts behind them, in the same copy), one synchronise
    if (!filter) samples_host = nullptr;
    std::vector<unsigned char> host;
    if (matrices_host) HIP_TRY(hipMemcpyAsync(matrices_host, matrices, mat, hipMemcpyDeviceToHost, c->stream));
    if (flags_host || samples_host) {
        host.resize(rows_bytes + (samples_host ? samples_bytes : 0));
        HIP_TRY(hipMemcpyAsync(host.data(), rows_dev, host.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags_host)
        for (int r = 0; r < N; ++r) flags_host[r] = ((const WarpPasteRow*)host.data())[r].flags;
    if (samples_host) memcpy(samples_host, host.data() + rows_bytes, samples_bytes);
    return SDM_OK;
}

// sdm_align_paste_tensor (filtered false) and sdm_align_paste_tensor_filtered: the same checks, the same fit, then the paste
int paste_fit_call(sdm_ctx* c, const int* lm, const float* tmpl, int K, int cw, int ch, const sdm_align_tensor* spec,
                   const sdm_align_filter* filter, bool filtered, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                   int n_frames, float* matrices_host, int* flags_host, int* samples_host, bool nv12 = false, void* const* dst_chroma = nullptr)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = align_check_call(c, lm, tmpl, K, cw, ch)) || (rc = align_check_spec(spec)) || (filtered && (rc = align_check_filter(filter))) ||
        (rc = paste_check_args(in_dev, paste, frames, n_frames, nv12, dst_chroma)) || (rc = align_check_rows(c)))
        return rc;
    std::vector<int> frame_of_row;
    if ((rc = paste_frames_of_rows(c, frames, n_frames, frame_of_row))) return rc;
    sdm_ctx::Align& a = c->align;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = a.in.ensure((size_t)3 * K)) || (rc = a.faces.ensure(align_face_records(c->N, filtered)))) return rc;
    if ((rc = align_fit_rows(c, lm, tmpl, K, cw, ch))) return rc;
    return paste_run(c, true, frame_of_row, cw, ch, spec, in_dev, paste, frames, n_frames, matrices_host, flags_host, filtered ? filter : nullptr,
                     samples_host, nv12, dst_chroma);
}

// sdm_align_paste_tensor_at (filtered false) and sdm_align_paste_tensor_at_filtered
int paste_at_call(sdm_ctx* c, const float* matrices_host, const int* image_index, int n_rows, int cw, int ch, const sdm_align_tensor* spec,
                  const sdm_align_filter* filter, bool filtered, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                  int n_frames, int* flags_host, int* samples_host, bool nv12 = false, void* const* dst_chroma = nullptr)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    if (!matrices_host) return fail(SDM_ERR_INVALID, "no matrices");
    if (n_rows < 1) return fail(SDM_ERR_INVALID, "n_rows must be >= 1");
    if (cw < 1 || cw > 1024 || ch < 1 || ch > 1024) return fail(SDM_ERR_INVALID, "crop width and height must be in [1, 1024]");
    int rc;
    if ((rc = align_check_spec(spec)) || (filtered && (rc = align_check_filter(filter))) ||
        (rc = paste_check_args(in_dev, paste, frames, n_frames, nv12, dst_chroma)))
        return rc;
    std::vector<int> frame_of_row;
    if ((rc = paste_frames_of_index(image_index, n_rows, n_frames, frame_of_row))) return rc;
    std::vector<AlignFace> faces((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const sdm_frame& fr = frames[frame_of_row[r]];
        AlignFace& f = faces[r];
        memcpy(f.m, matrices_host + (size_t)6 * r, 6 * sizeof(float));
        f.flags = 0; f.w = fr.width; f.h = fr.height; f.stride = fr.stride_bytes; f.off = 0;
    }
    sdm_ctx::Align& a = c->align;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = a.faces.ensure(align_face_records(n_rows, filtered)))) return rc;
    HIP_TRY(hipMemcpyAsync(a.faces.p, faces.data(), faces.size() * sizeof(AlignFace), hipMemcpyHostToDevice, c->stream));
    return paste_run(c, false, frame_of_row, cw, ch, spec, in_dev, paste, frames, n_frames, nullptr, flags_host, filtered ? filter : nullptr,
                     samples_host, nv12, dst_chroma);
}

int warp_paste_check_mesh(sdm_ctx* c)
{
    if (c->L <= 0) return fail(SDM_ERR_INVALID, "geometry not set");
    if (c->warp.T < 1 || c->warp.L != c->L) return fail(SDM_ERR_INVALID, "no mesh (sdm_warp_set_mesh first)");
    return SDM_OK;
}

// sdm_warp_paste_tensor and sdm_warp_paste_tensor_nv12: the same checks in the same order
int warp_paste_fit_call(sdm_ctx* c, const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                        int n_frames, float* matrices_host, int* flags_host, bool nv12, void* const* dst_chroma, bool filtered = false,
                        const sdm_align_filter* filter = nullptr, int* samples_host = nullptr)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = warp_paste_check_mesh(c))) return rc;
    if (c->N < 1) return fail(SDM_ERR_INVALID, "no current rows (sdm_set_x, sdm_detect_batch or sdm_track_step first)");
    if ((rc = align_check_spec(spec)) || (filtered && (rc = align_check_filter(filter))) ||
        (rc = paste_check_args(in_dev, paste, frames, n_frames, nv12, dst_chroma)) || (rc = align_check_rows(c)))
        return rc;
    std::vector<int> frame_of_row;
    if ((rc = paste_frames_of_rows(c, frames, n_frames, frame_of_row))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return warp_paste_run(c, c->x[c->cur].p, align_source_dev(c), c->idx_identity ? nullptr : c->img_idx.p, frame_of_row, spec, in_dev, paste,
                          frames, n_frames, matrices_host, flags_host, nv12, dst_chroma, filtered ? filter : nullptr, samples_host);
}

// sdm_warp_paste_tensor_at and sdm_warp_paste_tensor_at_nv12
int warp_paste_at_call(sdm_ctx* c, const float* points_host, const int* image_index, int n_rows, const sdm_align_tensor* spec, const void* in_dev,
                       const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, int* flags_host, bool nv12, void* const* dst_chroma,
                       bool filtered = false, const sdm_align_filter* filter = nullptr, int* samples_host = nullptr)
{
    if (!c) return fail(SDM_ERR_INVALID, "null context");
    int rc;
    if ((rc = warp_paste_check_mesh(c))) return rc;
    if (!points_host) return fail(SDM_ERR_INVALID, "no points");
    if (n_rows < 1) return fail(SDM_ERR_INVALID, "n_rows must be >= 1");
    if ((rc = align_check_spec(spec)) || (filtered && (rc = align_check_filter(filter))) ||
        (rc = paste_check_args(in_dev, paste, frames, n_frames, nv12, dst_chroma)))
        return rc;
    std::vector<int> frame_of_row;
    if ((rc = paste_frames_of_index(image_index, n_rows, n_frames, frame_of_row))) return rc;
    sdm_ctx::Warp& w = c->warp;
    const int L = w.L, K = w.K;
    // the points in the landmark state's layout (row: L x then L y), the mesh's landmarks at their indices, 0 elsewhere: the fit and the
    // prepare kernel read them as they read the state
    std::vector<float> x((size_t)n_rows * 2 * L, 0.0f);
    for (int r = 0; r < n_rows; ++r)
        for (int k = 0; k < K; ++k) {
            x[(size_t)r * 2 * L + w.lm_host[k]] = points_host[((size_t)r * K + k) * 2];
            x[(size_t)r * 2 * L + L + w.lm_host[k]] = points_host[((size_t)r * K + k) * 2 + 1];
        }
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = w.points.ensure(x.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(w.points.p, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    // warp_fit_kernel's own record wants an image per row: a stack of one 1 x 1 image (of its flags only FOLDED is read)
    AlignSourceDev src{};
    src.width = src.height = src.stride = 1;
    return warp_paste_run(c, w.points.p, src, nullptr, frame_of_row, spec, in_dev, paste, frames, n_frames, nullptr, flags_host, nv12, dst_chroma,
                          filtered ? filter : nullptr, samples_host);
}

}  // namespace

extern "C" {

int sdm_warp_paste_tensor(sdm_ctx* c, const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                          int n_frames, float* matrices_host, int* flags_host)
{
    return warp_paste_fit_call(c, spec, in_dev, paste, frames, n_frames, matrices_host, flags_host, false, nullptr);
}

int sdm_warp_paste_tensor_at(sdm_ctx* c, const float* points_host, const int* image_index, int n_rows, const sdm_align_tensor* spec,
                             const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, int* flags_host)
{
    return warp_paste_at_call(c, points_host, image_index, n_rows, spec, in_dev, paste, frames, n_frames, flags_host, false, nullptr);
}

// the calls that take NV12 destinations
int sdm_warp_paste_tensor_nv12(sdm_ctx* c, const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste,
                               const sdm_frame* frames, void* const* dst_chroma, int n_frames, float* matrices_host, int* flags_host)
{
    return warp_paste_fit_call(c, spec, in_dev, paste, frames, n_frames, matrices_host, flags_host, true, dst_chroma);
}

int sdm_warp_paste_tensor_at_nv12(sdm_ctx* c, const float* points_host, const int* image_index, int n_rows, const sdm_align_tensor* spec,
                                  const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames, void* const* dst_chroma,
                                  int n_frames, int* flags_host)
{
    return warp_paste_at_call(c, points_host, image_index, n_rows, spec, in_dev, paste, frames, n_frames, flags_host, true, dst_chroma);
}

// the filtered calls: a list that may mix NV12 and the per-pixel formats
int sdm_warp_paste_tensor_filtered(sdm_ctx* c, const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                   const sdm_align_paste* paste, const sdm_frame* frames, void* const* dst_chroma, int n_frames,
                                   float* matrices_host, int* flags_host, int* samples_host)
{
    return warp_paste_fit_call(c, spec, in_dev, paste, frames, n_frames, matrices_host, flags_host, true, dst_chroma, true, filter, samples_host);
}

int sdm_warp_paste_tensor_at_filtered(sdm_ctx* c, const float* points_host, const int* image_index, int n_rows, const sdm_align_tensor* spec,
                                      const sdm_align_filter* filter, const void* in_dev, const sdm_align_paste* paste,
                                      const sdm_frame* frames, void* const* dst_chroma, int n_frames, int* flags_host, int* samples_host)
{
    return warp_paste_at_call(c, points_host, image_index, n_rows, spec, in_dev, paste, frames, n_frames, flags_host, true, dst_chroma, true, filter,
                              samples_host);
}

int sdm_align_paste_tensor(sdm_ctx* c, const int* lm, const float* tmpl, int K, int cw, int ch, const sdm_align_tensor* spec,
                           const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, float* matrices_host,
                           int* flags_host)
{
    return paste_fit_call(c, lm, tmpl, K, cw, ch, spec, nullptr, false, in_dev, paste, frames, n_frames, matrices_host, flags_host, nullptr);
}

int sdm_align_paste_tensor_at(sdm_ctx* c, const float* matrices_host, const int* image_index, int n_rows, int cw, int ch,
                              const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                              int n_frames, int* flags_host)
{
    return paste_at_call(c, matrices_host, image_index, n_rows, cw, ch, spec, nullptr, false, in_dev, paste, frames, n_frames, flags_host, nullptr);
}

int sdm_align_paste_tensor_filtered(sdm_ctx* c, const int* lm, const float* tmpl, int K, int cw, int ch, const sdm_align_tensor* spec,
                                    const sdm_align_filter* filter, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                                    int n_frames, float* matrices_host, int* flags_host, int* samples_host)
{
    return paste_fit_call(c, lm, tmpl, K, cw, ch, spec, filter, true, in_dev, paste, frames, n_frames, matrices_host, flags_host, samples_host);
}

int sdm_align_paste_tensor_at_filtered(sdm_ctx* c, const float* matrices_host, const int* image_index, int n_rows, int cw, int ch,
                                       const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                       const sdm_align_paste* paste, const sdm_frame* frames, int n_frames, int* flags_host, int* samples_host)
{
    return paste_at_call(c, matrices_host, image_index, n_rows, cw, ch, spec, filter, true, in_dev, paste, frames, n_frames, flags_host,
                         samples_host);
}

// the calls that take NV12 destinations: filter NULL is plain bilinear
int sdm_align_paste_tensor_nv12(sdm_ctx* c, const int* lm, const float* tmpl, int K, int cw, int ch, const sdm_align_tensor* spec,
                                const sdm_align_filter* filter, const void* in_dev, const sdm_align_paste* paste, const sdm_frame* frames,
                                void* const* dst_chroma, int n_frames, float* matrices_host, int* flags_host, int* samples_host)
{
    return paste_fit_call(c, lm, tmpl, K, cw, ch, spec, filter, filter != nullptr, in_dev, paste, frames, n_frames, matrices_host, flags_host,
                          samples_host, true, dst_chroma);
}

int sdm_align_paste_tensor_at_nv12(sdm_ctx* c, const float* matrices_host, const int* image_index, int n_rows, int cw, int ch,
                                   const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                   const sdm_align_paste* paste, const sdm_frame* frames, void* const* dst_chroma, int n_frames,
                                   int* flags_host, int* samples_host)
{
    return paste_at_call(c, matrices_host, image_index, n_rows, cw, ch, spec, filter, filter != nullptr, in_dev, paste, frames, n_frames,
                         flags_host, samples_host, true, dst_chroma);
}

}  // extern "C"
