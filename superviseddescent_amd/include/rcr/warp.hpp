// rcr/warp.hpp -- piecewise-affine warped faces from landmarks kept on the device (include/sdm.h, "Warped faces", sdm_warp_*): the
// template is triangulated over the landmarks and every triangle is mapped by its own affine transform, so every landmark lands on its
// template point -- the shape-normalised texture that expression, action-unit, liveness and face-swap networks take as input --
// without copying the landmarks or the frames to the host for an image library.
//
//     rcr::tracker tr(model, 64);
//     auto lms = tr.step(ids, frames);
//     rcr::WarpMesh mesh = rcr::WarpMesh::of_mean(model.get_mean(), idx, 112, 112);      // default template, Delaunay triangles
//     auto w = rcr::warped_crops_tensor(tr, mesh, rcr::TensorSpec(), out_dev, device_frames);
//     // out_dev: rows x 3 x 112 x 112 float16; w.matrices.row(i): stream ids[i]'s T crop -> source maps; w.flags[i]: SDM_WARP_*
//
// The rows of detection_model::detect_batch work the same way (the overload taking the frames and the rows).
//
// With an rcr::AlignFilter behind the spec the texture is area-averaged where a triangle minifies (w.samples: Sx, Sy of every triangle):
//
//     auto w = rcr::warped_crops_tensor(tr, mesh, rcr::TensorSpec(), rcr::AlignFilter(), out_dev, device_frames);
//
// rcr::paste_warped_tensor is the way back: a network's output in template space blended into the frames under every face's own shape.
//
//     auto p = rcr::paste_warped_tensor(tr, mesh, paste_spec, net_out_dev, device_frames);       // p.flags[i]: SDM_WARP_*
//     auto q = rcr::paste_warped_tensor(tr, mesh, paste_spec, net_out_dev, nv12_frames, std::vector<void*>());   // NV12, UV behind Y
//     std::vector<int> samples;                                                                  // rows x T x 2: (Sx, Sy) of every triangle
//     auto a = rcr::paste_warped_tensor(tr, mesh, paste_spec, rcr::AlignFilter(), net_out_dev, frames, {}, rcr::PasteMask{}, &samples);
#pragma once

#ifndef RCR_WARP_HPP_
#define RCR_WARP_HPP_

#include "rcr/alignment.hpp"

#include <stdexcept>
#include <vector>

namespace rcr {

/** The Delaunay triangulation of K x 2 CV_32FC1 points (sdm_warp_delaunay; host code): triples of point positions, counter-clockwise in
 *  the header's sense, the same for the same input. */
inline std::vector<int> delaunay(cv::Mat points)
{
    if (points.cols != 2 || points.type() != CV_32FC1) throw std::runtime_error("delaunay: K x 2 CV_32FC1 points expected");
    cv::Mat p = points.isContinuous() ? points : points.clone();
    std::vector<int> tri((size_t)6 * std::max(p.rows, 1));
    int n = 0;
    superviseddescent::hip::check(sdm_warp_delaunay(p.ptr<float>(0), p.rows, tri.data(), 2 * std::max(p.rows, 1), &n), "sdm_warp_delaunay");
    tri.resize((size_t)3 * n);
    return tri;
}

/** The mesh of a warp: K landmark indices, their template points (K x 2 CV_32FC1, crop pixels), triangles over the positions
 *  0 .. K - 1 (three ints each, at most 254 triangles) and the crop size. */
struct WarpMesh {
    std::vector<int> landmark_index;
    cv::Mat tmpl;
    std::vector<int> triangles;
    int width = 0, height = 0;

    int n_triangles() const { return (int)triangles.size() / 3; }

    /** template given, triangles = its Delaunay triangulation (or a list of one's own, e.g. one that leaves the mouth's interior out) */
    static WarpMesh of_template(const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height, const std::vector<int>& triangles = {})
    {
        WarpMesh m;
        m.landmark_index = landmark_index;
        m.tmpl = tmpl.isContinuous() ? tmpl : tmpl.clone();
        m.triangles = triangles.empty() ? delaunay(m.tmpl) : triangles;
        m.width = width; m.height = height;
        return m;
    }
    /** the default: alignment_template of the mean with `margin`, Delaunay triangles */
    static WarpMesh of_mean(cv::Mat mean, const std::vector<int>& landmark_index, int width, int height, double margin = 0.1)
    {
        return of_template(landmark_index, alignment_template(mean, landmark_index, width, height, margin), width, height);
    }
};

struct warped_tensor_result {
    cv::Mat matrices;              // rows x (6 T) CV_32FC1: per row the T crop -> source maps M00 M01 M02 M10 M11 M12 (NaN for a degenerate row)
    std::vector<int> flags;        // SDM_WARP_DEGENERATE / SDM_WARP_PARTIAL / SDM_WARP_FOLDED bits
    cv::Mat labels;                // height x width CV_8UC1: the triangle of every crop pixel, SDM_WARP_NO_TRIANGLE = none
    std::vector<int> samples;      // the overloads taking an AlignFilter: rows x T x 2, (Sx, Sy) of every triangle; empty otherwise
};

namespace detail {

// the n current rows of the handle `c` warped onto the mesh's template, as a tensor in device memory, from `frames` in place or -- no
// frames -- from the handle's own images; `filter`: nullptr, or the sampling of sdm_warp_crops_tensor_filtered
inline warped_tensor_result warp_tensor_current_rows(sdm_ctx* c, int n, const WarpMesh& mesh, const std::vector<DeviceFrame>& frames,
                                                     const std::vector<const void*>& chroma, const TensorSpec& spec, void* out_dev,
                                                     const AlignFilter* filter = nullptr)
{
    using superviseddescent::hip::check;
    if (mesh.tmpl.rows != (int)mesh.landmark_index.size() || mesh.tmpl.cols != 2 || mesh.tmpl.type() != CV_32FC1)
        throw std::runtime_error("warped_crops_tensor: one template point (x, y) per landmark");
    if (mesh.triangles.size() % 3 != 0) throw std::runtime_error("warped_crops_tensor: three positions per triangle");
    if (!chroma.empty() && chroma.size() != frames.size()) throw std::runtime_error("warped_crops_tensor: one chroma pointer (or nullptr) per frame");
    cv::Mat t = mesh.tmpl.isContinuous() ? mesh.tmpl : mesh.tmpl.clone();
    check(sdm_warp_set_mesh(c, mesh.landmark_index.data(), t.ptr<float>(0), (int)mesh.landmark_index.size(), mesh.triangles.data(),
                            mesh.n_triangles(), mesh.width, mesh.height), "sdm_warp_set_mesh");
    std::vector<sdm_frame> f;
    for (const auto& d : frames) f.push_back(sdm_frame{d.data, d.width, d.height, d.stride_bytes, d.format});
    const SecondPlanes<const void*> planes(frames, &chroma);                  // (a frame's own second_plane where chroma names none)
    check(sdm_align_set_source_frames(c, f.empty() ? nullptr : f.data(), planes.data(), (int)f.size()),
          "sdm_align_set_source_frames");
    sdm_align_tensor s{};
    s.dtype = spec.dtype; s.layout = spec.layout; s.channels = spec.channels; s.order = spec.order; s.gray_shift = spec.gray_shift;
    for (int k = 0; k < 3; ++k) { s.scale[k] = spec.scale[k]; s.bias[k] = spec.bias[k]; }
    warped_tensor_result res;
    res.matrices = cv::Mat(n, 6 * mesh.n_triangles(), CV_32FC1);
    res.flags.resize((size_t)n);
    int rc;
    if (filter) {
        const sdm_align_filter fl{filter->mode, filter->max_samples, filter->min_scale};
        res.samples.resize((size_t)n * mesh.n_triangles() * 2);
        rc = sdm_warp_crops_tensor_filtered(c, &s, &fl, out_dev, res.matrices.ptr<float>(0), res.flags.data(), res.samples.data());
    } else {
        rc = sdm_warp_crops_tensor(c, &s, out_dev, res.matrices.ptr<float>(0), res.flags.data());
    }
    if (!frames.empty()) sdm_align_set_source_frames(c, nullptr, nullptr, 0);     // (no pointer to the caller's frames stays behind)
    check(rc, filter ? "sdm_warp_crops_tensor_filtered" : "sdm_warp_crops_tensor");
    res.labels = cv::Mat(mesh.height, mesh.width, CV_8UC1);
    check(sdm_warp_get_labels(c, res.labels.ptr<uint8_t>(0)), "sdm_warp_get_labels");
    return res;
}

// landmark rows on device frames: a handle of its own, the frames as its image set, the rows uploaded
inline warped_tensor_result warp_tensor_rows(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                             const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec, void* out_dev,
                                             const std::vector<const void*>& chroma, const AlignFilter* filter)
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::set_device_frames(h, frames);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("warped_crops_tensor: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::warp_tensor_current_rows(c, x.rows, mesh, frames, chroma, spec, out_dev, filter);
}

}  // namespace detail

/** The streams of the tracker's last step warped onto the mesh's template, written to `out_dev` (device memory, rows * channels *
 *  height * width elements of spec.dtype, 16-byte aligned): two launches from `frames` where they lie on the device -- the frames of
 *  that step, any of the six formats, same sizes, same order -- or, `frames` empty, from the step's gray images. */
inline warped_tensor_result warped_crops_tensor(tracker& tr, const WarpMesh& mesh, const TensorSpec& spec, void* out_dev,
                                                const std::vector<DeviceFrame>& frames = {}, const std::vector<const void*>& chroma = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("warped_crops_tensor: step the tracker first");
    return detail::warp_tensor_current_rows(tr.context(), tr.rows().rows, mesh, frames, chroma, spec, out_dev);
}

/** The same for landmark rows on device frames, e.g. the result of detection_model::detect_batch(frames, boxes, image_index): row i is
 *  warped from frames[image_index[i]] (default: frames[i]).  As aligned_crops_tensor's overload of this shape, it works on a handle
 *  of its own: the frames become its image set and the rows are uploaded. */
inline warped_tensor_result warped_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                                const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec, void* out_dev,
                                                const std::vector<const void*>& chroma = {})
{
    return detail::warp_tensor_rows(model, frames, rows, image_index, mesh, spec, out_dev, chroma, nullptr);
}

/** The two forms with area-averaged sampling (include/sdm.h, "Warped faces, filtered"; rcr::AlignFilter of rcr/alignment.hpp): every pixel
 *  of a triangle whose map minifies is the average of Sx x Sy bilinear sub-samples of its footprint, the counts chosen per triangle and
 *  per axis; triangles at (1, 1) get the bits of the forms above.  The result's `samples` holds rows x T x 2 counts. */
inline warped_tensor_result warped_crops_tensor(tracker& tr, const WarpMesh& mesh, const TensorSpec& spec, const AlignFilter& filter, void* out_dev,
                                                const std::vector<DeviceFrame>& frames = {}, const std::vector<const void*>& chroma = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("warped_crops_tensor: step the tracker first");
    return detail::warp_tensor_current_rows(tr.context(), tr.rows().rows, mesh, frames, chroma, spec, out_dev, &filter);
}

inline warped_tensor_result warped_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                                const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec,
                                                const AlignFilter& filter, void* out_dev, const std::vector<const void*>& chroma = {})
{
    return detail::warp_tensor_rows(model, frames, rows, image_index, mesh, spec, out_dev, chroma, &filter);
}

struct warp_paste_result {
    cv::Mat matrices;              // rows x (6 T) CV_32FC1: the crop -> frame maps, as warped_crops_tensor returns them (empty: the form with points)
    std::vector<int> flags;        // SDM_WARP_DEGENERATE / SDM_WARP_PARTIAL / SDM_WARP_FOLDED bits
};

namespace detail {

inline void warp_paste_set_mesh(sdm_ctx* c, const WarpMesh& mesh)
{
    if (mesh.tmpl.rows != (int)mesh.landmark_index.size() || mesh.tmpl.cols != 2 || mesh.tmpl.type() != CV_32FC1)
        throw std::runtime_error("paste_warped_tensor: one template point (x, y) per landmark");
    if (mesh.triangles.size() % 3 != 0) throw std::runtime_error("paste_warped_tensor: three positions per triangle");
    cv::Mat t = mesh.tmpl.isContinuous() ? mesh.tmpl : mesh.tmpl.clone();
    superviseddescent::hip::check(sdm_warp_set_mesh(c, mesh.landmark_index.data(), t.ptr<float>(0), (int)mesh.landmark_index.size(),
                                                    mesh.triangles.data(), mesh.n_triangles(), mesh.width, mesh.height), "sdm_warp_set_mesh");
}

// the n current rows of the handle `c`: the fit of warped_crops_tensor, then the tensor at `in_dev` pasted into `frames` in place;
// `chroma`: nullptr, or -- the overloads for NV12 destinations, sdm_warp_paste_tensor_nv12 -- the frames' UV planes (empty: every one
// directly behind its Y plane); `filter`: nullptr, or -- the overloads taking an AlignFilter, sdm_warp_paste_tensor_filtered -- the
// sampling, with `samples` (may be nullptr) taking rows x T x 2 counts
inline warp_paste_result warp_paste_current_rows(sdm_ctx* c, int n, const WarpMesh& mesh, const TensorSpec& spec, const void* in_dev,
                                                 const std::vector<DeviceFrame>& frames, const PasteMask& mask,
                                                 const std::vector<void*>* chroma = nullptr, const AlignFilter* filter = nullptr,
                                                 std::vector<int>* samples = nullptr)
{
    warp_paste_set_mesh(c, mesh);
    const std::vector<sdm_frame> f = paste_frames(frames);
    if (chroma) paste_chroma(*chroma, f.size());                                // (its size check)
    const SecondPlanes<void*> planes(frames, chroma);                           // (a frame's own second_plane where chroma names none)
    const sdm_align_tensor s = paste_spec(spec);
    const sdm_align_paste p{mask.alpha_dev, mask.per_row ? 1 : 0};
    warp_paste_result res;
    res.matrices = cv::Mat(n, 6 * mesh.n_triangles(), CV_32FC1);
    res.flags.resize((size_t)n);
    if (filter) {
        const sdm_align_filter fl{filter->mode, filter->max_samples, filter->min_scale};
        if (samples) samples->assign((size_t)n * mesh.n_triangles() * 2, 0);
        superviseddescent::hip::check(sdm_warp_paste_tensor_filtered(c, &s, &fl, in_dev, &p, f.empty() ? nullptr : f.data(),
                                                                     planes.data(), (int)f.size(),
                                                                     res.matrices.ptr<float>(0), res.flags.data(),
                                                                     samples ? samples->data() : nullptr),
                                      "sdm_warp_paste_tensor_filtered");
        return res;
    }
    if (chroma || planes.any) {
        superviseddescent::hip::check(sdm_warp_paste_tensor_nv12(c, &s, in_dev, &p, f.empty() ? nullptr : f.data(), planes.data(),
                                                                 (int)f.size(), res.matrices.ptr<float>(0), res.flags.data()),
                                      "sdm_warp_paste_tensor_nv12");
        return res;
    }
    superviseddescent::hip::check(sdm_warp_paste_tensor(c, &s, in_dev, &p, f.empty() ? nullptr : f.data(), (int)f.size(),
                                                        res.matrices.ptr<float>(0), res.flags.data()), "sdm_warp_paste_tensor");
    return res;
}

// landmark rows on device frames: a handle of its own, the frames as its image set, the rows uploaded.  chroma: as above
inline warp_paste_result warp_paste_rows(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                         const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec, const void* in_dev,
                                         const PasteMask& mask, const std::vector<void*>* chroma, const AlignFilter* filter = nullptr,
                                         std::vector<int>* samples = nullptr)
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::set_device_frames(h, frames);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("paste_warped_tensor: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::warp_paste_current_rows(c, x.rows, mesh, spec, in_dev, frames, mask, chroma, filter, samples);
}

// explicit points: sdm_warp_paste_tensor_at, or with chroma sdm_warp_paste_tensor_at_nv12
inline warp_paste_result warp_paste_points(detection_model& model, cv::Mat points, const std::vector<int>& image_index, const WarpMesh& mesh,
                                           const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                           const PasteMask& mask, const std::vector<void*>* chroma, const AlignFilter* filter = nullptr,
                                           std::vector<int>* samples = nullptr)
{
    using superviseddescent::hip::check;
    if (points.type() != CV_32FC1 || points.cols != 2 * (int)mesh.landmark_index.size() || points.rows < 1)
        throw std::runtime_error("paste_warped_tensor: points must be rows x 2K CV_32FC1");
    if (!image_index.empty() && (int)image_index.size() != points.rows) throw std::runtime_error("paste_warped_tensor: one image index per row");
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::warp_paste_set_mesh(h.get(), mesh);
    cv::Mat pts = points.isContinuous() ? points : points.clone();
    const std::vector<sdm_frame> f = detail::paste_frames(frames);
    if (chroma) detail::paste_chroma(*chroma, f.size());                        // (its size check)
    const detail::SecondPlanes<void*> planes(frames, chroma);                   // (a frame's own second_plane where chroma names none)
    const sdm_align_tensor s = detail::paste_spec(spec);
    const sdm_align_paste p{mask.alpha_dev, mask.per_row ? 1 : 0};
    warp_paste_result res;
    res.flags.resize((size_t)points.rows);
    const int* index = image_index.empty() ? nullptr : image_index.data();
    if (filter) {
        const sdm_align_filter fl{filter->mode, filter->max_samples, filter->min_scale};
        if (samples) samples->assign((size_t)points.rows * mesh.n_triangles() * 2, 0);
        check(sdm_warp_paste_tensor_at_filtered(h.get(), pts.ptr<float>(0), index, points.rows, &s, &fl, in_dev, &p, f.empty() ? nullptr : f.data(),
                                                planes.data(), (int)f.size(), res.flags.data(),
                                                samples ? samples->data() : nullptr),
              "sdm_warp_paste_tensor_at_filtered");
    } else if (chroma || planes.any)
        check(sdm_warp_paste_tensor_at_nv12(h.get(), pts.ptr<float>(0), index, points.rows, &s, in_dev, &p, f.empty() ? nullptr : f.data(),
                                            planes.data(), (int)f.size(), res.flags.data()),
              "sdm_warp_paste_tensor_at_nv12");
    else
        check(sdm_warp_paste_tensor_at(h.get(), pts.ptr<float>(0), index, points.rows, &s, in_dev, &p, f.empty() ? nullptr : f.data(),
                                       (int)f.size(), res.flags.data()), "sdm_warp_paste_tensor_at");
    return res;
}

}  // namespace detail

/** The way back of warped_crops_tensor: `in_dev` -- a network's output in template space on the streams of the tracker's last step,
 *  rows * channels * height * width elements of spec.dtype in spec.layout, 16-byte aligned device memory -- is warped back under every
 *  face's own shape, triangle by triangle, and blended into `frames` IN PLACE (the frames of that step, GRAY / BGR / RGB / BGRA / RGBA;
 *  NV12 is refused) (include/sdm.h, "Pasting warped faces back").  spec and mask: as for paste_crops_tensor; a tap outside the mesh's
 *  hull has opacity 0 whatever the mask says. */
inline warp_paste_result paste_warped_tensor(tracker& tr, const WarpMesh& mesh, const TensorSpec& spec, const void* in_dev,
                                             const std::vector<DeviceFrame>& frames, const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_warped_tensor: step the tracker first");
    return detail::warp_paste_current_rows(tr.context(), tr.rows().rows, mesh, spec, in_dev, frames, mask);
}

/** The same for landmark rows on device frames (as the detection_model overload of warped_crops_tensor: a handle of its own, the frames
 *  as its image set, the rows uploaded): row i is pasted into frames[image_index[i]] (default: frames[i]). */
inline warp_paste_result paste_warped_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                             const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec,
                                             const void* in_dev, const PasteMask& mask = {})
{
    return detail::warp_paste_rows(model, frames, rows, image_index, mesh, spec, in_dev, mask, nullptr);
}

/** The explicit form (sdm_warp_paste_tensor_at): `points` rows x 2K CV_32FC1 -- per row x, y of the mesh's first landmark, then of its
 *  second, ... -- as they were when the tensor was cut; the rows need not be current any more.  The model gives the landmark count the
 *  mesh's indices refer to; no landmark state and no image is needed.  Row i goes to frames[image_index[i]] (default: frames[i]). */
inline warp_paste_result paste_warped_tensor(detection_model& model, cv::Mat points, const std::vector<int>& image_index, const WarpMesh& mesh,
                                             const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                             const PasteMask& mask = {})
{
    return detail::warp_paste_points(model, points, image_index, mesh, spec, in_dev, frames, mask, nullptr);
}

/** The three forms for destinations that may hold NV12 frames (include/sdm.h, "Pasting warped faces back into NV12 frames"): luma and
 *  4:2:0 chroma are blended in place, the other formats get the bytes of the forms above.  `chroma`: per frame the UV plane of an NV12
 *  frame (nullptr: directly behind its Y plane); an empty vector: every UV plane lies behind its Y plane.  `chroma` stands where the
 *  forms above have their defaulted mask, so a bare `{}` in that place names neither a mask nor a chroma vector: the call is
 *  ambiguous (as for the paste_crops_tensor overloads of rcr/alignment.hpp).  Write `rcr::PasteMask{}` or `std::vector<void*>{}`. */
inline warp_paste_result paste_warped_tensor(tracker& tr, const WarpMesh& mesh, const TensorSpec& spec, const void* in_dev,
                                             const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma, const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_warped_tensor: step the tracker first");
    return detail::warp_paste_current_rows(tr.context(), tr.rows().rows, mesh, spec, in_dev, frames, mask, &chroma);
}

inline warp_paste_result paste_warped_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma,
                                             cv::Mat rows, const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec,
                                             const void* in_dev, const PasteMask& mask = {})
{
    return detail::warp_paste_rows(model, frames, rows, image_index, mesh, spec, in_dev, mask, &chroma);
}

inline warp_paste_result paste_warped_tensor(detection_model& model, cv::Mat points, const std::vector<int>& image_index, const WarpMesh& mesh,
                                             const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                             const std::vector<void*>& chroma, const PasteMask& mask = {})
{
    return detail::warp_paste_points(model, points, image_index, mesh, spec, in_dev, frames, mask, &chroma);
}

/** The three forms with area-averaged sampling (include/sdm.h, "Pasting warped faces back, filtered"; rcr::AlignFilter of
 *  rcr/alignment.hpp): a frame pixel whose triangle is smaller in the frame than in the crop averages Sx x Sy sub-samples, chosen per
 *  triangle and per axis.  The destinations may mix NV12 and the other formats; `chroma` as above (empty: every UV plane behind its Y
 *  plane).  `samples`, when given, takes rows x T x 2 ints: (Sx, Sy) of every triangle. */
inline warp_paste_result paste_warped_tensor(tracker& tr, const WarpMesh& mesh, const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                             const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma = {},
                                             const PasteMask& mask = {}, std::vector<int>* samples = nullptr)
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_warped_tensor: step the tracker first");
    return detail::warp_paste_current_rows(tr.context(), tr.rows().rows, mesh, spec, in_dev, frames, mask, &chroma, &filter, samples);
}

inline warp_paste_result paste_warped_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma,
                                             cv::Mat rows, const std::vector<int>& image_index, const WarpMesh& mesh, const TensorSpec& spec,
                                             const AlignFilter& filter, const void* in_dev, const PasteMask& mask = {},
                                             std::vector<int>* samples = nullptr)
{
    return detail::warp_paste_rows(model, frames, rows, image_index, mesh, spec, in_dev, mask, &chroma, &filter, samples);
}

inline warp_paste_result paste_warped_tensor(detection_model& model, cv::Mat points, const std::vector<int>& image_index, const WarpMesh& mesh,
                                             const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                             const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma = {},
                                             const PasteMask& mask = {}, std::vector<int>* samples = nullptr)
{
    return detail::warp_paste_points(model, points, image_index, mesh, spec, in_dev, frames, mask, &chroma, &filter, samples);
}

}  // namespace rcr
#endif /* RCR_WARP_HPP_ */
