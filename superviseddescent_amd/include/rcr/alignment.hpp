// rcr/alignment.hpp -- aligned face crops from landmarks kept on the device (include/sdm.h, sdm_align_*): a similarity fitted to a
// few landmarks of every face puts the face in a canonical position in an out_width x out_height crop -- the input of recognition,
// expression or attribute networks -- without copying the landmarks or the frames to the host for an image library.
//
//     rcr::tracker tr(model, 64);
//     auto lms = tr.step(ids, frames);                                         // gray frames: what the cascade runs on
//     cv::Mat tmpl = rcr::alignment_template(model.get_mean(), idx, 112, 112); // or the template of a recognition network
//     auto a = rcr::aligned_crops(tr, idx, tmpl, 112, 112, colour_frames);     // CV_8UC3 crops of the BGR frames
//     // a.crops[i]: stream ids[i]; a.matrices.row(i): its crop -> source map (M00 M01 M02 M10 M11 M12); a.flags[i]: SDM_ALIGN_*
//
// The rows of detection_model::detect_batch work the same way (the overload taking the images and the rows).
//
// rcr::aligned_crops_tensor writes the crops as a network's input tensor straight from frames on the device, and rcr::paste_crops_tensor is
// its way back: a network's output on those crops, warped back through the rows' similarities and blended into the frames in place.
#pragma once

#ifndef RCR_ALIGNMENT_HPP_
#define RCR_ALIGNMENT_HPP_

#include "rcr/model.hpp"
#include "rcr/tracker.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace rcr {

struct aligned_crops_result {
    std::vector<cv::Mat> crops;    // one out_height x out_width CV_8UC1 / CV_8UC3 image per row
    cv::Mat matrices;              // rows x 6 CV_32FC1: the crop -> source map of every row (NaN for a degenerate row)
    std::vector<int> flags;        // SDM_ALIGN_DEGENERATE / SDM_ALIGN_PARTIAL bits
};

/** The default template (K x 2 CV_32FC1, crop pixels; computed in double): the mean's landmarks `landmark_index` with their
 *  enclosing box centred in the crop and scaled so that its larger side is (1 - 2 margin) of the crop's smaller side. */
inline cv::Mat alignment_template(cv::Mat mean, const std::vector<int>& landmark_index, int width, int height, double margin = 0.2)
{
    const int L = (int)mean.total() / 2;
    if (landmark_index.empty()) throw std::runtime_error("alignment_template: no landmarks");
    std::vector<double> px, py;
    for (int i : landmark_index) {
        if (i < 0 || i >= L) throw std::runtime_error("alignment_template: landmark index out of range");
        px.push_back(mean.at<float>(i));
        py.push_back(mean.at<float>(i + L));
    }
    const double x0 = *std::min_element(px.begin(), px.end()), x1 = *std::max_element(px.begin(), px.end());
    const double y0 = *std::min_element(py.begin(), py.end()), y1 = *std::max_element(py.begin(), py.end());
    const double extent = std::max(x1 - x0, y1 - y0);
    if (!(extent > 0)) throw std::runtime_error("alignment_template: the selected mean points have no extent");
    const double s = (1.0 - 2.0 * margin) * std::min(width, height) / extent;
    cv::Mat t((int)px.size(), 2, CV_32FC1);
    for (size_t k = 0; k < px.size(); ++k) {
        t.at<float>((int)k, 0) = (float)((px[k] - (x0 + x1) / 2) * s + (width - 1) / 2.0);
        t.at<float>((int)k, 1) = (float)((py[k] - (y0 + y1) / 2) * s + (height - 1) / 2.0);
    }
    return t;
}

namespace detail {

// crops of the n current rows of the handle `c`, from its own images or -- `colour` not empty -- from equally sized CV_8UC1 / CV_8UC3
// images that stand in for them (one per image of the context, in its order)
inline aligned_crops_result align_current_rows(sdm_ctx* c, int n, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                               int height, const std::vector<cv::Mat>& colour)
{
    using superviseddescent::hip::check;
    if (tmpl.rows != (int)landmark_index.size() || tmpl.cols != 2) throw std::runtime_error("aligned_crops: one template point (x, y) per landmark");
    cv::Mat t = tmpl.isContinuous() ? tmpl : tmpl.clone();
    int C = 1;
    std::vector<uint8_t> stack;
    if (!colour.empty()) {
        const int w = colour[0].cols, h = colour[0].rows, type = colour[0].type();
        if (type != CV_8UC1 && type != CV_8UC3) throw std::runtime_error("aligned_crops: the source images must be CV_8UC1 or CV_8UC3");
        C = type == CV_8UC3 ? 3 : 1;
        const size_t row_bytes = (size_t)w * C;
        stack.resize(colour.size() * (size_t)h * row_bytes);
        for (size_t i = 0; i < colour.size(); ++i) {
            if (colour[i].cols != w || colour[i].rows != h || colour[i].type() != type)
                throw std::runtime_error("aligned_crops: the source images must be equally sized, of one type");
            for (int r = 0; r < h; ++r) std::memcpy(&stack[(i * h + r) * row_bytes], colour[i].ptr<uint8_t>(r), row_bytes);
        }
        check(sdm_align_set_source(c, stack.data(), (int)colour.size(), w, h, (int)row_bytes, C, 0), "sdm_align_set_source");
    } else {
        check(sdm_align_set_source(c, nullptr, 0, 0, 0, 0, 0, 0), "sdm_align_set_source");
    }
    aligned_crops_result res;
    std::vector<uint8_t> out((size_t)n * width * height * C);
    res.matrices = cv::Mat(n, 6, CV_32FC1);
    res.flags.resize((size_t)n);
    const int rc = sdm_align_crops(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, out.data(), 0,
                                   res.matrices.ptr<float>(0), res.flags.data());
    if (!colour.empty()) sdm_align_set_source(c, nullptr, 0, 0, 0, 0, 0, 0);     // (back to the context's images)
    check(rc, "sdm_align_crops");
    const size_t crop_bytes = (size_t)width * height * C;
    for (int r = 0; r < n; ++r) {
        cv::Mat m(height, width, C == 3 ? CV_8UC3 : CV_8UC1);
        std::memcpy(m.ptr<uint8_t>(0), out.data() + r * crop_bytes, crop_bytes);
        res.crops.push_back(m);
    }
    return res;
}

}  // namespace detail

/** Crops of the streams of the tracker's last step (tracker::step), from the step's frames (gray) or from `colour_frames`: one
 *  CV_8UC3 (or CV_8UC1) image per frame of that step, same size, same order -- e.g. the BGR frames the gray ones came from. */
inline aligned_crops_result aligned_crops(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                          const std::vector<cv::Mat>& colour_frames = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("aligned_crops: step the tracker first");
    return detail::align_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, colour_frames);
}

/** Crops of landmark rows on their images, e.g. the N x 2L result of detection_model::detect_batch(images, boxes, image_index):
 *  row i is cut from images[image_index[i]] (default: images[i]), or from the same entry of `colour_images`.  The C++
 *  detection_model keeps no device context between calls (each detect_batch runs on a handle of its own), so this overload
 *  uploads the images and the rows to a handle of its own as well: unlike the tracker overload, the frames and the landmarks
 *  cross the host link here.  Streams whose landmarks should stay on the device go through rcr::tracker. */
inline aligned_crops_result aligned_crops(detection_model& model, const std::vector<cv::Mat>& images, cv::Mat rows,
                                          const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl,
                                          int width, int height, const std::vector<cv::Mat>& colour_images = {})
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, images, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), true);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("aligned_crops: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::align_current_rows(c, x.rows, landmark_index, tmpl, width, height, colour_images);
}

/** What sdm_align_crops_tensor writes (sdm_align_tensor of include/sdm.h): the element type, the layout, 1 or 3 channels, their order,
 *  and element = float32(v) * scale[c] + bias[c] per output channel c (ignored for SDM_ALIGN_U8). */
struct TensorSpec {
    int dtype = SDM_ALIGN_F16, layout = SDM_ALIGN_NCHW, channels = 3, order = SDM_ALIGN_ORDER_RGB;
    float scale[3] = {1.0f, 1.0f, 1.0f}, bias[3] = {0.0f, 0.0f, 0.0f};
    int gray_shift = 14;
    /** mean and std in 0-255 units: scale = float(1 / std), bias = float(-mean / std), the quotients computed in double */
    TensorSpec& normalise(const double (&mean)[3], const double (&std)[3])
    {
        for (int c = 0; c < 3; ++c) { scale[c] = (float)(1.0 / std[c]); bias[c] = (float)(-mean[c] / std[c]); }
        return *this;
    }
    size_t element_size() const { return dtype == SDM_ALIGN_U8 ? 1 : dtype == SDM_ALIGN_F16 ? 2 : 4; }
};

/** The sampling of sdm_align_crops_tensor_filtered (sdm_align_filter of include/sdm.h): with SDM_ALIGN_FILTER_AREA a row whose similarity
 *  minifies averages S x S bilinear sub-samples per pixel, S the smallest integer with S^2 >= scale^2, at most max_samples (1 ... 16);
 *  rows with scale^2 < min_scale^2 (min_scale finite, >= 1) keep S = 1, the bits of the unfiltered call. */
struct AlignFilter {
    int mode = SDM_ALIGN_FILTER_AREA, max_samples = 16;
    float min_scale = 1.0f;
};

struct aligned_tensor_result {
    cv::Mat matrices;              // rows x 6 CV_32FC1: the crop -> source map of every row (NaN for a degenerate row)
    std::vector<int> flags;        // SDM_ALIGN_DEGENERATE / SDM_ALIGN_PARTIAL bits
    std::vector<int> samples;      // the overloads taking an AlignFilter: S of every row; empty otherwise
};

namespace detail {

// the n current rows of the handle `c` as a tensor in device memory, cut from `frames` in place (`chroma`: empty, or per frame the UV
// plane of an NV12 frame, nullptr = behind its Y plane) or -- no frames -- from the handle's own images; `filter`: nullptr, or the
// sampling of sdm_align_crops_tensor_filtered
inline aligned_tensor_result align_tensor_current_rows(sdm_ctx* c, int n, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                                       int height, const std::vector<DeviceFrame>& frames, const std::vector<const void*>& chroma,
                                                       const TensorSpec& spec, void* out_dev, const AlignFilter* filter = nullptr)
{
    using superviseddescent::hip::check;
    if (tmpl.rows != (int)landmark_index.size() || tmpl.cols != 2) throw std::runtime_error("aligned_crops_tensor: one template point (x, y) per landmark");
    if (!chroma.empty() && chroma.size() != frames.size()) throw std::runtime_error("aligned_crops_tensor: one chroma pointer (or nullptr) per frame");
    cv::Mat t = tmpl.isContinuous() ? tmpl : tmpl.clone();
    std::vector<sdm_frame> f;
    for (const auto& d : frames) f.push_back(sdm_frame{d.data, d.width, d.height, d.stride_bytes, d.format});
    const SecondPlanes<const void*> planes(frames, &chroma);                  // (a frame's own second_plane where chroma names none)
    check(sdm_align_set_source_frames(c, f.empty() ? nullptr : f.data(), planes.data(), (int)f.size()),
          "sdm_align_set_source_frames");
    sdm_align_tensor s{};
    s.dtype = spec.dtype; s.layout = spec.layout; s.channels = spec.channels; s.order = spec.order; s.gray_shift = spec.gray_shift;
    for (int k = 0; k < 3; ++k) { s.scale[k] = spec.scale[k]; s.bias[k] = spec.bias[k]; }
    aligned_tensor_result res;
    res.matrices = cv::Mat(n, 6, CV_32FC1);
    res.flags.resize((size_t)n);
    int rc;
    if (filter) {
        const sdm_align_filter f{filter->mode, filter->max_samples, filter->min_scale};
        res.samples.resize((size_t)n);
        rc = sdm_align_crops_tensor_filtered(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, &s, &f, out_dev,
                                             res.matrices.ptr<float>(0), res.flags.data(), res.samples.data());
    } else {
        rc = sdm_align_crops_tensor(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, &s, out_dev,
                                    res.matrices.ptr<float>(0), res.flags.data());
    }
    if (!frames.empty()) sdm_align_set_source_frames(c, nullptr, nullptr, 0);     // (no pointer to the caller's frames stays behind)
    check(rc, filter ? "sdm_align_crops_tensor_filtered" : "sdm_align_crops_tensor");
    return res;
}

}  // namespace detail

/** The streams of the tracker's last step as a network's input tensor, written to `out_dev` (device memory, rows * channels * height *
 *  width elements of spec.dtype, 16-byte aligned): cut in one launch from `frames` where they lie on the device -- the frames of that
 *  step, any of the six formats, same sizes, same order -- or, `frames` empty, from the step's gray images. */
inline aligned_tensor_result aligned_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                                  const TensorSpec& spec, void* out_dev, const std::vector<DeviceFrame>& frames = {},
                                                  const std::vector<const void*>& chroma = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("aligned_crops_tensor: step the tracker first");
    return detail::align_tensor_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, frames, chroma, spec, out_dev);
}

/** The same with the sampling of `filter`: faces that are larger in the frame than in the crop are averaged over every pixel's footprint;
 *  the result's `samples` holds S of every stream. */
inline aligned_tensor_result aligned_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                                  const TensorSpec& spec, const AlignFilter& filter, void* out_dev,
                                                  const std::vector<DeviceFrame>& frames = {}, const std::vector<const void*>& chroma = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("aligned_crops_tensor: step the tracker first");
    return detail::align_tensor_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, frames, chroma, spec, out_dev,
                                             &filter);
}

/** The same for landmark rows on device frames, e.g. the result of detection_model::detect_batch(frames, boxes, image_index): row i is
 *  cut from frames[image_index[i]] (default: frames[i]).  As the cv::Mat overload of aligned_crops, this one works on a handle of its
 *  own: the frames become its image set (colour converted to gray once, which the crops do not read) and the rows are uploaded. */
inline aligned_tensor_result aligned_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                                  const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl,
                                                  int width, int height, const TensorSpec& spec, void* out_dev,
                                                  const std::vector<const void*>& chroma = {}, const AlignFilter* filter = nullptr)
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::set_device_frames(h, frames);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("aligned_crops_tensor: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::align_tensor_current_rows(c, x.rows, landmark_index, tmpl, width, height, frames, chroma, spec, out_dev, filter);
}

/** The same with the sampling of `filter` (the result's `samples`: S of every row). */
inline aligned_tensor_result aligned_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                                  const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl,
                                                  int width, int height, const TensorSpec& spec, const AlignFilter& filter, void* out_dev,
                                                  const std::vector<const void*>& chroma = {})
{
    return aligned_crops_tensor(model, frames, rows, image_index, landmark_index, tmpl, width, height, spec, out_dev, chroma, &filter);
}

/** The crop-space opacity of a paste (sdm_align_paste of include/sdm.h): device memory, height x width bytes for all rows or -- per_row --
 *  one such map per row; nullptr: 255 everywhere inside the crop. */
struct PasteMask {
    const uint8_t* alpha_dev = nullptr;
    bool per_row = false;
};

struct paste_result {
    cv::Mat matrices;              // rows x 6 CV_32FC1: the crop -> frame map of every row (NaN for a degenerate row of the fit)
    std::vector<int> flags;        // SDM_ALIGN_DEGENERATE / SDM_ALIGN_PARTIAL bits
    std::vector<int> samples;      // the overloads taking an AlignFilter: S of every row; empty otherwise
};

namespace detail {

inline sdm_align_tensor paste_spec(const TensorSpec& spec)
{
    sdm_align_tensor s{};
    s.dtype = spec.dtype; s.layout = spec.layout; s.channels = spec.channels; s.order = spec.order; s.gray_shift = spec.gray_shift;
    for (int k = 0; k < 3; ++k) { s.scale[k] = spec.scale[k]; s.bias[k] = spec.bias[k]; }
    return s;
}

inline std::vector<sdm_frame> paste_frames(const std::vector<DeviceFrame>& frames)
{
    std::vector<sdm_frame> f;
    for (const auto& d : frames) f.push_back(sdm_frame{d.data, d.width, d.height, d.stride_bytes, d.format});
    return f;
}

// the UV planes of an NV12 paste as the C call takes them: one entry per frame, or none at all
inline void* const* paste_chroma(const std::vector<void*>& chroma, size_t n_frames)
{
    if (!chroma.empty() && chroma.size() != n_frames) throw std::runtime_error("paste_crops_tensor: one chroma entry (or nullptr) per frame");
    return chroma.empty() ? nullptr : chroma.data();
}

// the n current rows of the handle `c`: the fit of aligned_crops_tensor, then the tensor at `in_dev` pasted into `frames` in place;
// `filter`: nullptr, or the sampling of sdm_align_paste_tensor_filtered; `chroma`: nullptr, or -- the overloads for NV12 destinations,
// sdm_align_paste_tensor_nv12 -- the frames' UV planes (empty: every one directly behind its Y plane)
inline paste_result paste_current_rows(sdm_ctx* c, int n, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                       const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames, const PasteMask& mask,
                                       const AlignFilter* filter = nullptr, const std::vector<void*>* chroma = nullptr)
{
    using superviseddescent::hip::check;
    if (tmpl.rows != (int)landmark_index.size() || tmpl.cols != 2) throw std::runtime_error("paste_crops_tensor: one template point (x, y) per landmark");
    cv::Mat t = tmpl.isContinuous() ? tmpl : tmpl.clone();
    const std::vector<sdm_frame> f = paste_frames(frames);
    if (chroma) paste_chroma(*chroma, f.size());                                // (its size check)
    const SecondPlanes<void*> planes(frames, chroma);                           // (a frame's own second_plane where chroma names none)
    const sdm_align_tensor s = paste_spec(spec);
    const sdm_align_paste p{mask.alpha_dev, mask.per_row ? 1 : 0};
    paste_result res;
    res.matrices = cv::Mat(n, 6, CV_32FC1);
    res.flags.resize((size_t)n);
    if (chroma || planes.any) {
        const sdm_align_filter fl = filter ? sdm_align_filter{filter->mode, filter->max_samples, filter->min_scale} : sdm_align_filter{};
        if (filter) res.samples.resize((size_t)n);
        check(sdm_align_paste_tensor_nv12(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, &s,
                                          filter ? &fl : nullptr, in_dev, &p, f.empty() ? nullptr : f.data(), planes.data(),
                                          (int)f.size(), res.matrices.ptr<float>(0), res.flags.data(), filter ? res.samples.data() : nullptr),
              "sdm_align_paste_tensor_nv12");
        return res;
    }
    if (filter) {
        const sdm_align_filter fl{filter->mode, filter->max_samples, filter->min_scale};
        res.samples.resize((size_t)n);
        check(sdm_align_paste_tensor_filtered(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, &s, &fl,
                                              in_dev, &p, f.empty() ? nullptr : f.data(), (int)f.size(), res.matrices.ptr<float>(0),
                                              res.flags.data(), res.samples.data()),
              "sdm_align_paste_tensor_filtered");
        return res;
    }
    check(sdm_align_paste_tensor(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height, &s, in_dev, &p,
                                 f.empty() ? nullptr : f.data(), (int)f.size(), res.matrices.ptr<float>(0), res.flags.data()),
          "sdm_align_paste_tensor");
    return res;
}

}  // namespace detail

/** The way back of aligned_crops_tensor: `in_dev` -- a network's output on the crops of the tracker's last step, rows * channels * height *
 *  width elements of spec.dtype in spec.layout, 16-byte aligned device memory -- is warped back through every stream's fitted similarity
 *  and blended into `frames` IN PLACE (the frames of that step, GRAY / BGR / RGB / BGRA / RGBA; NV12: the overloads with `chroma`), in one launch
 *  (include/sdm.h, "Pasting crops back").  An element is decoded as e * spec.scale[c] + spec.bias[c]: scale = std, bias = mean in 0-255
 *  units undo TensorSpec::normalise(mean, std) of the crop call. */
inline paste_result paste_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                       const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                       const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_crops_tensor: step the tracker first");
    return detail::paste_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, spec, in_dev, frames, mask);
}

/** The same with the sampling of `filter` (sdm_align_paste_tensor_filtered): where the crop is larger than the face in the frame, every
 *  frame pixel averages S x S sub-samples of the crop; the result's `samples` holds S of every stream. */
inline paste_result paste_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                       const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                       const std::vector<DeviceFrame>& frames, const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_crops_tensor: step the tracker first");
    return detail::paste_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, spec, in_dev, frames, mask, &filter);
}

/** NV12 destinations (include/sdm.h, "Pasting crops back into NV12 frames"): `frames` may hold SDM_FRAME_NV12 entries -- the decoder
 *  surfaces the tracker stepped on -- beside the other five formats; luma and 4:2:0 chroma are blended in place.  `chroma`: per frame the
 *  UV plane's device pointer, or nullptr / an empty vector for "directly behind the Y plane" (as for aligned_crops_tensor). */
inline paste_result paste_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                       const TensorSpec& spec, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                       const std::vector<void*>& chroma, const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_crops_tensor: step the tracker first");
    return detail::paste_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, spec, in_dev, frames, mask, nullptr,
                                      &chroma);
}

/** NV12 destinations with the sampling of `filter`. */
inline paste_result paste_crops_tensor(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                       const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                       const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma, const PasteMask& mask = {})
{
    if (tr.rows().rows < 1) throw std::runtime_error("paste_crops_tensor: step the tracker first");
    return detail::paste_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, spec, in_dev, frames, mask, &filter,
                                      &chroma);
}

/** The same for landmark rows on device frames (as the detection_model overload of aligned_crops_tensor: a handle of its own, the frames
 *  as its image set, the rows uploaded): row i is pasted into frames[image_index[i]] (default: frames[i]).  `chroma`: nullptr, or the
 *  frames' UV planes -- then NV12 frames are accepted (the overloads below). */
inline paste_result paste_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                       const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                       int height, const TensorSpec& spec, const void* in_dev, const PasteMask& mask = {},
                                       const AlignFilter* filter = nullptr, const std::vector<void*>* chroma = nullptr)
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::set_device_frames(h, frames);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("paste_crops_tensor: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::paste_current_rows(c, x.rows, landmark_index, tmpl, width, height, spec, in_dev, frames, mask, filter, chroma);
}

/** NV12 destinations for landmark rows: `chroma` as in the tracker overload; `filter`: nullptr (plain bilinear) or the sampling. */
inline paste_result paste_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma,
                                       cv::Mat rows, const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl,
                                       int width, int height, const TensorSpec& spec, const void* in_dev, const PasteMask& mask = {},
                                       const AlignFilter* filter = nullptr)
{
    return paste_crops_tensor(model, frames, rows, image_index, landmark_index, tmpl, width, height, spec, in_dev, mask, filter, &chroma);
}

inline paste_result paste_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma,
                                       cv::Mat rows, const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl,
                                       int width, int height, const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                       const PasteMask& mask = {})
{
    return paste_crops_tensor(model, frames, rows, image_index, landmark_index, tmpl, width, height, spec, in_dev, mask, &filter, &chroma);
}

/** The same with the sampling of `filter` (the result's `samples`: S of every row). */
inline paste_result paste_crops_tensor(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                       const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                       int height, const TensorSpec& spec, const AlignFilter& filter, const void* in_dev,
                                       const PasteMask& mask = {})
{
    return paste_crops_tensor(model, frames, rows, image_index, landmark_index, tmpl, width, height, spec, in_dev, mask, &filter);
}

/** The explicit form (sdm_align_paste_tensor_at): `matrices` rows x 6 CV_32FC1 as an earlier crop call returned them -- the rows need not
 *  be current any more; no model, no landmark state.  Row i goes to frames[image_index[i]] (default: frames[i]).  The result's matrices
 *  are the ones given. */
inline paste_result paste_crops_tensor(cv::Mat matrices, const std::vector<int>& image_index, int width, int height, const TensorSpec& spec,
                                       const void* in_dev, const std::vector<DeviceFrame>& frames, const PasteMask& mask = {},
                                       const AlignFilter* filter = nullptr, const std::vector<void*>* chroma = nullptr)
{
    using superviseddescent::hip::check;
    if (matrices.type() != CV_32FC1 || matrices.cols != 6 || matrices.rows < 1) throw std::runtime_error("paste_crops_tensor: matrices must be rows x 6 CV_32FC1");
    if (!image_index.empty() && (int)image_index.size() != matrices.rows) throw std::runtime_error("paste_crops_tensor: one image index per row");
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    paste_result res;
    res.matrices = matrices.isContinuous() ? matrices : matrices.clone();
    res.flags.resize((size_t)matrices.rows);
    const std::vector<sdm_frame> f = detail::paste_frames(frames);
    if (chroma) detail::paste_chroma(*chroma, f.size());                        // (its size check)
    const detail::SecondPlanes<void*> planes(frames, chroma);                   // (a frame's own second_plane where chroma names none)
    const sdm_align_tensor s = detail::paste_spec(spec);
    const sdm_align_paste p{mask.alpha_dev, mask.per_row ? 1 : 0};
    if (chroma || planes.any) {
        const sdm_align_filter fl = filter ? sdm_align_filter{filter->mode, filter->max_samples, filter->min_scale} : sdm_align_filter{};
        if (filter) res.samples.resize((size_t)matrices.rows);
        check(sdm_align_paste_tensor_at_nv12(h.get(), res.matrices.ptr<float>(0), image_index.empty() ? nullptr : image_index.data(),
                                             matrices.rows, width, height, &s, filter ? &fl : nullptr, in_dev, &p,
                                             f.empty() ? nullptr : f.data(), planes.data(), (int)f.size(),
                                             res.flags.data(), filter ? res.samples.data() : nullptr),
              "sdm_align_paste_tensor_at_nv12");
        return res;
    }
    if (filter) {
        const sdm_align_filter fl{filter->mode, filter->max_samples, filter->min_scale};
        res.samples.resize((size_t)matrices.rows);
        check(sdm_align_paste_tensor_at_filtered(h.get(), res.matrices.ptr<float>(0), image_index.empty() ? nullptr : image_index.data(),
                                                 matrices.rows, width, height, &s, &fl, in_dev, &p, f.empty() ? nullptr : f.data(), (int)f.size(),
                                                 res.flags.data(), res.samples.data()),
              "sdm_align_paste_tensor_at_filtered");
        return res;
    }
    check(sdm_align_paste_tensor_at(h.get(), res.matrices.ptr<float>(0), image_index.empty() ? nullptr : image_index.data(), matrices.rows, width,
                                    height, &s, in_dev, &p, f.empty() ? nullptr : f.data(), (int)f.size(), res.flags.data()),
          "sdm_align_paste_tensor_at");
    return res;
}

/** The explicit form with the sampling of `filter` (sdm_align_paste_tensor_at_filtered; the result's `samples`: S of every row). */
inline paste_result paste_crops_tensor(cv::Mat matrices, const std::vector<int>& image_index, int width, int height, const TensorSpec& spec,
                                       const AlignFilter& filter, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                       const PasteMask& mask = {})
{
    return paste_crops_tensor(matrices, image_index, width, height, spec, in_dev, frames, mask, &filter);
}

/** The explicit form for NV12 destinations (sdm_align_paste_tensor_at_nv12): `chroma` as in the tracker overload. */
inline paste_result paste_crops_tensor(cv::Mat matrices, const std::vector<int>& image_index, int width, int height, const TensorSpec& spec,
                                       const void* in_dev, const std::vector<DeviceFrame>& frames, const std::vector<void*>& chroma,
                                       const PasteMask& mask = {})
{
    return paste_crops_tensor(matrices, image_index, width, height, spec, in_dev, frames, mask, nullptr, &chroma);
}

inline paste_result paste_crops_tensor(cv::Mat matrices, const std::vector<int>& image_index, int width, int height, const TensorSpec& spec,
                                       const AlignFilter& filter, const void* in_dev, const std::vector<DeviceFrame>& frames,
                                       const std::vector<void*>& chroma, const PasteMask& mask = {})
{
    return paste_crops_tensor(matrices, image_index, width, height, spec, in_dev, frames, mask, &filter, &chroma);
}

/** A landmark region (sdm_region_mask of include/sdm.h, "Landmark region masks"): the union of `polygons` minus `holes` -- each the
 *  positions of 3 to 128 landmarks in order --, moved outwards by `grow` crop pixels, with a linear ramp `feather` pixels wide.
 *  `hull`: the positions, in polygons followed by holes, of the polygons that are the convex hull of their landmarks. */
struct RegionMask {
    std::vector<std::vector<int>> polygons, holes;
    std::vector<int> hull;
    float grow = 0.0f, feather = 0.0f;
};

struct region_masks_result {
    cv::Mat matrices;              // rows x 6 CV_32FC1: the crop -> frame map of every row
    std::vector<int> flags;        // SDM_ALIGN_DEGENERATE / SDM_ALIGN_PARTIAL / SDM_REGION_NONFINITE bits; a flagged row's map is zeros
};

namespace detail {

// the region as the C calls take it: the vertex counts (holes last), the hull bits, and the vertex indices one polygon after the other
struct RegionArgs {
    std::vector<int> sizes, vertex_index;
    sdm_region_mask region{};
    explicit RegionArgs(const RegionMask& r)
    {
        for (const auto* list : {&r.polygons, &r.holes})
            for (const auto& p : *list) {
                sizes.push_back((int)p.size());
                vertex_index.insert(vertex_index.end(), p.begin(), p.end());
            }
        unsigned bits = 0;
        for (int g : r.hull) {
            if (g < 0 || g >= (int)sizes.size()) throw std::runtime_error("region_masks: hull names a polygon that is not there");
            bits |= 1u << g;
        }
        region = sdm_region_mask{sizes.data(), (int)sizes.size(), (int)r.holes.size(), bits, r.grow, r.feather};
    }
    RegionArgs(const RegionArgs&) = delete;
    RegionArgs& operator=(const RegionArgs&) = delete;
};

inline region_masks_result region_masks_current_rows(sdm_ctx* c, int n, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                                     int height, const RegionMask& region, uint8_t* out_dev)
{
    using superviseddescent::hip::check;
    if (tmpl.rows != (int)landmark_index.size() || tmpl.cols != 2) throw std::runtime_error("region_masks: one template point (x, y) per landmark");
    cv::Mat t = tmpl.isContinuous() ? tmpl : tmpl.clone();
    const RegionArgs a(region);
    region_masks_result res;
    res.matrices = cv::Mat(n, 6, CV_32FC1);
    res.flags.resize((size_t)n);
    check(sdm_align_region_mask(c, landmark_index.data(), t.ptr<float>(0), (int)landmark_index.size(), width, height,
                                a.vertex_index.empty() ? nullptr : a.vertex_index.data(), &a.region, out_dev, res.matrices.ptr<float>(0),
                                res.flags.data()),
          "sdm_align_region_mask");
    return res;
}

}  // namespace detail

/** One crop-space opacity map per stream of the tracker's last step, drawn from its landmarks on the device: `out_dev` -- rows * height *
 *  width bytes of 16-byte aligned device memory, row n at n * height * width -- is what PasteMask{out_dev, true} takes.  The fit is that
 *  of aligned_crops_tensor on `landmark_index` / `tmpl`, so the maps line up with its crops. */
inline region_masks_result region_masks(tracker& tr, const std::vector<int>& landmark_index, cv::Mat tmpl, int width, int height,
                                        const RegionMask& region, uint8_t* out_dev)
{
    if (tr.rows().rows < 1) throw std::runtime_error("region_masks: step the tracker first");
    return detail::region_masks_current_rows(tr.context(), tr.rows().rows, landmark_index, tmpl, width, height, region, out_dev);
}

/** The same for landmark rows on device frames (as the detection_model overload of paste_crops_tensor: a handle of its own, the frames as
 *  its image set, the rows uploaded). */
inline region_masks_result region_masks(detection_model& model, const std::vector<DeviceFrame>& frames, cv::Mat rows,
                                        const std::vector<int>& image_index, const std::vector<int>& landmark_index, cv::Mat tmpl, int width,
                                        int height, const RegionMask& region, uint8_t* out_dev)
{
    using superviseddescent::hip::check;
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    sdm_ctx* c = h.get();
    detail::configure(h, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(), false);
    detail::set_device_frames(h, frames);
    cv::Mat x = rows.isContinuous() ? rows : rows.clone();
    if (x.cols != 2 * (int)model.get_landmark_ids().size()) throw std::runtime_error("region_masks: rows must hold 2L coordinates");
    if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
    else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
    check(sdm_set_x(c, x.ptr<float>(0), x.rows), "sdm_set_x");
    return detail::region_masks_current_rows(c, x.rows, landmark_index, tmpl, width, height, region, out_dev);
}

/** The explicit form (sdm_align_region_mask_at): `matrices` rows x 6 CV_32FC1 as an earlier crop call returned them, `points` rows x 2P
 *  CV_32FC1 -- (x, y) of every vertex in the frame, one polygon after the other --; of `region`'s polygons only the sizes are read.  No
 *  model, no landmark state.  The result's matrices are the ones given. */
inline region_masks_result region_masks(cv::Mat matrices, cv::Mat points, int width, int height, const RegionMask& region, uint8_t* out_dev)
{
    using superviseddescent::hip::check;
    const detail::RegionArgs a(region);
    if (matrices.type() != CV_32FC1 || matrices.cols != 6 || matrices.rows < 1) throw std::runtime_error("region_masks: matrices must be rows x 6 CV_32FC1");
    if (points.type() != CV_32FC1 || points.rows != matrices.rows || points.cols != 2 * (int)a.vertex_index.size())
        throw std::runtime_error("region_masks: points must be rows x 2P CV_32FC1");
    superviseddescent::hip::Handle h(superviseddescent::hip::device());
    region_masks_result res;
    res.matrices = matrices.isContinuous() ? matrices : matrices.clone();
    res.flags.resize((size_t)matrices.rows);
    cv::Mat p = points.isContinuous() ? points : points.clone();
    check(sdm_align_region_mask_at(h.get(), res.matrices.ptr<float>(0), p.ptr<float>(0), matrices.rows, width, height, &a.region, out_dev,
                                   res.flags.data()),
          "sdm_align_region_mask_at");
    return res;
}

}  // namespace rcr
#endif /* RCR_ALIGNMENT_HPP_ */
