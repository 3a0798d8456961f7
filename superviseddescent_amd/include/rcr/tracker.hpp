// rcr/tracker.hpp -- multi-stream face tracking with the landmark state kept on the device (include/sdm.h, sdm_track_*): the loop
// the reference's apps/rcr/rcr-track.cpp:133-177 sketches -- start a face from a detector box, follow it frame by frame with
// detect(image, initialisation) (include/rcr/model.hpp:146-157), restart it from a new box once it is lost -- for many faces at
// once, without the landmarks of a stream leaving the device between frames.
//
//     rcr::tracker tr(model, 64);                       // 64 stream slots, realign initialisation
//     tr.start({0, 1}, {box_a, box_b});                 // boxes from a face detector
//     auto lms = tr.step({0, 1}, {frame, frame});       // two faces in one frame: two streams on the same image
//     if (tr.lost()[1]) tr.start({1}, {new_box});       // have_face = false -> detector -> restart
//
// Rolled faces (phone video, ceiling cameras, tilted heads): tr.upright(288) makes every step cut each stream's face upright as a
// 288 x 288 chip -- the roll from the stream's own previous eye line --, run the cascade there and map the result back
// (include/sdm.h, "Rolled faces"); tr.start(ids, boxes, rolls) starts streams whose faces are rolled in their boxes.
//
// Faces in video: tr.smooth(1.0f, 5.0f) puts a One-Euro filter behind the tracker (include/sdm.h, "Tracking, filtered"), and
// tr.step(ids, frames, dt) returns the filtered landmarks and leaves them as the context's current rows -- crops, warps, pastes and
// poses follow them; raw_rows() holds what the cascade gave.  Tracking itself is not changed by the filter.
//
// Faces that move fast: tr.motion() makes every step estimate each tracked stream's translation since its last frame by block
// matching on a 32 x 32 chip of block means and start the cascade from the shifted landmarks (include/sdm.h, "Tracking,
// motion-compensated"); tr.last_motion(ids) returns what the search found.
#pragma once

#ifndef RCR_TRACKER_HPP_
#define RCR_TRACKER_HPP_

#include "rcr/model.hpp"

#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

namespace rcr {

class tracker {
public:
    enum class init_mode { previous = SDM_TRACK_INIT_PREVIOUS, realign = SDM_TRACK_INIT_REALIGN };
    enum status { free_slot = SDM_TRACK_FREE, started = SDM_TRACK_STARTED, tracked = SDM_TRACK_TRACKED, lost_slot = SDM_TRACK_LOST };

    /** `capacity` stream slots on the device of superviseddescent::hip::device().  A stream is lost when its result is not finite,
     *  its enclosing box is smaller than min_size pixels, the box centre leaves the image, or its inter-eye distance changes by more
     *  than the factor max_scale_change in one step (0: no such rule).  The model's regressors are uploaded here, once. */
    tracker(detection_model& model, int capacity, init_mode init = init_mode::realign, float min_size = 8.0f, float max_scale_change = 1.5f)
        : model(model)
    {
        using superviseddescent::hip::check;
        sdm_ctx* c = handle.get();
        detail::configure(handle, {}, model.get_hog_params(), model.get_landmark_ids(), model.get_right_eye_ids(), model.get_left_eye_ids(),
                          false);
        auto& regressors = model.get_optimised_model().get_regressors();
        if (regressors.size() != model.get_hog_params().size()) throw std::runtime_error("tracker: one regressor per HoGParam expected");
        for (size_t level = 0; level < regressors.size(); ++level) {
            cv::Mat R = regressors[level].x.isContinuous() ? regressors[level].x : regressors[level].x.clone();
            if (R.empty() || R.rows != sdm_feature_dim(c, (int)level) || R.cols != 2 * num_landmarks())
                throw std::runtime_error("tracker: the regressor of level " + std::to_string(level) + " does not match the HOG geometry");
            check(sdm_set_regressor(c, (int)level, R.ptr<float>(0)), "sdm_set_regressor");
        }
        cv::Mat mean = model.get_mean().isContinuous() ? model.get_mean() : model.get_mean().clone();
        if ((int)mean.total() != 2 * num_landmarks()) throw std::runtime_error("tracker: the mean must hold 2L coordinates");
        check(sdm_track_configure(c, capacity, mean.ptr<float>(0), (int)init, min_size, max_scale_change), "sdm_track_configure");
    }

    /** (Re)start streams from face boxes, live or lost. */
    void start(const std::vector<int>& ids, const std::vector<cv::Rect>& boxes)
    {
        if (ids.size() != boxes.size()) throw std::runtime_error("tracker::start: one box per stream id expected");
        std::vector<int> b;
        for (const auto& r : boxes) { b.push_back(r.x); b.push_back(r.y); b.push_back(r.width); b.push_back(r.height); }
        superviseddescent::hip::check(sdm_track_start(handle.get(), ids.data(), b.data(), (int)ids.size()), "sdm_track_start");
    }

    /** Upright mode for rolled faces: chip x chip pixels per face, guard = the NEAR_EDGE band (default chip / 8).  chip == 0: off. */
    void upright(int chip, int guard = -1)
    {
        using superviseddescent::hip::check;
        if (chip == 0) { check(sdm_track_configure_upright(handle.get(), 0), "sdm_track_configure_upright"); return; }
        check(sdm_upright_configure(handle.get(), chip, guard < 0 ? chip / 8 : guard), "sdm_upright_configure");
        check(sdm_track_configure_upright(handle.get(), 1), "sdm_track_configure_upright");
    }

    /** (Re)start streams whose faces are rolled by rolls[i] degrees (clockwise positive) in their boxes; upright mode only. */
    void start(const std::vector<int>& ids, const std::vector<cv::Rect>& boxes, const std::vector<float>& rolls)
    {
        if (ids.size() != boxes.size() || ids.size() != rolls.size()) throw std::runtime_error("tracker::start: one box and one roll per stream id expected");
        std::vector<int> b;
        for (const auto& r : boxes) { b.push_back(r.x); b.push_back(r.y); b.push_back(r.width); b.push_back(r.height); }
        superviseddescent::hip::check(sdm_track_start_rolled(handle.get(), ids.data(), b.data(), rolls.data(), (int)ids.size()), "sdm_track_start_rolled");
    }

    /** A One-Euro filter on what step(..., dt) returns: min_cutoff > 0 Hz (how steady a still face is), beta >= 0 Hz per face size
     *  per second (how fast the filter lets go when the face moves), d_cutoff > 0 Hz.  Every stream's filter starts empty. */
    void smooth(float min_cutoff, float beta, float d_cutoff = 1.0f)
    {
        superviseddescent::hip::check(sdm_track_configure_filter(handle.get(), SDM_TRACK_FILTER_ONE_EURO, min_cutoff, beta, d_cutoff),
                                      "sdm_track_configure_filter");
    }
    /** The filter off again. */
    void smooth_off()
    {
        superviseddescent::hip::check(sdm_track_configure_filter(handle.get(), SDM_TRACK_FILTER_OFF, 0.f, 0.f, 0.f), "sdm_track_configure_filter");
    }

    /** What the last step's search found for one stream: the shift in pixels, the best SAD, SAD(0, 0), the cell size k and whether
     *  the stream was searched (a started stream, or one without a valid chip, is not: all zeros). */
    struct motion_result { int dx, dy, sad_best, sad_zero, k, searched; };

    /** Motion-compensated initialisation: search 1 ... 16 chip pixels, scale in [0.5, 4] (the chip's side in face sizes), min_gain
     *  0 ... 255 (how much, in 256ths, the best offset must beat staying in place).  Every stream's chip starts empty. */
    void motion(int search = 8, float scale = 1.25f, int min_gain = 64)
    {
        superviseddescent::hip::check(sdm_track_configure_motion(handle.get(), SDM_TRACK_MOTION_SAD, search, scale, min_gain),
                                      "sdm_track_configure_motion");
    }
    /** The mode off again. */
    void motion_off()
    {
        superviseddescent::hip::check(sdm_track_configure_motion(handle.get(), SDM_TRACK_MOTION_OFF, 0, 0.f, 0), "sdm_track_configure_motion");
    }
    /** The last step's search results of the streams `ids`; grids (n x {k, ox, oy}) and chips (n x 32 x 32 bytes) when asked for. */
    std::vector<motion_result> last_motion(const std::vector<int>& ids, std::vector<int>* grids = nullptr, std::vector<uint8_t>* chips = nullptr)
    {
        std::vector<int> m(ids.size() * 6);
        if (grids) grids->resize(ids.size() * 3);
        if (chips) chips->resize(ids.size() * 1024);
        superviseddescent::hip::check(sdm_track_get_motion(handle.get(), ids.data(), (int)ids.size(), m.data(), grids ? grids->data() : nullptr,
                                                           chips ? chips->data() : nullptr), "sdm_track_get_motion");
        std::vector<motion_result> out(ids.size());
        for (size_t i = 0; i < ids.size(); ++i) out[i] = {m[6 * i], m[6 * i + 1], m[6 * i + 2], m[6 * i + 3], m[6 * i + 4], m[6 * i + 5]};
        return out;
    }

    void stop(const std::vector<int>& ids)
    {
        superviseddescent::hip::check(sdm_track_stop(handle.get(), ids.data(), (int)ids.size()), "sdm_track_stop");
    }

    /** One frame for the streams `ids`: row i belongs to stream ids[i] and reads frames[image_index[i]] (default: frames[i]).
     *  Returns the landmarks of every row; lost() holds the rows' lost masks (0 = tracked, else SDM_TRACK_LOST_* bits) and rows()
     *  the n x 2L result. */
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<cv::Mat>& frames,
                                                    const std::vector<int>& image_index = {})
    {
        detail::upload_images(handle, frames);
        return step_on_current_images(ids, image_index);
    }

    /** The same on frames that are already on the device (rcr::DeviceFrame: gray and NV12 luma in place, colour converted once on the
     *  device; every frame with its own size and pitch). */
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<DeviceFrame>& frames,
                                                    const std::vector<int>& image_index = {})
    {
        detail::set_device_frames(handle, frames);
        return step_on_current_images(ids, image_index);
    }

    /** The same through the filter of smooth(): dt = seconds since the streams' last step with dt, one value (a float or double) for
     *  all rows or a std::vector<float> with one per row.  Returns the FILTERED landmarks, which are the context's current rows
     *  afterwards; rows() holds them as n x 2L, raw_rows() the cascade's own result, lost() the masks.
     *  (Templates, so that a braced third argument still means image_index.) */
    template <class Dt, typename std::enable_if<std::is_floating_point<Dt>::value, int>::type = 0>
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<cv::Mat>& frames, Dt dt,
                                                    const std::vector<int>& image_index = {})
    {
        return step(ids, frames, std::vector<float>(ids.size(), (float)dt), image_index);
    }
    template <class Dt, typename std::enable_if<std::is_floating_point<Dt>::value, int>::type = 0>
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<DeviceFrame>& frames, Dt dt,
                                                    const std::vector<int>& image_index = {})
    {
        return step(ids, frames, std::vector<float>(ids.size(), (float)dt), image_index);
    }
    template <class Dt, typename std::enable_if<std::is_same<Dt, std::vector<float>>::value, int>::type = 0>
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<cv::Mat>& frames, const Dt& dt,
                                                    const std::vector<int>& image_index = {})
    {
        detail::upload_images(handle, frames);
        return step_on_current_images(ids, image_index, &dt);
    }
    template <class Dt, typename std::enable_if<std::is_same<Dt, std::vector<float>>::value, int>::type = 0>
    std::vector<LandmarkCollection<cv::Vec2f>> step(const std::vector<int>& ids, const std::vector<DeviceFrame>& frames, const Dt& dt,
                                                    const std::vector<int>& image_index = {})
    {
        detail::set_device_frames(handle, frames);
        return step_on_current_images(ids, image_index, &dt);
    }

    /** The streams' filtered landmarks, their derivative rows (pixels per second, n x 2L) and primed flags; a stream whose filter
     *  holds nothing yet gives zeros. */
    std::pair<std::vector<LandmarkCollection<cv::Vec2f>>, std::vector<int>> get_filtered(const std::vector<int>& ids, cv::Mat* derivative = nullptr)
    {
        cv::Mat rows((int)ids.size(), 2 * num_landmarks(), CV_32FC1), d((int)ids.size(), 2 * num_landmarks(), CV_32FC1);
        std::vector<int> primed(ids.size());
        superviseddescent::hip::check(sdm_track_get_filtered(handle.get(), ids.data(), (int)ids.size(), rows.ptr<float>(0), d.ptr<float>(0),
                                                             primed.data()), "sdm_track_get_filtered");
        if (derivative) *derivative = d;
        return {collections(rows), primed};
    }

    /** The streams' landmarks (a started stream: its aligned mean) and statuses. */
    std::pair<std::vector<LandmarkCollection<cv::Vec2f>>, std::vector<int>> get(const std::vector<int>& ids)
    {
        cv::Mat rows((int)ids.size(), 2 * num_landmarks(), CV_32FC1);
        std::vector<int> st(ids.size());
        superviseddescent::hip::check(sdm_track_get(handle.get(), ids.data(), (int)ids.size(), rows.ptr<float>(0), st.data()), "sdm_track_get");
        return {collections(rows), st};
    }

    const std::vector<int>& lost() const { return last_lost; }
    const cv::Mat& rows() const { return last_rows; }
    /** The cascade's own rows of the last step (the same as rows() after a step without dt). */
    const cv::Mat& raw_rows() const { return last_raw; }
    sdm_ctx* context() const { return handle.get(); }

private:
    std::vector<LandmarkCollection<cv::Vec2f>> step_on_current_images(const std::vector<int>& ids, const std::vector<int>& image_index,
                                                                      const std::vector<float>* dt = nullptr)
    {
        using superviseddescent::hip::check;
        sdm_ctx* c = handle.get();
        const int n = (int)ids.size();
        check(sdm_set_templates(c, nullptr, 0, 0), "sdm_set_templates");
        if (image_index.empty()) check(sdm_set_sample_image_index(c, nullptr, 0), "sdm_set_sample_image_index");
        else check(sdm_set_sample_image_index(c, image_index.data(), (int)image_index.size()), "sdm_set_sample_image_index");
        cv::Mat rows(n, 2 * num_landmarks(), CV_32FC1);
        std::vector<int> masks(ids.size());
        if (dt) {
            if (dt->size() != ids.size()) throw std::runtime_error("tracker::step: one dt per stream id expected");
            cv::Mat raw(n, 2 * num_landmarks(), CV_32FC1);
            check(sdm_track_step_filtered(c, ids.data(), n, dt->data(), raw.ptr<float>(0), masks.data(), rows.ptr<float>(0)),
                  "sdm_track_step_filtered");
            last_raw = raw;
        } else {
            check(sdm_track_step(c, ids.data(), n, rows.ptr<float>(0), masks.data()), "sdm_track_step");
            last_raw = rows;
        }
        last_rows = rows;
        last_lost = masks;
        return collections(rows);
    }

    int num_landmarks() const { return (int)model.get_landmark_ids().size(); }
    std::vector<LandmarkCollection<cv::Vec2f>> collections(const cv::Mat& rows) const
    {
        std::vector<LandmarkCollection<cv::Vec2f>> out;
        for (int r = 0; r < rows.rows; ++r) out.push_back(to_landmark_collection(rows.row(r), model.get_landmark_ids()));
        return out;
    }

    detection_model& model;
    superviseddescent::hip::Handle handle;
    cv::Mat last_rows, last_raw;
    std::vector<int> last_lost;
};

}  // namespace rcr
#endif /* RCR_TRACKER_HPP_ */
