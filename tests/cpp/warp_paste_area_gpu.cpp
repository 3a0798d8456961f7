// GPU test driver of the rcr::paste_warped_tensor overloads that take an rcr::AlignFilter (superviseddescent_amd/include/rcr/warp.hpp;
// run by tests/test_cpp_warp_paste_area.py on the MI355X box): a float16 NCHW RGB tensor with mean / std and a per-row opacity map pasted
// with area-averaged sampling into rcr::DeviceFrame s of format NV12 -- the UV plane directly behind Y (chroma nullptr) or in an
// allocation of its own -- and BGR in ONE list, each pass into a fresh copy of the frames: through the fit of landmark rows (the
// detection_model overload), through those rows' mesh landmarks (the explicit overload), and through the explicit overload with its
// defaulted chroma (every UV plane behind its Y plane) and no samples vector; and through the tracker's overload: a tracker started on
// the given boxes and stepped once on a copy of the frames, its rows pasted into another fresh copy.
//   usage: warp_paste_area_gpu <dir>
//   <dir>/meta.txt      S crop_w crop_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes_plane0 bytes_uv separate
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another: plane 0, then the UV plane
//   <dir>/rows.f32      S x 2L landmark rows          <dir>/tmpl.f32    K x 2 template points (triangles: their Delaunay triangulation)
//   <dir>/tensor.f16    S x 3 x crop_h x crop_w       <dir>/alpha.u8    S x crop_h x crop_w
//   <dir>/boxes.i32     S x 4: the tracker's start boxes, stream s on frame s
// writes fit.u8, at.u8, behind.u8 and track.u8 (the frames' bytes after each paste), mats.f32, flags.i32, flags_at.i32, samples.i32,
// samples_at.i32, and the tracker's track_rows.f32 (S x 2L), track_flags.i32, track_samples.i32
#include "rcr/warp.hpp"

#include "gpu_driver.hpp"

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "warp_paste_area_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt", 2);                                    // tail: bytes_uv separate
        const int S = sc.S, cw = sc.w, ch = sc.h, K = (int)sc.lm.size();
        const std::vector<int>& lm = sc.lm;
        const std::vector<int>& bytes = sc.bytes;
        std::vector<int> uv_bytes(S), separate(S);
        for (int s = 0; s < S; ++s) { uv_bytes[s] = sc.tail[s][0]; separate[s] = sc.tail[s][1]; }
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        auto tm = read_all<float>(dir + "/tmpl.f32");
        auto tensor = read_all<uint8_t>(dir + "/tensor.f16");
        auto alpha = read_all<uint8_t>(dir + "/alpha.u8");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L || (int)tm.size() != 2 * K || tensor.size() != (size_t)S * 3 * cw * ch * 2 || alpha.size() != (size_t)S * cw * ch)
            throw std::runtime_error("scenario size mismatch");
        DeviceMemory mem;
        const uint8_t* in_dev = mem.upload(tensor.data(), tensor.size());
        const rcr::PasteMask mask{mem.upload(alpha.data(), alpha.size()), true};
        cv::Mat x(S, 2 * L, CV_32FC1), tmpl(K, 2, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        std::memcpy(tmpl.ptr<float>(0), tm.data(), tm.size() * 4);
        rcr::TensorSpec spec;                                                       // float16, NCHW, RGB
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
        for (int c = 0; c < 3; ++c) { spec.scale[c] = sd[c]; spec.bias[c] = mean[c]; }
        const rcr::WarpMesh mesh = rcr::WarpMesh::of_template(lm, tmpl, cw, ch);
        cv::Mat points(S, 2 * K, CV_32FC1);
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < K; ++k) {
                points.at<float>(s, 2 * k) = x.at<float>(s, lm[k]);
                points.at<float>(s, 2 * k + 1) = x.at<float>(s, L + lm[k]);
            }
        rcr::warp_paste_result fit;
        const rcr::AlignFilter filter;                                              // area, at most 16 sub-samples per axis, min_scale 1
        std::vector<int> samples;
        auto boxes = read_all<int>(dir + "/boxes.i32");
        if ((int)boxes.size() != 4 * S) throw std::runtime_error("one box per stream expected");
        rcr::tracker tr(model, S);
        const char* names[4] = {"/fit.u8", "/at.u8", "/behind.u8", "/track.u8"};
        for (int pass = 0; pass < 4; ++pass) {
            std::vector<rcr::DeviceFrame> frames;
            std::vector<void*> chroma;
            size_t at = 0;
            for (int s = 0; s < S; ++s) {
                // planes that lie together: one allocation, misaligned by 0 ... 3; a separate UV plane: its own, misaligned by 1 ... 4 mod 4
                // (pass 2: every frame's planes together)
                const bool apart = separate[s] && pass != 2;
                uint8_t* p = mem.upload(pixels.data() + at, (size_t)bytes[s] + (apart ? 0 : (size_t)uv_bytes[s]), (size_t)(s % 4));
                uint8_t* uv = apart ? mem.upload(pixels.data() + at + bytes[s], (size_t)uv_bytes[s], (size_t)((s + 1) % 4)) : nullptr;
                at += (size_t)bytes[s] + (size_t)uv_bytes[s];
                frames.push_back(rcr::DeviceFrame{p, sc.W[s], sc.H[s], sc.stride[s], sc.fmt[s]});
                chroma.push_back(uv);
            }
            rcr::warp_paste_result res;
            if (pass == 0) res = fit = rcr::paste_warped_tensor(model, frames, chroma, x, {}, mesh, spec, filter, in_dev, mask, &samples);
            else if (pass == 1) res = rcr::paste_warped_tensor(model, points, {}, mesh, spec, filter, in_dev, frames, chroma, mask, &samples);
            else if (pass == 2) res = rcr::paste_warped_tensor(model, points, {}, mesh, spec, filter, in_dev, frames, std::vector<void*>{}, mask);
            else {
                // the tracker steps on frames of its own (the step reads them in place), then pastes its rows into this pass's copy
                std::vector<rcr::DeviceFrame> seen;
                size_t from = 0;
                for (int s = 0; s < S; ++s) {
                    seen.push_back(rcr::DeviceFrame{mem.upload(pixels.data() + from, (size_t)bytes[s] + (size_t)uv_bytes[s], (size_t)(s % 4)), sc.W[s],
                                                    sc.H[s], sc.stride[s], sc.fmt[s]});
                    from += (size_t)bytes[s] + (size_t)uv_bytes[s];
                }
                std::vector<int> ids(S);
                std::vector<cv::Rect> b0;
                for (int s = 0; s < S; ++s) { ids[s] = s; b0.push_back(cv::Rect(boxes[4 * s], boxes[4 * s + 1], boxes[4 * s + 2], boxes[4 * s + 3])); }
                tr.start(ids, b0);
                tr.step(ids, seen);
                res = rcr::paste_warped_tensor(tr, mesh, spec, filter, in_dev, frames, chroma, mask, &samples);
                write_bytes(dir + "/track_rows.f32", tr.rows().ptr<float>(0), (size_t)S * 2 * L * 4);
                write_bytes(dir + "/track_flags.i32", res.flags.data(), (size_t)S * 4);
                write_bytes(dir + "/track_samples.i32", samples.data(), samples.size() * 4);
            }
            if (pass < 2 && samples.size() != (size_t)S * mesh.n_triangles() * 2) throw std::runtime_error("samples: rows x T x 2 expected");
            if (pass < 2) write_bytes(dir + (pass == 0 ? "/samples.i32" : "/samples_at.i32"), samples.data(), samples.size() * 4);
            std::vector<uint8_t> host(pixels.size());
            at = 0;
            for (int s = 0; s < S; ++s) {
                const bool apart = separate[s] && pass != 2;
                const size_t n0 = (size_t)bytes[s] + (apart ? 0 : (size_t)uv_bytes[s]);
                mem.download(host.data() + at, frames[s].data, n0);
                if (apart) mem.download(host.data() + at + n0, chroma[s], (size_t)uv_bytes[s]);
                at += (size_t)bytes[s] + (size_t)uv_bytes[s];
            }
            write_bytes(dir + names[pass], host.data(), host.size());
            if (pass < 2) write_bytes(dir + (pass == 0 ? "/flags.i32" : "/flags_at.i32"), res.flags.data(), (size_t)S * 4);
        }
        // a filter the library refuses comes back as an exception
        bool refused = false;
        try {
            rcr::AlignFilter bad;
            bad.max_samples = 17;
            rcr::paste_warped_tensor(model, points, {}, mesh, spec, bad, in_dev, std::vector<rcr::DeviceFrame>(1, rcr::DeviceFrame{nullptr, 2, 2, 6, SDM_FRAME_BGR}));
        } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::runtime_error("max_samples = 17 was accepted");
        write_bytes(dir + "/mats.f32", fit.matrices.ptr<float>(0), (size_t)S * 6 * mesh.n_triangles() * 4);
        std::printf("%d rows of %d x %d pasted four times\n", S, cw, ch);
        return 0;
    });
}
