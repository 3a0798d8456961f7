// GPU test driver of rcr::region_masks (superviseddescent_amd/include/rcr/alignment.hpp; run by tests/test_cpp_region_mask.py on the
// MI355X box): the maps of landmark rows on rcr::DeviceFrame s of several formats -- once through the fit (the detection_model
// overload), once through the matrices that call returned and the rows' own points (the explicit overload).
//   usage: region_mask_gpu <dir>
//   <dir>/meta.txt      S crop_w crop_h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes
//   <dir>/region.txt    n_polygons n_holes grow feather, then per polygon (the holes last): hull size idx_0 ... idx_{size-1}
//   <dir>/model.bin     the detection model (rcr::save_detection_model layout)
//   <dir>/frames.u8     the frames' bytes, one after another (`bytes` each)
//   <dir>/rows.f32      S x 2L landmark rows          <dir>/tmpl.f32    K x 2 template points
// writes fit.u8 and at.u8 (S x crop_h x crop_w bytes each), mats.f32, flags.i32, flags_at.i32
#include "rcr/alignment.hpp"

#include "gpu_driver.hpp"

int main(int argc, char** argv)
{
    return driver_main(argc, argv, "region_mask_gpu", [](const std::string& dir) {
        const Scenario sc(dir + "/meta.txt");
        const int S = sc.S, cw = sc.w, ch = sc.h, K = (int)sc.lm.size();
        rcr::RegionMask region;
        {
            std::ifstream f(dir + "/region.txt");
            int n_polygons = 0, n_holes = 0;
            f >> n_polygons >> n_holes >> region.grow >> region.feather;
            for (int g = 0; g < n_polygons; ++g) {
                int hull = 0, size = 0;
                f >> hull >> size;
                std::vector<int> p((size_t)(size > 0 ? size : 0));
                for (int& v : p) f >> v;
                if (hull) region.hull.push_back(g);
                (g < n_polygons - n_holes ? region.polygons : region.holes).push_back(p);
            }
            if (!f || n_polygons < 1) throw std::runtime_error("cannot read region.txt");
        }
        rcr::detection_model model = rcr::load_detection_model(dir + "/model.bin");
        auto pixels = read_all<uint8_t>(dir + "/frames.u8");
        auto rows = read_all<float>(dir + "/rows.f32");
        auto tm = read_all<float>(dir + "/tmpl.f32");
        const int L = (int)model.get_landmark_ids().size();
        if ((int)rows.size() != S * 2 * L || (int)tm.size() != 2 * K) throw std::runtime_error("scenario size mismatch");
        DeviceMemory mem;
        std::vector<rcr::DeviceFrame> frames;
        size_t at = 0;
        for (int s = 0; s < S; ++s) {
            uint8_t* p = mem.upload(pixels.data() + at, (size_t)sc.bytes[s], (size_t)(s % 4));         // misalignment 0 ... 3
            at += (size_t)sc.bytes[s];
            frames.push_back(rcr::DeviceFrame{p, sc.W[s], sc.H[s], sc.stride[s], sc.fmt[s]});
        }
        cv::Mat x(S, 2 * L, CV_32FC1), tmpl(K, 2, CV_32FC1);
        std::memcpy(x.ptr<float>(0), rows.data(), rows.size() * 4);
        std::memcpy(tmpl.ptr<float>(0), tm.data(), tm.size() * 4);
        const size_t bytes = (size_t)S * cw * ch;
        std::vector<uint8_t> host(bytes);
        uint8_t* out_fit = mem.alloc(bytes);
        const rcr::region_masks_result fit = rcr::region_masks(model, frames, x, {}, sc.lm, tmpl, cw, ch, region, out_fit);
        mem.download(host.data(), out_fit, bytes);
        write_bytes(dir + "/fit.u8", host.data(), bytes);
        write_bytes(dir + "/flags.i32", fit.flags.data(), (size_t)S * 4);
        write_mat(dir + "/mats.f32", fit.matrices);
        // the explicit form: the rows' own points, one polygon after the other
        std::vector<int> verts;
        for (const auto* list : {&region.polygons, &region.holes})
            for (const auto& p : *list) verts.insert(verts.end(), p.begin(), p.end());
        cv::Mat points(S, 2 * (int)verts.size(), CV_32FC1);
        for (int s = 0; s < S; ++s)
            for (size_t k = 0; k < verts.size(); ++k) {
                points.at<float>(s, 2 * (int)k) = x.at<float>(s, verts[k]);
                points.at<float>(s, 2 * (int)k + 1) = x.at<float>(s, L + verts[k]);
            }
        uint8_t* out_at = mem.alloc(bytes);
        const rcr::region_masks_result again = rcr::region_masks(fit.matrices, points, cw, ch, region, out_at);
        mem.download(host.data(), out_at, bytes);
        write_bytes(dir + "/at.u8", host.data(), bytes);
        write_bytes(dir + "/flags_at.i32", again.flags.data(), (size_t)S * 4);
        std::printf("%d rows of %d x %d drawn twice\n", S, cw, ch);
        return 0;
    });
}
