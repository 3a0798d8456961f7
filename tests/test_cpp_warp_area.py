"""The rcr::warped_crops_tensor overloads that take an rcr::AlignFilter (superviseddescent_amd/include/rcr/warp.hpp,
tests/cpp/warp_area_gpu.cpp): landmark rows on the gray, BGR, RGBA and NV12 DeviceFrames of the filtered warp's device tests give the
bytes, matrices, flags and samples of the Python layer on the same rows and frames -- the same kernels behind the same C-ABI."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import warp_area_cases as C
import warp_area_ref as WA


@pytest.mark.gpu
def test_cpp_filtered_warped_crops_match_python(built, tmp_path):
    import torch
    from superviseddescent_amd import Context, HoGParam, align_filter, ibug
    ids, L, mean = C.IDS, C.L, C.MEAN
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = C.place()
    w, h = C.CROPS[1]
    idx, tmpl, tri = C.MESHES["rcr22"](w, h)
    x = C.rows_for(frames, range(4), idx, tmpl, w, h, C.SEED, scales=[2.6, 1.7, 4.2, 3.3])
    d = str(tmp_path)
    B.write_model(d, L, params, mean, ids)
    meta = [f"4 {w} {h} {len(idx)} " + " ".join(map(str, idx)) + "\n"]
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for fr in frames:
            end = (fr["uv_off"] + ((fr["h"] + 1) // 2) * fr["stride"]) if fr["fmt"] == T.NV12 else fr["off"] + fr["h"] * fr["stride"]
            f.write(buf[fr["off"]:end].tobytes())
            meta.append(f"{fr['fmt']} {fr['w']} {fr['h']} {fr['stride']} {end - fr['off']} {fr['uv_off'] - fr['off'] if fr['fmt'] == T.NV12 else -1}\n")
    x.tofile(os.path.join(d, "rows.f32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("".join(meta))
    B.run(B.gpu_driver("warp_area_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    c = Context(0)
    try:
        re_, le_ = ibug.eye_indices(ids)
        c.set_model_geometry(L, re_, le_, params)
        dev = torch.from_numpy(buf).cuda()
        lst, chroma = B.device_frames(dev, frames), B.device_chroma(dev, frames)
        c.set_frames_device(lst)
        c.set_sample_image_index(None)
        c.set_x(x)
        c.align_set_source_frames(lst, chroma=chroma)
        c.warp_set_mesh(idx, tmpl, tri, w, h)
        f16, mats, flags, smp = c.warp_crops_tensor(filter="area", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
        capped = align_filter("area", 3, 2.0)
        u8, _, _, smp_u8 = c.warp_crops_tensor(filter=capped, dtype="uint8", layout="nhwc", order="bgr")
        lab = c.warp_labels()
        assert (smp > 3).any() and len({tuple(p) for p in smp.reshape(-1, 2)}) >= 4 and smp_u8.max() == 3
        assert rd("f16.bin", np.uint16).tobytes() == f16.cpu().numpy().tobytes()
        assert rd("u8.bin", np.uint8).tobytes() == u8.cpu().numpy().tobytes()
        assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes() and np.array_equal(rd("flags.i32", np.int32), flags)
        assert np.array_equal(rd("labels.u8", np.uint8).reshape(h, w), lab)
        assert np.array_equal(rd("samples.i32", np.int32).reshape(smp.shape), smp)
        assert np.array_equal(rd("samples_u8.i32", np.int32).reshape(smp.shape), smp_u8)
        # and both are the restatement's
        host = [K.host_frame(buf, fr) for fr in frames]
        for r in range(4):
            m = mats[r].reshape(-1, 6)
            want_s = WA.samples(m, False, capped.mode, capped.max_samples, capped.min_scale)
            assert np.array_equal(smp_u8[r], want_s)
            want = WA.tensor(host[r], m, lab, want_s, dtype="uint8", layout="nhwc", order="bgr")
            assert np.array_equal(u8[r].cpu().numpy(), want)
    finally:
        c.close()
