"""rcr::warped_crops_tensor (superviseddescent_amd/include/rcr/warp.hpp, tests/cpp/warp_gpu.cpp): landmark rows on the gray, BGR, RGBA and
NV12 DeviceFrames of the device tests give the bytes of the Python layer on the same rows and frames -- the same kernels behind the
same C-ABI --, and rcr::WarpMesh::of_mean is the Python layer's default mesh."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import warp_cases as W
import warp_ref as R


@pytest.mark.gpu
def test_cpp_warped_crops_match_python(built, tmp_path):
    import torch
    from superviseddescent_amd import Context, HoGParam, ibug
    ids, L, mean = W.IDS, W.L, W.MEAN
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = W.place()
    w, h = W.CROPS[1]
    idx, tmpl, tri = W.mesh_rcr22(w, h)
    x = W.rows_for(frames, range(4), idx, tmpl, w, h, 21)
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
    B.run(B.gpu_driver("warp_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    # the C++ layer's default mesh is the Python layer's
    assert rd("tmpl.f32", np.uint32).tobytes() == tmpl.tobytes() and np.array_equal(rd("tri.i32", np.int32).reshape(-1, 3), tri)
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
        f16, mats, flags = c.warp_crops_tensor(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
        u8, _, _ = c.warp_crops_tensor(dtype="uint8", layout="nhwc", order="bgr")
        lab = c.warp_labels()
        assert rd("f16.bin", np.uint16).tobytes() == f16.cpu().numpy().tobytes()
        assert rd("u8.bin", np.uint8).tobytes() == u8.cpu().numpy().tobytes()
        assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes() and np.array_equal(rd("flags.i32", np.int32), flags)
        assert np.array_equal(rd("labels.u8", np.uint8).reshape(h, w), lab)
        # and both are the restatement's
        host = [K.host_frame(buf, fr) for fr in frames]
        for r in range(4):
            want = R.tensor(host[r], mats[r].reshape(-1, 6), lab, dtype="uint8", layout="nhwc", order="bgr")
            assert np.array_equal(u8[r].cpu().numpy(), want)
    finally:
        c.close()
