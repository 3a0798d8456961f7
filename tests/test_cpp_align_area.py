"""The rcr::aligned_crops_tensor overload with an rcr::AlignFilter (tests/cpp/align_area_gpu.cpp): landmark rows of several scales on two
ragged BGR DeviceFrames and one NV12 frame give the bytes and the S of the Python layer -- the same kernels behind the same C-ABI."""
import os

import numpy as np
import pytest

import align_area_cases as C
import align_area_ref as AR
import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B


@pytest.mark.gpu
def test_cpp_area_crops_match_python(built, tmp_path):
    import torch
    from superviseddescent_amd import Context, HoGParam, _lib, ibug
    ids = ibug.RCR22_IDS
    L = len(ids)
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    d = str(tmp_path)
    rng = np.random.default_rng(4321)
    B.write_model(d, L, params, mean, ids, seed=rng)                     # (the similarities below draw on behind the regressors)
    buf, frames = K.place([(37, 29, T.BGR), (64, 48, T.BGR), (7, 5, T.NV12)], 13)
    lm = [3, 6, 9, 12, 15]
    w, h = 7, 7
    tmpl = (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1, h - 1)).astype(np.float32)
    sims = [C.similarity(f, w, h, s, rng) for f, s in zip(frames, (1.7, 4.5, 2.6))]
    x = K.landmark_rows(sims, tmpl, lm, L)
    sizes = []
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for fr in frames:
            n = fr["h"] * fr["stride"] + (((fr["h"] + 1) // 2) * fr["stride"] if fr["fmt"] == T.NV12 else 0)
            sizes.append(n)
            f.write(buf[fr["off"]:fr["off"] + n].tobytes())
    x.tofile(os.path.join(d, "rows.f32"))
    tmpl.tofile(os.path.join(d, "tmpl.f32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"3 {w} {h} {len(lm)} " + " ".join(map(str, lm)) + "\n")
        f.write("".join(f"{fr['fmt']} {fr['w']} {fr['h']} {fr['stride']} {n}\n" for fr, n in zip(frames, sizes)))
    B.run(B.gpu_driver("align_area_gpu", tmp_path), [d], 300)
    # the Python layer on the same bytes
    c = Context(0)
    try:
        re_, le_ = ibug.eye_indices(ids)
        c.set_model_geometry(L, re_, le_, params)
        dev = torch.from_numpy(buf).cuda()
        lst = B.device_frames(dev, frames)
        c.set_frames_device(lst)
        c.set_sample_image_index(None)
        c.set_x(x)
        c.align_set_source_frames(lst)
        f16, mats, flags, samples = c.align_crops_tensor(lm, tmpl, w, h, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375],
                                                         filter="area")
        u8, _, _, capped = c.align_crops_tensor(lm, tmpl, w, h, dtype="uint8", layout="nhwc", order="bgr",
                                                filter=_lib.align_filter("area", max_samples=2))
        assert list(samples) == [2, 5, 3] and list(capped) == [2, 2, 2]
        rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
        assert rd("f16.bin", np.uint16).tobytes() == f16.cpu().numpy().tobytes()
        assert rd("u8.bin", np.uint8).tobytes() == u8.cpu().numpy().tobytes()
        assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes() and np.array_equal(rd("flags.i32", np.int32), flags)
        assert np.array_equal(rd("samples.i32", np.int32), samples) and np.array_equal(rd("samples_u8.i32", np.int32), capped)
        # and both are the restatement's
        host = [K.host_frame(buf, fr) for fr in frames]
        for r in range(3):
            want = AR.tensor(host[r], mats[r], w, h, 2, dtype="uint8", layout="nhwc", order="bgr")
            assert np.array_equal(u8[r].cpu().numpy(), want)
    finally:
        c.close()
