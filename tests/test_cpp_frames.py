"""The rcr::DeviceFrame overloads of the C++ header layer (tests/cpp/frames_gpu.cpp): detection_model::detect_batch and
tracker::step on BGR frames that are already on the device -- ragged sizes, odd pitches -- against the cv::Mat overloads on the same
pixels, and against the Python layer: the same kernels, so the same bytes."""
import os

import numpy as np
import pytest

import cpp_build as B


@pytest.mark.gpu
def test_cpp_device_frames_match_the_mat_overloads(built, tmp_path):
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, synth
    ids = ibug.RCR22_IDS
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
    d = str(tmp_path)
    rng = np.random.default_rng(1234)
    R = B.write_model(d, len(ids), params, mean, ids, seed=rng)              # (the colour channels below draw on behind the regressors)
    frames, _, boxes = synth.make_tracks(3, 2, seed=57)                      # frames x streams x H x W
    cut = ((slice(0, 230), slice(0, 256)), (slice(0, 256), slice(0, 241)), (slice(0, 199), slice(0, 233)))      # three sizes
    colour = []
    for t in range(2):
        row = []
        for s in range(3):
            g = frames[t, s][cut[s]]
            c = rng.integers(0, 256, g.shape + (3,), dtype=np.uint8)
            c[..., 1] = g
            row.append(c)
        colour.append(row)
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for row in colour:
            for c in row:
                f.write(c.tobytes())
    boxes[0].astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("3 2\n" + "".join(f"{c.shape[0]} {c.shape[1]}\n" for c in colour[0]))
    B.run(B.gpu_driver("frames_gpu", tmp_path), [d], 300)

    def rd(name):
        return np.fromfile(os.path.join(d, name), np.float32).reshape(3, 2 * len(ids))

    assert rd("detect_dev.f32").tobytes() == rd("detect_mat.f32").tobytes()
    assert rd("track_dev.f32").tobytes() == rd("track_mat.f32").tobytes()
    # the Python layer on the same frames, uploaded from the host
    regs = [LinearRegressor() for _ in params]
    for reg, r in zip(regs, R):
        reg.x = r
    model = detection_model(SupervisedDescentOptimiser(regs), mean, ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    assert rd("detect_dev.f32").tobytes() == model.detect_batch(colour[0], boxes[0]).tobytes()
    tr = model.tracker(3)
    tr.start(np.arange(3), boxes[0])
    tr.step(np.arange(3), colour[0])
    assert rd("track_dev.f32").tobytes() == tr.step(np.arange(3), colour[1])[0].tobytes()
    model.optimised_model.ctx.close()
