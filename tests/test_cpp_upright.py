"""rcr::detection_model::detect_batch_upright and rcr::tracker's upright mode (tests/cpp/upright_gpu.cpp): rolled boxes on three frames
of different sizes give the bits of the Python layer -- the same kernels behind the same C-ABI."""
import os

import numpy as np
import pytest

import cpp_build as B


@pytest.mark.gpu
def test_cpp_upright_matches_python(built, tmp_path):
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug
    ids = ibug.RCR22_IDS
    L = len(ids)
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    d = str(tmp_path)
    rng = np.random.default_rng(4321)
    R = B.write_model(d, L, params, mean, ids, seed=rng)                 # (the frames below draw on behind the regressors)
    sizes = [(160, 120), (97, 131), (64, 64)]                            # (width, height)
    T, chip, guard = 4, 97, 12
    frames = [[rng.integers(0, 256, (h, w), dtype=np.uint8) for w, h in sizes] for _ in range(T)]
    boxes = np.array([[40, 30, 50, 50], [-20, 40, 60, 64], [10, 12, 40, 40]], np.int32)
    rolls = np.array([17.3, -90.0, 135.0], np.float32)
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for fs in frames:
            for im in fs:
                f.write(im.tobytes())
    boxes.tofile(os.path.join(d, "boxes.i32"))
    rolls.tofile(os.path.join(d, "rolls.f32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"3 {T} {chip} {guard}\n" + "".join(f"{w} {h}\n" for w, h in sizes))
    B.run(B.gpu_driver("upright_gpu", tmp_path), [d], 300)
    # the Python layer on the same bytes
    regs = [LinearRegressor() for _ in params]
    for r, x in zip(regs, R):
        r.x = x
    dm = detection_model(SupervisedDescentOptimiser(regs), mean, ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    x = dm.detect_batch(frames[0], boxes, roll=rolls, chip=chip, guard=guard)
    M, flags = dm.upright_info()
    assert rd("cpp_detect.f32", np.uint32).tobytes() == x.tobytes()
    assert rd("cpp_mats.f32", np.uint32).tobytes() == M.tobytes() and np.array_equal(rd("cpp_flags.i32", np.int32), flags)
    tr = dm.tracker(3, init="upright", chip=chip, guard=guard)
    tr.start([0, 1, 2], boxes, roll=rolls)
    lms, masks = [], []
    for t in range(T):
        res, lost = tr.step([0, 1, 2], frames[t])
        lms.append(res)
        masks.append(lost)
        if lost.any():
            tr.start(np.arange(3)[lost != 0], boxes[lost != 0], roll=rolls[lost != 0])
    assert rd("cpp_track.f32", np.uint32).tobytes() == np.stack(lms).tobytes()
    assert np.array_equal(rd("cpp_lost.i32", np.int32).reshape(T, 3), np.stack(masks))
