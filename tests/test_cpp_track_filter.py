"""rcr::tracker's temporal landmark filter (tests/cpp/track_filter_gpu.cpp): tracker::smooth and the step overloads that take dt --
a vector, one value, cv::Mat and DeviceFrame frame lists -- give the bits of the Python layer on the same model file and video: the
filtered rows, the raw rows, the masks, and the slots' filter state after the run."""
import os

import numpy as np
import pytest

import cpp_build as B


@pytest.mark.gpu
def test_cpp_filtered_tracker_matches_python(built, tmp_path):
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, synth
    ids = ibug.RCR22_IDS
    L = len(ids)
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    d = str(tmp_path)
    R = B.write_model(d, L, params, mean, ids, seed=977)
    frames, _, boxes = synth.make_tracks(6, 12, seed=81)
    frames = frames.copy()
    frames[5, 2] = frames[5, 2][:, ::-1] // 2                          # a frame that is not stream 2's: it may be lost and restarted
    T, S, H, W = frames.shape
    smooth = (1.0, 5.0, 1.5)
    dt = np.random.default_rng(978).uniform(1 / 120, 1 / 10, (T, S)).astype(np.float32)
    frames.tofile(os.path.join(d, "frames.u8"))
    boxes.astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    dt.tofile(os.path.join(d, "dt.f32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{S} {T} {H} {W} {S} {smooth[0]} {smooth[1]} {smooth[2]}\n")
    B.run(B.gpu_driver("track_filter_gpu", tmp_path), [d], 300)
    # the same loop through the Python Tracker
    regs = [LinearRegressor() for _ in params]
    for r, x in zip(regs, R):
        r.x = x
    dm = detection_model(SupervisedDescentOptimiser(regs), mean, ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    tr = dm.tracker(S, smooth=smooth)
    sid = np.arange(S)
    have = np.zeros(S, bool)
    filt, raws, masks = [], [], []
    for t in range(T):
        if (~have).any():
            tr.start(sid[~have], boxes[t][~have])
        out, lost, raw = tr.step(sid, list(frames[t]), dt=dt[t, 0] if t % 3 == 0 else dt[t])
        have = lost == 0
        filt.append(out)
        raws.append(raw)
        masks.append(lost)
    rows, deriv, primed = tr.get_filtered(sid)
    rd = lambda name, kind: np.fromfile(os.path.join(d, name), kind)
    assert rd("cpp_filtered.f32", np.uint32).tobytes() == np.stack(filt).tobytes()
    assert rd("cpp_raw.f32", np.uint32).tobytes() == np.stack(raws).tobytes()
    assert np.array_equal(rd("cpp_lost.i32", np.int32).reshape(T, S), np.stack(masks))
    assert rd("cpp_state.f32", np.uint32).tobytes() == np.concatenate([rows, deriv]).tobytes()
    assert np.array_equal(rd("cpp_primed.i32", np.int32), primed)
    assert (np.stack(filt) != np.stack(raws)).any(axis=2).sum() >= T * S // 2        # (the filter was at work)
    dm.optimised_model.ctx.close()
