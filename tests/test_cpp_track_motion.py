"""rcr::tracker's motion-compensated initialisation (tests/cpp/track_motion_gpu.cpp): tracker::motion and tracker::last_motion give
the bits of the Python layer on the same model file and video -- the rows, the masks, every step's search results, and the slots'
grids and chips after the run."""
import os

import numpy as np
import pytest

import cpp_build as B


@pytest.mark.gpu
def test_cpp_motion_tracker_matches_python(built, tmp_path):
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, synth
    ids = ibug.RCR22_IDS
    L = len(ids)
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    d = str(tmp_path)
    R = B.write_model(d, L, params, mean, ids, seed=979)
    frames, _, boxes = synth.make_tracks(4, 4, seed=83, size=320, max_step=12.0)
    T, S, H, W = frames.shape
    motion = (8, 1.25, 0)
    frames.tofile(os.path.join(d, "frames.u8"))
    boxes.astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{S} {T} {H} {W} {S} {motion[0]} {motion[1]} {motion[2]}\n")
    B.run(B.gpu_driver("track_motion_gpu", tmp_path), [d], 300)
    # the same loop through the Python Tracker
    regs = [LinearRegressor() for _ in params]
    for r, x in zip(regs, R):
        r.x = x
    dm = detection_model(SupervisedDescentOptimiser(regs), mean, ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    tr = dm.tracker(S, motion=motion)
    sid = np.arange(S)
    have = np.zeros(S, bool)
    rows, masks, found = [], [], []
    for t in range(T):
        if (~have).any():
            tr.start(sid[~have], boxes[t][~have])
        res, lost = tr.step(sid, list(frames[t]))
        have = lost == 0
        rows.append(res)
        masks.append(lost)
        found.append(tr.motion(sid)[0])
    _, grids, chips = tr.motion(sid)
    rd = lambda name, kind: np.fromfile(os.path.join(d, name), kind)
    assert rd("cpp_landmarks.f32", np.uint32).tobytes() == np.stack(rows).tobytes()
    assert np.array_equal(rd("cpp_lost.i32", np.int32).reshape(T, S), np.stack(masks))
    assert np.array_equal(rd("cpp_motion.i32", np.int32).reshape(T, S, 6), np.stack(found))
    assert np.array_equal(rd("cpp_grids.i32", np.int32).reshape(S, 3), grids)
    assert np.array_equal(rd("cpp_chips.u8", np.uint8).reshape(S, 32, 32), chips)
    assert np.stack(found)[1:, :, 5].any() and chips.any()              # (the search was at work)
    dm.optimised_model.ctx.close()
