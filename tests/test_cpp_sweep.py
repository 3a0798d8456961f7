"""The regulariser sweep through the C++ header layer (tests/cpp/sweep_gpu.cpp): regressors constructed from a
superviseddescent::RegulariserSweep, trained with train(..., callback, holdout), against the Python layer on the same scenario --
the same kernels, so the same bytes."""
import os

import numpy as np
import pytest

import cpp_build as B


@pytest.mark.gpu
def test_cpp_sweep_scenario_matches_python_layer(built, tmp_path):
    from superviseddescent_amd import (HoGParam, HogTransform, LinearRegressor, RegulariserSweep, SupervisedDescentOptimiser, ibug,
                                       synth)
    ids = ["31", "37", "40", "43", "46", "49", "55"]
    params = [(1, 3, 12, 4, 0.9), (1, 3, 8, 4, 0.6)]
    candidates = [0.5, 1.5, 6.0, 40.0]
    holdout = 45
    images, boxes, gt = synth.make_faces(39, seed=1901)
    x_star, x0, idx = synth.make_samples(boxes, gt, ids, n_perturb=4, seed=1902)          # 195 rows
    d = str(tmp_path)
    images.tofile(d + "/images.u8"); x0.tofile(d + "/x0.f32"); x_star.tofile(d + "/xstar.f32")
    idx.astype(np.int32).tofile(d + "/img_index.i32")
    with open(d + "/meta.txt", "w") as f:
        f.write(f"{images.shape[0]} {images.shape[1]} {images.shape[2]} {x0.shape[0]} {len(ids)} {len(params)} {holdout}\n")
        for p in params:
            f.write(" ".join(str(v) for v in p) + "\n")
        f.write(" ".join(ids) + "\n" + " ".join(ibug.RIGHT_EYE_IDS) + "\n" + " ".join(ibug.LEFT_EYE_IDS) + "\n")
        f.write(f"1 1 {len(candidates)} " + " ".join(repr(c) for c in candidates) + "\n")
    B.run(B.gpu_driver("sweep_gpu", tmp_path), [d], 300)

    def rd(name):
        return np.fromfile(os.path.join(d, name), np.float32).reshape(-1, 2 * len(ids))

    sdo = SupervisedDescentOptimiser([LinearRegressor(RegulariserSweep(1, candidates, True)) for _ in params])
    hog = HogTransform(images, [HoGParam(*p) for p in params], ids, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx)
    x_train = sdo.train(x_star, x0, None, hog, holdout=holdout)
    assert rd("cpp_x_train.f32").tobytes() == x_train.tobytes()
    lines = open(d + "/cpp_sweep.txt").read().strip().splitlines()
    for l, reg in enumerate(sdo.regressors):
        assert rd(f"cpp_R{l}.f32").tobytes() == reg.x.tobytes(), l
        rec = lines[l].split()
        assert int(rec[0]) == reg.sweep["best"]
        vals = np.array([float(v) for v in rec[1:]]).reshape(len(candidates), 4)
        assert np.array_equal(vals[:, 0], reg.sweep["holdout_errors"]) and np.array_equal(vals[:, 1], reg.sweep["fit_errors"])
        assert np.array_equal(vals[:, 2].astype(np.float32), reg.sweep["lambdas"])
        assert np.array_equal(vals[:, 3].astype(np.int32), reg.sweep["status"])
    assert rd("cpp_x_test.f32").tobytes() == sdo.test(x0, None, hog).tobytes()
