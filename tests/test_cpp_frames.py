"""The rcr::DeviceFrame overloads of the C++ header layer (tests/cpp/frames_gpu.cpp): detection_model::detect_batch and
tracker::step on BGR frames that are already on the device -- ragged sizes, odd pitches -- against the cv::Mat overloads on the same
pixels, and against the Python layer: the same kernels, so the same bytes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_frames_match_the_mat_overloads(built, tmp_path):
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, model_io, synth
    ids = ibug.RCR22_IDS
    mean = ibug.select_mean(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
    rng = np.random.default_rng(1234)
    R = [rng.normal(0, 3e-3, (len(ids) * p.patch_dim + 1, 2 * len(ids))).astype(np.float32) for p in params]
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
    d = str(tmp_path)
    model_io.save_detection_model(model_io.DetectionModelFile(
        [model_io.RegressorRecord(r, 1, 1.5, False) for r in R], mean, ids,
        [(p.vlhog_variant, p.num_cells, p.cell_size, p.num_bins, p.relative_patch_size) for p in params],
        ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS), os.path.join(d, "model.bin"))
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for row in colour:
            for c in row:
                f.write(c.tobytes())
    boxes[0].astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("3 2\n" + "".join(f"{c.shape[0]} {c.shape[1]}\n" for c in colour[0]))
    exe = str(tmp_path / "frames_gpu")
    lib = os.path.join(ROOT, "superviseddescent_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "superviseddescent_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "frames_gpu.cpp"), "-o", exe, "-L" + lib, "-lsdm_hip",
                           "-Wl,-rpath," + lib, "-lpthread", "-ldl"])
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr

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
