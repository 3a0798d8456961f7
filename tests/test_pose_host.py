"""Head pose (ModelProjection of the reference's examples/pose_estimation.cpp) without a GPU: the Python and C++ host projections
against the float64 restatement (tests/pose_f64.py), the camera independence of the normalised coordinates, and the C-ABI's
pose entry points (declared, exported, bound)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cpp_build as B
import pose_f64 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float32 evaluation vs float64: max |error| per row / max |u, v| of the row.  Measured 1.5e-6 (Python, numpy's float32 sin / cos)
# on 2 000 random rows at +-30 and +-89 degrees; 3e-6 leaves about 2x margin.
REL_TOL = 3e-6
POSE_SYMBOLS = ["sdm_pose_set_model", "sdm_pose_set_x", "sdm_pose_get_x", "sdm_pose_set_x_device", "sdm_pose_set_templates",
                "sdm_pose_templates_from_landmarks", "sdm_pose_set_targets", "sdm_pose_features", "sdm_pose_train_level",
                "sdm_pose_set_regressor", "sdm_pose_get_regressor", "sdm_pose_test"]


def random_poses(n, limit, seed, t=(0.0, 0.0, -2000.0)):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 6), np.float32)
    x[:, :3] = rng.uniform(-limit, limit, (n, 3))
    x[:, 3:] = t
    return x


def edge_poses():
    """Every combination of 0 and +-89 degrees on the three axes."""
    v = np.array([-89.0, 0.0, 89.0], np.float32)
    g = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    x = np.zeros((g.shape[0], 6), np.float32)
    x[:, :3], x[:, 5] = g, -2000.0
    return x


def rel_err(y, ref):
    return np.abs(np.asarray(y, np.float64) - ref).max(1) / np.abs(ref).max(1)


def example_projection():
    from superviseddescent_amd import ModelProjection
    return ModelProjection(np.concatenate([P.EXAMPLE_POINTS.T, np.ones((1, 10), np.float32)]))


@pytest.mark.parametrize("poses", ["random30", "edge89", "random89_translated"])
def test_python_host_projection_matches_float64(poses):
    x = {"random30": lambda: random_poses(2000, 30, 1), "edge89": edge_poses,
         "random89_translated": lambda: random_poses(500, 89, 2, t=(40.0, -25.0, -1500.0))}[poses]()
    y = example_projection()(x)
    assert y.dtype == np.float32 and y.shape == (x.shape[0], 20)
    assert rel_err(y, P.project(x)).max() < REL_TOL
    # one row at a time (the reference's call shape, :305-309) gives the same row
    assert np.array_equal(example_projection()(x[3], 0), y[3:4])


def test_normalised_coordinates_do_not_depend_on_screen_or_clip_planes():
    from superviseddescent_amd import ModelProjection
    x = np.concatenate([random_poses(300, 30, 3), edge_poses()])
    pts = np.concatenate([P.EXAMPLE_POINTS.T, np.ones((1, 10), np.float32)])
    base = ModelProjection(pts)(x)
    for cam in [(1800.0, 640.0, 480.0, 1.0, 5000.0), (1800.0, 1920.0, 1080.0, 10.0, 3000.0), (1800.0, 300.0, 900.0, 0.1, 1e5)]:
        y = ModelProjection(pts, *cam)(x)
        assert rel_err(y, base.astype(np.float64)).max() < 2 * REL_TOL, cam
        assert rel_err(y, P.project(x, P.EXAMPLE_POINTS, *cam)).max() < REL_TOL, cam
    # (the focal length cancels as well: the field of view is derived from it, :46 -- u, v are the camera-space ratios X/-Z, Y/Z)
    assert rel_err(ModelProjection(pts, 900.0)(x), base.astype(np.float64)).max() < 2 * REL_TOL


@pytest.fixture(scope="module")
def pose_host_bin(built, tmp_path_factory):
    """tests/cpp/pose_host.cpp built with g++ and the flags of tests/cpp/Makefile into a temp dir."""
    return B.gpu_driver("pose_host", tmp_path_factory.mktemp("pose_cpp"))


def run_cpp_host(binary, tmp_path, x, points=P.EXAMPLE_POINTS, cam=(1800.0, 1000.0, 1000.0, 1.0, 5000.0)):
    f = tmp_path / "in.txt"
    lines = [str(len(points))] + ["%.9g %.9g %.9g" % tuple(p) for p in points] + ["%.9g %.9g %.9g %.9g %.9g" % cam, str(len(x))]
    lines += ["%.9g %.9g %.9g %.9g %.9g %.9g" % tuple(r) for r in x]
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([binary, str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return np.array([[float(v) for v in ln.split()] for ln in out.stdout.strip().splitlines()], np.float32)


def test_cpp_host_operator_matches_float64(pose_host_bin, tmp_path):
    x = np.concatenate([random_poses(400, 30, 4), edge_poses()])
    y = run_cpp_host(pose_host_bin, tmp_path, x)
    assert y.shape == (x.shape[0], 20)
    assert rel_err(y, P.project(x)).max() < REL_TOL
    cam = (1800.0, 640.0, 480.0, 2.0, 4000.0)
    y2 = run_cpp_host(pose_host_bin, tmp_path, x, cam=cam)
    assert rel_err(y2, P.project(x, P.EXAMPLE_POINTS, *cam)).max() < REL_TOL
    assert rel_err(y2, y.astype(np.float64)).max() < 2 * REL_TOL


def test_pose_entry_points_declared_and_exported(built):
    from superviseddescent_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sdm_pose_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(POSE_SYMBOLS)
    assert set(POSE_SYMBOLS) <= set(_lib.EXPORTED)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in POSE_SYMBOLS)
    bound = _lib.lib()
    assert all(getattr(bound, s).restype is ctypes.c_int and getattr(bound, s).argtypes for s in POSE_SYMBOLS)


def test_model_projection_argument_checks():
    from superviseddescent_amd import ModelProjection
    with pytest.raises(ValueError):
        ModelProjection(np.zeros((5, 10), np.float32))
    with pytest.raises(ValueError):
        ModelProjection(np.zeros((4, 65), np.float32))
    with pytest.raises(ValueError):
        example_projection()(np.zeros((1, 5), np.float32))
    assert example_projection().K == 10
