"""Head pose on the device (csrc/sdm_pose.hip, include/sdm.h sdm_pose_*): the ModelProjection cascade of the reference's
examples/pose_estimation.cpp against the float64 restatement of its formulas (tests/pose_f64.py), its bit-level contracts
(fused vs level by level, batch independence, reproducible training), the detect -> pose hand-off and the C++ port of the
example's main."""
import numpy as np
import pytest

import cpp_build as B
import pose_f64 as P
from pose_cases import homogeneous, poses as random_poses, rel_err
from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, ModelProjection, Regulariser, SdmError,
                                   SupervisedDescentOptimiser, detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
MN = Regulariser.RegularisationType.MatrixNorm
# device float32 projection vs float64, max |error| per row / max |u, v| of the row (the host evaluation measures 1.5e-6)
FEAT_TOL = 6e-6
# the example end to end: predicted angles of the device cascade vs the float64 cascade trained on the same samples, degrees
PREDICT_TOL_DEG = 5e-3


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("K", [10, 64])
def test_device_features_match_float64(ctx, K):
    if K == 10:
        pts = P.EXAMPLE_POINTS
    else:
        pts = np.random.default_rng(7).uniform(-60, 60, (K, 3)).astype(np.float32)
    x = np.concatenate([random_poses(3000, 11), random_poses(500, 12, 89.0)])
    ctx.pose_set_model(pts)
    ctx.pose_set_x(x)
    f = ctx.pose_features()                                  # no templates for these rows: the projections themselves
    err = rel_err(f, P.project(x, pts)).max()
    print(f"K={K}: device features vs float64, max relative error {err:.3e}")
    assert err < FEAT_TOL
    t = ModelProjection(homogeneous(pts))(x)
    ctx.pose_set_templates(t)
    assert np.abs(ctx.pose_features()).max() < 1e-6          # features - templates of the host projection


@pytest.mark.parametrize("n", [500, 200_000])
def test_teacher_forced_training_levels(ctx, n):
    """Per level, the device and the float64 solve start from the SAME x_k (the device's); x_{k+1} compared relative to ||x*||."""
    x_star = random_poses(n, 21)
    y = ModelProjection(homogeneous(P.EXAMPLE_POINTS))(x_star)
    xk = np.tile(P.EXAMPLE_X0, (n, 1))
    ctx.pose_set_model(P.EXAMPLE_POINTS)
    for level in range(3):
        ctx.pose_set_x(xk)
        ctx.pose_set_templates(y)
        ctx.pose_set_targets(x_star)
        A32 = ctx.pose_features().astype(np.float64)          # the float32 rows the device's normal equations are formed from
        lam_rule = P.reference_lambda(A32.T @ A32, n, 1, 2.0)
        R, lam = ctx.pose_train_level(level, MN, 2.0, True)
        x_dev = ctx.pose_get_x()
        obs = P.project(xk, P.EXAMPLE_POINTS) - y
        R64, lam64 = P.solve_level(obs, xk.astype(np.float64) - x_star, 1, 2.0, True)
        x64 = xk - obs @ R64
        full = np.linalg.norm(x_dev - x64) / np.linalg.norm(x_star.astype(np.float64))
        ang = np.linalg.norm(x_dev[:, :3] - x64[:, :3]) / np.linalg.norm(x_star[:, :3].astype(np.float64))
        print(f"N={n} level {level}: lambda {lam:.7g} (rule on the device rows {lam_rule:.7g}, on float64 rows {lam64:.7g}), "
              f"x_k+1 rel. ||x*|| {full:.3e}, angles {ang:.3e}")
        # lambda: the reference's float rule on the same float32 rows, to the rounding of the norm's sum (at the last levels the rows
        # are residuals of 1e-6 and their float32 rounding moves lambda itself by ~1e-5 against float64 rows)
        assert abs(lam - lam_rule) <= 4e-7 * lam_rule
        # measured at N = 500: <= 1.7e-8 of ||x*||, <= 1.1e-6 of the angles' norm
        assert full < 1e-7 and ang < 1e-5
        assert np.array_equal(ctx.pose_get_regressor(level), R)
        xk = x_dev


def example_training(n=500, seed=31):
    x_star = random_poses(n, seed)
    proj = ModelProjection(homogeneous(P.EXAMPLE_POINTS))
    y = proj(x_star)
    x0 = np.tile(P.EXAMPLE_X0, (n, 1))
    return x_star, y, x0, proj


def example_optimiser():
    return SupervisedDescentOptimiser([LinearRegressor(Regulariser(MN, 2.0, True)) for _ in range(3)])


def test_example_end_to_end_predict(built):
    x_star, y, x0, proj = example_training()
    sdo = example_optimiser()
    residuals = []
    x_train = sdo.train(x_star, x0, y, proj, lambda x: residuals.append(np.linalg.norm(x - x_star) / np.linalg.norm(x_star)))
    assert len(residuals) == 3 and residuals[2] < residuals[1] < residuals[0] < 1e-3
    assert np.array_equal(x_train, sdo.ctx.pose_get_x())
    pred = sdo.predict(P.EXAMPLE_X0, P.example_templates(), proj)[0]
    Rs, _ = P.train(x_star, x0, y)
    ref = P.test(P.EXAMPLE_X0, P.example_templates(), Rs)[0]
    gt = np.array(P.EXAMPLE_GROUND_TRUTH)
    print(f"predicted {pred[:3]}, float64 {ref[:3]}, example ground truth {gt} (|device - gt| = {np.abs(pred[:3] - gt)})")
    assert np.abs(pred[:3] - ref[:3]).max() < PREDICT_TOL_DEG
    assert np.abs(pred[:3] - gt).max() < 1.0
    assert np.array_equal(pred[3:], P.EXAMPLE_X0[3:])       # b = 0 in the translation columns: R leaves them alone


def test_fused_cascade_is_bit_identical_to_levels_and_batches(built):
    x_star, y, x0, proj = example_training()
    sdo = example_optimiser()
    sdo.train(x_star, x0, y, proj)
    n = 100_000
    tgt = random_poses(n, 41, 35.0)
    tmpl = proj(tgt)
    init = np.tile(P.EXAMPLE_X0, (n, 1))
    init[:, :3] = np.random.default_rng(42).uniform(-5, 5, (n, 3))
    fused = sdo.test(init, tmpl, proj)
    seen = []
    levels = sdo.test(init, tmpl, proj, lambda x: seen.append(x))
    assert len(seen) == 3 and np.array_equal(seen[-1], levels)
    assert np.array_equal(fused, levels)
    assert np.array_equal(sdo.test(init[:17], tmpl[:17], proj), fused[:17])
    assert np.array_equal(sdo.test(init[50_001:50_018], tmpl[50_001:50_018], proj), fused[50_001:50_018])
    for i in (0, 5, n - 1):
        assert np.array_equal(sdo.predict(init[i], tmpl[i], proj)[0], fused[i])


def test_training_is_deterministic(built):
    x_star, y, x0, proj = example_training(20_000, 51)
    runs = []
    for _ in range(2):
        sdo = example_optimiser()
        xt = sdo.train(x_star, x0, y, proj)
        runs.append(([r.x.copy() for r in sdo.regressors], [r.last_lambda for r in sdo.regressors], xt))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


def test_detect_to_pose_on_the_device(built):
    ids = ibug.RCR22_IDS
    re, le = ibug.eye_indices(ids)
    images, boxes, gt = synth.make_faces(64, seed=303)
    x_star, x0, img_index = synth.make_samples(boxes, gt, ids, n_perturb=1, seed=304)
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS[:2]]
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(MN, 1.5, False)) for _ in params])
    sdo.train(x_star, x0, None, HogTransform(images, params, ids, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, img_index))
    dm = detection_model(sdo, ibug.select_mean(ids), ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    # images of different sizes (padding right / bottom, the faces stay where they are): every row has its own image centre
    padded = [np.pad(im, ((0, 8 * (i % 3)), (0, 16 * (i % 4))), mode="edge") for i, im in enumerate(images)]
    lms = dm.detect_batch(padded, boxes)
    n, L = lms.shape[0], len(ids)

    # nine of the example's ten points exist in RCR-22 (ibug 34 does not)
    keep = [i for i, lid in enumerate(P.EXAMPLE_IBUG_IDS) if lid in ids]
    pose_ids = [P.EXAMPLE_IBUG_IDS[i] for i in keep]
    assert len(pose_ids) == 9
    pts = P.EXAMPLE_POINTS[keep]
    focal = 1800.0
    idx = [ids.index(i) for i in pose_ids]
    hw = np.array([im.shape[1] for im in padded], np.float32)[:, None] / np.float32(2.0)
    hh = np.array([im.shape[0] for im in padded], np.float32)[:, None] / np.float32(2.0)
    host_tmpl = np.concatenate([(lms[:, idx] - hw) / np.float32(focal), (lms[:, [L + i for i in idx]] - hh) / np.float32(focal)], 1)

    # the gather itself: with every model point at the origin the projection is exactly 0, so the features are -templates
    c = sdo.ctx
    c.pose_set_model(np.zeros_like(pts), focal)
    c.pose_templates_from_landmarks(idx, focal)
    c.pose_set_x(np.tile(P.EXAMPLE_X0, (n, 1)))
    assert np.array_equal(-c.pose_features(), host_tmpl)

    # a pose cascade for the nine points, then the detect batch's poses without the landmarks leaving the device
    proj = ModelProjection(homogeneous(pts), focal)
    xs = random_poses(2000, 305)
    pose_sdo = example_optimiser()
    pose_sdo.train(xs, np.tile(P.EXAMPLE_X0, (2000, 1)), proj(xs), proj)
    poses = dm.estimate_pose(pose_sdo, proj, pose_ids, focal)
    assert poses.shape == (n, 6) and np.isfinite(poses).all()
    assert np.array_equal(poses, pose_sdo.test(np.tile(P.EXAMPLE_X0, (n, 1)), host_tmpl, proj))
    # any subset the user has 3D coordinates for
    sub = ModelProjection(homogeneous(pts[:5]), focal)
    sub_sdo = example_optimiser()
    sub_sdo.train(xs, np.tile(P.EXAMPLE_X0, (2000, 1)), sub(xs), sub)
    p5 = dm.estimate_pose(sub_sdo, sub, pose_ids[:5], focal)
    assert np.array_equal(p5, sub_sdo.test(np.tile(P.EXAMPLE_X0, (n, 1)), host_tmpl[:, [0, 1, 2, 3, 4, 9, 10, 11, 12, 13]], sub))
    with pytest.raises(ValueError):
        dm.estimate_pose(pose_sdo, proj, ["31", "34"] + pose_ids[2:], focal)     # ibug 34 is not an RCR-22 landmark


def test_invalid_sizes_and_singular_system(ctx):
    def code(fn, *a):
        with pytest.raises(SdmError) as e:
            fn(*a)
        return e.value.code
    assert code(ctx.pose_set_model, np.zeros((0, 3), np.float32)) == -1
    assert code(ctx.pose_set_model, np.zeros((65, 3), np.float32)) == -1
    ctx.pose_set_model(np.zeros((64, 3), np.float32))
    ctx.pose_set_model(P.EXAMPLE_POINTS)                     # (a different K drops the regressors of earlier tests)
    assert code(ctx.pose_set_x, np.zeros((0, 6), np.float32)) == -1
    x = random_poses(3, 61)
    ctx.pose_set_x(x)
    assert code(ctx.pose_set_templates, np.zeros((3, 18), np.float32)) == -1
    ctx.pose_set_templates(ModelProjection(homogeneous(P.EXAMPLE_POINTS))(x))
    ctx.pose_set_targets(x)
    assert code(ctx.pose_train_level, 16, 0, 0.0, True) == -1
    assert code(ctx.pose_test, 0, 1) == -1                   # no regressor yet
    R, lam = ctx.pose_train_level(0, 0, 0.0, True)           # 3 rows, 20 unknowns, no regularisation: singular, not an error
    assert lam == 0.0 and R.shape == (20, 6)
    assert code(ctx.pose_test, 0, 0) == -1
    assert code(ctx.pose_test, 0, 17) == -1
    assert code(ctx.pose_test, 15, 2) == -1
    assert code(ctx.pose_set_regressor, 16, np.zeros((20, 6), np.float32)) == -1
    assert code(ctx.pose_templates_from_landmarks, list(range(9)), 1800.0) == -1   # K differs from the model's


def test_cpp_port_of_the_example(built, tmp_path):
    samples = str(tmp_path / "x_tr.txt")
    out = B.run(B.gpu_driver("pose_estimation_gpu", tmp_path), [samples], 300)
    lines = out.stdout.strip().splitlines()
    residuals = [float(v) for v in lines[1:4]]
    assert residuals[2] < residuals[0] < 1e-3
    pred = [float(v.split("=")[1].split(",")[0]) for v in lines[-1].split(":")[1].split(",")[:3]]
    x_tr = np.loadtxt(samples, dtype=np.float32)
    x0 = np.tile(P.EXAMPLE_X0, (len(x_tr), 1))
    Rs, _ = P.train(x_tr, x0, ModelProjection(homogeneous(P.EXAMPLE_POINTS))(x_tr))
    ref = P.test(P.EXAMPLE_X0, P.example_templates(), Rs)[0]
    assert np.abs(np.array(pred) - ref[:3]).max() < PREDICT_TOL_DEG
