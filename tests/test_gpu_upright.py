"""Upright-normalised detect and tracking on the device (csrc/sdm_upright.hip, include/sdm.h "Rolled faces"): the chips, matrices and
flags against their host restatement (tests/upright_ref.py), every upright call against plain detect_batch on the restated chips
mapped back, row independence at 4 096 rows, the tracker's upright steps, the argument limits, and the accuracy on rolled faces."""
import numpy as np
import pytest

import align_ref as A
import pose_f64 as P
import track_ref as T
import upright_cases as C
from upright_cases import BOXES, IDX, ROLLS, ragged_frames
import upright_ref as U
from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, ModelProjection, Regulariser, SdmError,
                                   SupervisedDescentOptimiser, detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
MIN_SIZE, MAX_SCALE = 8.0, 1.5
INVALID = -1
# Upright detect of a face rolled by 10 ... 180 degrees against plain detect of the same face unrolled: at most 1.00 on the CPU
# oracle (0.0226 - 0.0233 against 0.0233); the bound is the one the feature was specified with.  Measured on the MI355X: 0.964 - 1.009
# (0.0209 - 0.0219 against 0.0217).
DETECT_RATIO = 1.15
# plain detect_batch from the box of a face rolled by 30 degrees is at least this much worse than the upright path (CPU oracle: 15 x;
# measured on the MI355X: 17.0 x, 0.3592 against 0.0211)
PLAIN_WORSE = 5.0
# the worst frame of 36 (faces turning 2.5 degrees per frame) against frame 0's detect error: 1.16 on the CPU oracle (0.0262 against
# 0.0226); the margin covers another seed's noise.  Measured on the MI355X: 1.165 (0.0255 against 0.0219), no stream lost.
TRACK_RATIO = 1.35


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def make_model(regs, params):
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


@pytest.fixture(scope="module")
def rmodel(built):
    """one level, random regressor: the bit-exact tests need a cascade, not a good one"""
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    rng = np.random.default_rng(4321)
    regs = [LinearRegressor() for _ in params]
    for r, p in zip(regs, params):
        r.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
    return make_model(regs, params)


def trained(images, boxes, gt, seed):
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=3, seed=seed)
    regs = [LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in params]
    sdo = SupervisedDescentOptimiser(regs)
    sdo.train(x_star, x0, None, HogTransform(images, params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, MEAN, IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def hog(dm, images, idx=None):
    return HogTransform(images, dm.hog_params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx)


def detect_from(dm, init, images, idx=None):
    return dm.optimised_model.test(np.asarray(init, np.float32), None, hog(dm, images, idx))


def restated(dm, grays, idx, M, init, chip):
    """what an upright call must equal: plain detect on the host-restated chips from `init`, and that mapped back through M"""
    chips = np.stack([U.chips(grays[i], m, chip) for i, m in zip(idx, M)])
    q = detect_from(dm, init, list(chips))
    return chips, q, U.back(M, q)


@pytest.mark.parametrize("chip", [32, 64, 97])
def test_chips_matrices_flags_and_detect_on_the_chips(rmodel, chip):
    from oracle import sdm_oracle as orc
    frames, grays, keep = ragged_frames()
    guard = chip // 8
    c = rmodel.optimised_model.ctx
    res = rmodel.detect_batch(frames, BOXES, IDX, roll=ROLLS, chip=chip, guard=guard)
    M, flags, chips = c.upright_get(chips=True)
    M2, flags2 = rmodel.upright_info()
    assert np.array_equal(bits(M), bits(M2)) and np.array_equal(flags, flags2)
    grays[3] = c.download_image(3)                                    # the gray of the colour frame is the context's conversion
    b, g, r = (np.asarray(keep[3].cpu().numpy()[..., k], np.int64) for k in range(3))
    assert np.array_equal(grays[3], ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8))
    # matrices: the restatement's float32 bits; exact 0 / +-1 at multiples of 90 degrees
    Mr, _, cb = U.detect_setup(BOXES, ROLLS, chip)
    assert np.array_equal(bits(M), bits(Mr))
    for r_ in (0, 1, 2, 3, 4):
        assert set(np.abs(M[r_, :, :2]).reshape(-1).tolist()) == {0.0, 1.0}
    # chips: byte for byte the restated warp of the row's gray frame
    for r_ in range(len(BOXES)):
        ref = U.chips(grays[IDX[r_]], M[r_], chip)
        assert np.array_equal(chips[r_], ref), (chip, r_, int((chips[r_] != ref).sum()))
    assert chips[11].max() == 0                                       # (wholly outside its frame)
    # detect is detect on the chips: plain detect_batch on the chips as host images from the chip boxes, mapped back
    q = rmodel.detect_batch(list(chips), cb)
    assert np.array_equal(bits(res), bits(U.back(M, q)))
    sizes = [(gr.shape[1], gr.shape[0]) for gr in grays]
    expect = U.flags(M, q, chip, guard, [sizes[i][0] for i in IDX], [sizes[i][1] for i in IDX])
    assert np.array_equal(flags, expect)
    assert (flags & U.PARTIAL).any() and not (flags & U.PARTIAL).all()
    # and the oracle on the same chips
    oparams = [orc.HoGParam(1, 5, 6, 4, 0.6)]
    osdo = orc.SupervisedDescentOptimiser([orc.LinearRegressor(orc.Regulariser(orc.Regulariser.MATRIX_NORM, 1.5, False))],
                                          orc.InterEyeDistanceNormalisation(RE, LE))
    osdo.regressors[0].x = rmodel.optimised_model.regressors[0].x
    init = np.stack([synth.align_mean(MEAN, tuple(int(v) for v in bx)) for bx in cb])
    ox = osdo.test(init, None, orc.HogTransform(np.ascontiguousarray(chips), oparams, RE, LE, None, n_threads=8))
    rel = float(np.linalg.norm(q - ox) / np.linalg.norm(ox))
    print(f"chip {chip}: 12 rows on 5 ragged frames, chips / M / flags exact; detect on the chips vs oracle rel-L2 {rel:.2e}")
    assert rel < 1e-4


def test_rows_are_independent_at_4096_rows(rmodel):
    frames, _, boxes = synth.make_tracks(64, 1, seed=78)
    n, chip = 4096, 64
    rng = np.random.default_rng(6)
    idx = np.arange(n, dtype=np.int32) % 64
    bx = boxes[0][idx].copy()
    bx[:, :2] += bx[:, 2:] // 2 - 25 + rng.integers(-20, 21, (n, 2))          # 50-pixel boxes about the faces' centres
    bx[:, 2:] = 50
    rolls = rng.uniform(-180, 180, n).astype(np.float32)
    rolls[::16] = 90.0 * rng.integers(-3, 5, n // 16)
    c = rmodel.optimised_model.ctx
    full = rmodel.detect_batch(frames[0], bx, idx, roll=rolls, chip=chip, guard=8)
    M, flags = rmodel.upright_info()
    assert np.array_equal(bits(M), bits(U.detect_setup(bx, rolls, chip)[0]))
    assert np.array_equal(bits(full), bits(rmodel.detect_batch(frames[0], bx, idx, roll=rolls, chip=chip, guard=8)))
    # permuting the rows permutes results, matrices and flags bit for bit
    perm = rng.permutation(n)
    p = rmodel.detect_batch(frames[0], bx[perm], idx[perm], roll=rolls[perm], chip=chip, guard=8)
    Mp, fp = rmodel.upright_info()
    assert np.array_equal(bits(p), bits(full[perm])) and np.array_equal(bits(Mp), bits(M[perm])) and np.array_equal(fp, flags[perm])
    # every row alone (the images stay): only the split-K partition of the update depends on n, as for the plain tracker
    diffs = np.empty(n)
    for r in range(n):
        c.set_sample_image_index(idx[r:r + 1])
        one = c.detect_batch_upright(MEAN, bx[r:r + 1], rolls[r:r + 1])
        diffs[r] = np.linalg.norm((one[0] - full[r]).astype(np.float64)) / np.linalg.norm(full[r].astype(np.float64))
    print("row alone vs with 4095 others: worst %.2e, median %.2e" % (diffs.max(), np.median(diffs)))
    assert np.median(diffs) < 2e-7
    assert (diffs > 1e-5).sum() <= 8


def test_upright_tracker_steps(rmodel):
    S, n_frames, chip, guard = 8, 10, 288, 36
    frames, _, boxes, rolls = C.make_rolled_tracks(S, n_frames, 2.5, seed=81)
    ids = np.arange(S)
    c = rmodel.optimised_model.ctx
    same = np.arange(S)

    def plain_run():
        tr = rmodel.tracker(S, init="realign", min_size=MIN_SIZE, max_scale_change=MAX_SCALE)
        tr.start(ids, boxes)
        return [tr.step(ids, list(frames[t])) for t in range(3)]

    before = plain_run()
    tr = rmodel.tracker(S, init="upright", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, chip=chip, guard=guard)
    tr.start(ids, boxes)
    lm, st = tr.get(ids)
    assert (st == 1).all()
    # the first step equals detect_batch_upright at roll 0
    res, lost = tr.step(ids, list(frames[0]))
    M, flags = rmodel.upright_info()
    ref = rmodel.detect_batch(list(frames[0]), boxes, roll=0.0, chip=chip, guard=guard)
    assert np.array_equal(bits(res), bits(ref)) and not lost.any()
    assert np.array_equal(bits(M), bits(rmodel.upright_info()[0]))
    tr2 = rmodel.tracker(S, init="upright", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, chip=chip, guard=guard)
    tr2.start(ids, boxes)
    assert np.array_equal(bits(tr2.step(ids, list(frames[0]))[0]), bits(res))
    tr = tr2
    prev = res
    started = np.zeros(S, bool)
    start_roll = np.zeros(S, np.float32)
    for t in range(1, n_frames):
        if t == 4:                                                     # a mixed step: streams 1, 4 and 6 restart from their boxes with a roll
            started[[1, 4, 6]] = True
            start_roll[[1, 4, 6]] = rolls[t]
            tr.start(ids[started], boxes[started], roll=start_roll[started])
            assert list(tr.get(ids)[1]) == [1 if s else 2 for s in started]
        Mr, Wr = U.track_setup(prev, RE, LE, chip)
        init = U.track_init(prev, Wr, MEAN)
        if started.any():
            Ms, _, cb = U.detect_setup(boxes[started], start_roll[started], chip)
            Mr[started] = Ms
            init[started] = np.stack([synth.align_mean(MEAN, tuple(int(v) for v in b)) for b in cb])
        res, lost = tr.step(ids, list(frames[t]))
        M, flags, chips = c.upright_get(chips=True)
        assert np.array_equal(bits(M), bits(Mr)), t
        rchips, q, back = restated(rmodel, frames[t], same, Mr, init, chip)
        assert np.array_equal(chips, rchips), t
        assert np.array_equal(bits(res), bits(back)), t
        assert np.array_equal(lost, T.lost_mask(init, res, 320, 320, MIN_SIZE, MAX_SCALE, RE, LE)), t
        assert np.array_equal(flags, U.flags(Mr, q, chip, guard, 320, 320)), t
        if started.any():                                              # a stream started with roll= gives detect_batch_upright's bits
            d = rmodel.detect_batch(list(frames[t][started]), boxes[started], roll=start_roll[started], chip=chip, guard=guard)
            assert np.array_equal(bits(d), bits(res[started]))
        assert not lost.any()
        started[:] = False
        prev = res
    # the step left its rows, in frame coordinates, as the context's current rows: get, crops, pose
    res, lost = tr.step(ids, list(frames[n_frames - 1]))
    lm, st = tr.get(ids)
    assert np.array_equal(bits(lm), bits(res)) and (st == 2).all()
    assert np.array_equal(bits(c.get_x()), bits(res))
    crops, mats, cflags = rmodel.aligned_crops(48)
    fit, _ = A.fit64(res, np.arange(L), synth_template(48))
    assert np.abs(mats - fit).max() < 1e-3
    for r in range(S):
        assert np.array_equal(crops[r, :, :, 0], A.warp(frames[n_frames - 1][r], mats[r], 48, 48))
    keep = [i for i, lid in enumerate(P.EXAMPLE_IBUG_IDS) if lid in IDS]
    pts = P.EXAMPLE_POINTS[keep]
    proj = ModelProjection(np.concatenate([pts.T, np.ones((1, len(pts)), np.float32)]), 1800.0)
    xs = np.zeros((500, 6), np.float32)
    xs[:, :3] = np.random.default_rng(305).uniform(-30, 30, (500, 3))
    xs[:, 5] = -2000.0
    pose_sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 2.0, True)) for _ in range(2)])
    pose_sdo.train(xs, np.tile(P.EXAMPLE_X0, (500, 1)), proj(xs), proj)
    pose_ids = [P.EXAMPLE_IBUG_IDS[i] for i in keep]
    poses = rmodel.estimate_pose(pose_sdo, proj, pose_ids)
    c.set_x(res)                                                      # (the same rows, set from the host: frame coordinates)
    assert np.isfinite(poses).all() and np.array_equal(bits(rmodel.estimate_pose(pose_sdo, proj, pose_ids)), bits(poses))
    # a realign tracker on the same context gives the bits it gave before the upright tracker existed
    after = plain_run()
    for (a, la), (b, lb) in zip(before, after):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(la, lb)


def synth_template(size):
    from superviseddescent_amd.engine import alignment_template
    return alignment_template(MEAN, list(range(L)), size, size, 0.2)


def test_argument_limits_change_nothing(rmodel):
    frames, _, boxes = synth.make_tracks(4, 1, seed=83)
    imgs = list(frames[0])
    bx = boxes[0]
    c = rmodel.optimised_model.ctx
    ref = rmodel.detect_batch(imgs, bx, roll=10.0, chip=256, guard=32)
    M0, f0, ch0 = c.upright_get(chips=True)
    nan, inf = float("nan"), float("inf")

    def unchanged():
        M, f, ch = c.upright_get(chips=True)
        assert np.array_equal(bits(M), bits(M0)) and np.array_equal(f, f0) and np.array_equal(ch, ch0)
        assert np.array_equal(bits(c.get_x()), bits(ref))

    r4 = np.full(4, 10.0, np.float32)
    cases = [
        lambda: c.upright_configure(31, 0), lambda: c.upright_configure(1025, 0),              # chip outside [32, 1024]
        lambda: c.upright_configure(256, -1), lambda: c.upright_configure(256, 128),            # guard outside [0, chip / 2)
        lambda: c.upright_configure(33, 16),
        lambda: c.detect_batch_upright(MEAN, bx, [10, nan, 0, 0]),                              # a non-finite roll
        lambda: c.detect_batch_upright(MEAN, bx, [10, 0, inf, 0]),
        lambda: c.detect_batch_upright(MEAN, np.array([[5, 5, 0, 40]]), [0.0]),                 # a box without area
        lambda: c.detect_batch_upright(MEAN, np.array([[5, 5, 40, -3]]), [0.0]),
        lambda: c.detect_batch_upright(MEAN, np.zeros((0, 4), np.int32), np.zeros(0, np.float32)),   # n < 1
        lambda: c.detect_batch_upright(MEAN, np.tile(bx, (2, 1)), np.zeros(8, np.float32)),     # more rows than images, no index
    ]
    for f in cases:
        assert code(f) == INVALID
        unchanged()
    c.set_sample_image_index([0, 1, 2])
    assert code(c.detect_batch_upright, MEAN, bx, r4) == INVALID                                 # an index shorter than the rows
    c.set_sample_image_index(None)
    unchanged()
    rows = np.zeros((4, L * rmodel.hog_params[0].patch_dim + 1), np.float32)
    c.set_templates(rows)
    assert code(c.detect_batch_upright, MEAN, bx, r4) == INVALID                                 # templates set
    c.set_templates(None)
    unchanged()
    # and the refused calls left the path usable
    assert np.array_equal(bits(c.detect_batch_upright(MEAN, bx, r4)), bits(ref))
    # upright tracking: mode before configure, rolled start without the mode, then everything a step refuses
    tr = rmodel.tracker(4, init="realign")
    assert code(tr.start, [0], bx[:1], roll=5.0) == INVALID                                      # not in upright mode
    tr = rmodel.tracker(4, init="upright", chip=256, guard=32)
    tr.start([0, 1], bx[:2])
    res, _ = tr.step([0, 1], imgs[:2])
    state = tr.get(np.arange(4))

    def slots_unchanged():
        lm, st = tr.get(np.arange(4))
        assert np.array_equal(bits(lm), bits(state[0])) and np.array_equal(st, state[1])
        assert np.array_equal(bits(c.get_x()), bits(res))

    for f in (lambda: tr.start([2], bx[2:3], roll=nan), lambda: tr.start([2, 2], bx[2:4], roll=0.0), lambda: tr.start([4], bx[:1], roll=0.0),
              lambda: tr.start([2], np.array([[1, 1, 0, 5]]), roll=0.0), lambda: tr.step([0, 2], imgs[:2]), lambda: tr.step([0, 0], imgs[:2]),
              lambda: tr.step([0, 1], imgs[:1]), lambda: tr.step([0, 1], imgs[:2], image_index=[0])):
        assert code(f) == INVALID
        slots_unchanged()
    # contexts of their own: nothing configured, no geometry, no regressors, no images, no eyes
    b4, r4c = np.ascontiguousarray(bx, np.int32), np.ascontiguousarray(r4)

    def raw(ctx):
        return ctx._lib.sdm_detect_batch_upright(ctx._h, MEAN.ctypes.data, b4.ctypes.data, r4c.ctypes.data, 4, None)

    fresh = Context(0)
    try:
        assert raw(fresh) == INVALID                                                             # not configured
        assert fresh._lib.sdm_upright_get(fresh._h, None, None, None) == INVALID                 # no upright call to report
        fresh.upright_configure(64, 8)
        assert raw(fresh) == INVALID                                                             # no geometry
        assert code(fresh.track_configure_upright, True) == INVALID                              # before sdm_track_configure
        fresh.set_model_geometry(L, RE, LE, rmodel.hog_params)
        assert raw(fresh) == INVALID                                                             # no regressors
        fresh.set_regressor(0, rmodel.optimised_model.regressors[0].x)
        assert raw(fresh) == INVALID                                                             # no images
        fresh.upload_images(imgs)
        assert fresh.detect_batch_upright(MEAN, bx, r4).shape == (4, 2 * L)
    finally:
        fresh.close()
    other = Context(0)
    try:
        other.set_model_geometry(L, RE, LE, rmodel.hog_params)
        other.track_configure(4, MEAN, 1, 8.0, 1.5)
        assert code(other.track_configure_upright, True) == INVALID                              # without sdm_upright_configure
        assert code(other.track_start_rolled, [0], bx[:1], [5.0]) == INVALID                     # not in upright mode
        other.upright_configure(64, 8)
        other.track_configure_upright(True)
        other.track_start_rolled([0], bx[:1], [5.0])
        other.upload_images(imgs)
        assert code(other.track_step, [0]) == INVALID                                            # no regressors
        other.set_model_geometry(L, [], [], [HoGParam(1, 5, 6, 4, 0.0)])                         # fixed-size patches need no eyes
        other.track_configure(4, MEAN, 1, 8.0, 1.5)
        assert code(other.track_configure_upright, True) == INVALID                              # upright tracking does
    finally:
        other.close()


@pytest.fixture(scope="module")
def upright_trained(built):
    return trained(*C.make_rolled_faces(300, 0.0, seed=9301), seed=9302)


@pytest.fixture(scope="module")
def roll_trained(built):
    rolls = np.random.default_rng(9303).uniform(-12, 12, 300)
    return trained(*C.make_rolled_faces(300, rolls, seed=9304), seed=9305)


def mean_error(c, gt):
    c.set_targets(gt[:, SEL])
    return float(c.normalised_errors(fetch=False)[1])


def test_detect_accuracy_on_rolled_faces(upright_trained):
    dm = upright_trained
    c = dm.optimised_model.ctx
    images, boxes, gt = C.make_rolled_faces(48, 0.0, seed=9310)
    dm.detect_batch(images, boxes)
    base = mean_error(c, gt)
    worst = 0.0
    for angle in (10, 30, 45, 90, 180):
        images, boxes, gt = C.make_rolled_faces(48, float(angle), seed=9310)          # the same faces, rolled
        dm.detect_batch(images, boxes, roll=float(angle))
        e = mean_error(c, gt)
        _, flags = dm.upright_info()
        print(f"roll {angle:3d}: upright {e:.4f}, plain unrolled {base:.4f}, ratio {e / base:.3f}, near-edge rows {int(((flags & 2) != 0).sum())}")
        worst = max(worst, e / base)
        if angle == 30:
            dm.detect_batch(images, boxes)
            plain = mean_error(c, gt)
            print(f"roll  30: plain detect_batch from the box {plain:.4f} = {plain / e:.1f} x the upright path")
            assert plain >= PLAIN_WORSE * e
    print(f"worst upright / unrolled ratio {worst:.3f}")
    assert worst <= DETECT_RATIO


def test_tracking_accuracy_on_turning_faces(roll_trained):
    dm = roll_trained
    c = dm.optimised_model.ctx
    S, n_frames = 16, 36
    frames, gt, boxes, rolls = C.make_rolled_tracks(S, n_frames, 2.5, seed=9320)
    tr = dm.tracker(S, init="upright", chip=288)
    ids = np.arange(S)
    tr.start(ids, boxes)
    errs = []
    for t in range(n_frames):
        res, lost = tr.step(ids, list(frames[t]), fetch=False)
        assert not lost.any(), (t, lost)
        errs.append(mean_error(c, gt[t]))
    print("error per frame " + " ".join("%.4f" % e for e in errs))
    print(f"36 frames x {S} streams turning 2.5 degrees per frame: frame 0 {errs[0]:.4f}, worst {max(errs):.4f}, ratio {max(errs) / errs[0]:.3f}")
    assert max(errs) <= TRACK_RATIO * errs[0]
    # streams picked up mid-turn from their boxes and the roll are followed from there
    t0 = 20
    tr.start(ids, boxes, roll=rolls[t0])
    for t in range(t0, t0 + 6):
        res, lost = tr.step(ids, list(frames[t]), fetch=False)
        assert not lost.any()
        assert mean_error(c, gt[t]) <= TRACK_RATIO * errs[0]
