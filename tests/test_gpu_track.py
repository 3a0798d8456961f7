"""Multi-stream tracking on the device (csrc/sdm_track.hip, include/sdm.h sdm_track_*, detection_model.tracker): every step against
the detect batch it must equal bit for bit, the realign and lost rules against their host restatement (tests/track_ref.py), stream
independence, argument limits, accuracy on synthetic video, the track -> pose hand-off and the C++ layer's rcr::tracker."""
import os

import numpy as np
import pytest

import cpp_build as B
import pose_f64 as P
import track_ref as T
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
# a tracked face's normalised error may be at most this multiple of detect's from the true box: measured 1.050 on this video
# (DESIGN.md 4.8), so the bound is set from the measurement instead of the issue's guess of 1.5
ACCURACY_RATIO = 1.15


@pytest.fixture(scope="module")
def model(built):
    """An RCR-22 cascade trained as in test_gpu_full_size_properties.py (600 faces x 5 rows, the four shipped levels)."""
    images, boxes, gt = synth.make_faces(600, seed=9200, chunk=32)
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=9201)
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in params])
    sdo.train(x_star, x0, None, HogTransform(images, params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, MEAN, IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


@pytest.fixture(scope="module")
def video():
    return synth.make_tracks(8, 24, seed=77)


def hog(dm, images, idx=None):
    return HogTransform(images, dm.hog_params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx)


def detect_from(dm, init, images, idx=None):
    """set_x(init) + detect_batch on the same rows: what a step must equal"""
    return dm.optimised_model.test(np.asarray(init, np.float32), None, hog(dm, images, idx))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def aligned(boxes):
    return np.stack([synth.align_mean(MEAN, tuple(int(v) for v in b)) for b in boxes])


def test_first_step_is_detect_batch(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    tr = model.tracker(S)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    lm, st = tr.get(ids)
    assert (st == 1).all() and np.array_equal(bits(lm), bits(aligned(boxes[0])))     # STARTED, its landmarks the stored align_mean
    res, lost = tr.step(ids, list(frames[0]))
    ref = model.detect_batch(list(frames[0]), boxes[0])
    assert np.array_equal(bits(res), bits(ref))
    # two faces on one image: the rows read the image of their index
    tr.start([3, 5], boxes[0][[1, 6]])
    res2, _ = tr.step([3, 5], [frames[0][1], frames[0][6]], image_index=[0, 1])
    assert np.array_equal(bits(res2), bits(ref[[1, 6]]))


@pytest.mark.parametrize("mode", ["previous", "realign"])
def test_every_step_is_detect_from_its_initialisation(model, video, mode):
    from oracle import sdm_oracle as orc
    frames, _, boxes = video
    n_frames, S = frames.shape[:2]
    tr = model.tracker(S, init=mode, min_size=MIN_SIZE, max_scale_change=MAX_SCALE)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    prev = tr.step(ids, list(frames[0]))[0]
    oparams = [orc.HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    osdo = orc.SupervisedDescentOptimiser([orc.LinearRegressor(orc.Regulariser(orc.Regulariser.MATRIX_NORM, 1.5, False)) for _ in oparams],
                                          orc.InterEyeDistanceNormalisation(RE, LE))
    for lvl, r in enumerate(model.optimised_model.regressors):
        osdo.regressors[lvl].x = r.x
    worst, restarts = 0.0, 0
    started = np.zeros(S, bool)
    for t in range(1, n_frames):
        init = prev.copy() if mode == "previous" else T.realign(prev, MEAN)
        init[started] = prev[started]                                 # (a restarted stream begins from its box again)
        res, lost = tr.step(ids, list(frames[t]))
        assert np.array_equal(bits(res), bits(detect_from(model, init, list(frames[t]))))
        assert np.array_equal(lost, T.lost_mask(init, res, 256, 256, MIN_SIZE, MAX_SCALE, RE, LE))
        ohog = orc.HogTransform(np.ascontiguousarray(frames[t]), oparams, RE, LE, np.arange(S, dtype=np.int32), n_threads=16)
        ox = osdo.test(init, None, ohog)
        rel = float(np.linalg.norm(res - ox) / np.linalg.norm(ox))
        worst = max(worst, rel)
        assert rel < 1e-4, (t, rel)
        started = lost != 0
        prev = res.copy()
        if started.any():                                             # (rcr-track: the lost ones go back to the detector)
            tr.start(ids[started], boxes[t][started])
            restarts += int(started.sum())
            prev[started] = aligned(boxes[t][started])
    print(f"{mode}: {n_frames - 1} steps of {S} streams bit-identical to detect_batch; worst rel-L2 vs oracle {worst:.2e}, restarts {restarts}")


def test_streams_are_independent(model):
    frames, _, boxes = synth.make_tracks(64, 2, seed=78)
    n = 4096
    idx = np.arange(n, dtype=np.int32) % 64
    shift = ((np.arange(n) // 64) % 7 - 3)[:, None] * np.array([[1, 1, 0, 0]])
    sboxes = [boxes[t][idx] + shift for t in range(2)]
    tr = model.tracker(n, init="realign", min_size=0.0, max_scale_change=0.0)
    ids = np.arange(n)

    def warm():
        """every stream started and stepped once on frame 0 (deterministic: the same bits every time)"""
        tr.start(ids, sboxes[0])
        return tr.step(ids, frames[0], image_index=idx)[0]

    x0 = warm()
    assert np.array_equal(bits(x0), bits(warm()))
    full, _ = tr.step(ids, frames[1], image_index=idx)
    # permuting the ids within a step permutes the results bit for bit (first step and a later step)
    perm = np.random.default_rng(5).permutation(n)
    tr.start(ids, sboxes[0])
    p0, _ = tr.step(ids[perm], frames[0], image_index=idx[perm])
    assert np.array_equal(bits(p0), bits(x0[perm]))
    p1, _ = tr.step(ids[perm], frames[1], image_index=idx[perm])
    assert np.array_equal(bits(p1), bits(full[perm]))
    # alone, or with 7 / 255 others: only the split-K partition of the update depends on n
    diffs = []
    for k in (1, 8, 256):
        warm()
        before, _ = tr.get(ids)
        sub, _ = tr.step(ids[:k], frames[1], image_index=idx[:k])
        after, st = tr.get(ids)
        assert np.array_equal(bits(after[k:]), bits(before[k:]))       # the other slots' bits are untouched
        assert np.array_equal(bits(after[:k]), bits(sub)) and (st[:k] == 2).all()
        diffs.append(np.linalg.norm((sub - full[:k]).astype(np.float64), axis=1) / np.linalg.norm(full[:k].astype(np.float64), axis=1))
    per_face = np.concatenate(diffs)
    print("stream alone / with 7 / with 255 others vs with 4095: worst %.2e, median %.2e" % (per_face.max(), np.median(per_face)))
    assert np.median(per_face) < 2e-7
    assert (per_face > 1e-5).sum() <= 8


def test_lost_rule_refusal_and_restart(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    tr = model.tracker(S, init="previous", min_size=MIN_SIZE, max_scale_change=MAX_SCALE)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    prev, lost = tr.step(ids, list(frames[0]))
    assert not lost.any()
    # stream 0: its frame cropped to the left 64 columns -- the face is now beyond the right edge
    crop = np.ascontiguousarray(frames[1][0][:, :64])
    # stream 1: a blank frame
    blank = np.full_like(frames[1][1], 128)
    cx = (prev[0, :L].min() + prev[0, :L].max()) / 2
    assert cx > 64
    res, lost = tr.step([0, 1], [crop, blank])
    expect = T.lost_mask(prev[:2], res, np.array([64, 256]), 256, MIN_SIZE, MAX_SCALE, RE, LE)
    assert np.array_equal(lost, expect)
    assert lost[0] & T.OUTSIDE
    # on a blank frame the features carry no face: every level moves the shape by its bias row alone, so the stream drifts away
    # step by step until a rule catches it (one blank frame moves it by a few pixels only)
    n_blank, last = 1, res[1:2]
    while not lost[1] and n_blank < 100:
        init = last
        last, lost1 = tr.step([1], [blank])
        assert np.array_equal(lost1, T.lost_mask(init, last, 256, 256, MIN_SIZE, MAX_SCALE, RE, LE))
        lost = np.array([lost[0], lost1[0]])
        n_blank += 1
    print("lost masks: face out of the frame %d; blank frames %d after %d steps" % (lost[0], lost[1], n_blank))
    assert lost[1] != 0
    res = np.concatenate([res[:1], last])
    # a lost stream is refused and nothing changes
    before, st = tr.get(ids)
    assert (st[:2] == 3).all() and (st[2:] == 2).all()
    assert np.array_equal(bits(before[:2]), bits(res))                  # (it keeps its last landmarks)
    assert code(tr.step, [2, 0], list(frames[1][[2, 0]])) == INVALID
    assert code(tr.step, [1], [frames[1][1]]) == INVALID
    after, st2 = tr.get(ids)
    assert np.array_equal(bits(after), bits(before)) and np.array_equal(st, st2)
    # restarted from a new box it is tracked again
    tr.start([0, 1], boxes[1][:2])
    res, lost = tr.step([0, 1], list(frames[1][:2]))
    assert not lost.any()
    assert np.array_equal(bits(res), bits(model.detect_batch(list(frames[1][:2]), boxes[1][:2])))


def test_argument_limits_change_nothing(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    c = model.optimised_model.ctx
    # geometry / regressors / configuration missing, the geometry changed after configure: a context of its own
    fresh = Context(0)
    try:
        assert code(fresh.track_step, [0]) == INVALID                                       # no geometry, not configured
        fresh.set_model_geometry(L, RE, LE, model.hog_params)
        assert code(fresh.track_step, [0]) == INVALID                                       # not configured
        assert code(fresh.track_configure, 0, MEAN, 1, 8.0, 1.5) == INVALID                  # capacity < 1
        flat = MEAN.copy()
        flat[L:] = 0.25
        assert code(fresh.track_configure, 4, flat, 1, 8.0, 1.5) == INVALID                 # a mean without height
        fresh.track_configure(4, MEAN, 1, 8.0, 1.5)
        fresh.track_start([0], boxes[0][:1])
        fresh.upload_images(list(frames[0][:1]))
        assert code(fresh.track_step, [0]) == INVALID                                       # no regressors
        ids68 = ibug.IBUG68_IDS
        r68, l68 = ibug.eye_indices(ids68)
        fresh.set_model_geometry(68, r68, l68, model.hog_params)
        assert code(fresh.track_step, [0]) == INVALID                                       # L changed since configure
        assert code(fresh.track_get, [0]) == INVALID
    finally:
        fresh.close()
    # on the model's context, with live streams: every refused call leaves the slots and the current rows as they were
    tr = model.tracker(S)
    ids = np.arange(S)
    tr.start(ids[:6], boxes[0][:6])
    tr.step(ids[:6], list(frames[0][:6]))
    tr.start([6], boxes[0][6:7])
    ref_rows = c.get_x()
    state = tr.get(ids)

    def unchanged():
        lm, st = tr.get(ids)
        assert np.array_equal(bits(lm), bits(state[0])) and np.array_equal(st, state[1])
        assert np.array_equal(bits(c.get_x()), bits(ref_rows))

    cases = [
        lambda: tr.step([0, S], list(frames[1][:2])),                    # id out of range
        lambda: tr.step([-1], list(frames[1][:1])),
        lambda: tr.step([0, 1, 0], list(frames[1][:3])),                 # duplicate
        lambda: tr.step([0, 7], list(frames[1][:2])),                    # a free slot
        lambda: tr.step(ids[:7], list(frames[1][:6])),                   # no map and fewer images than rows
        lambda: tr.step(ids[:4], list(frames[1][:4]), image_index=[0, 1, 2]),   # a map shorter than the rows
        lambda: tr.start([0, 0], boxes[1][:2]),
        lambda: tr.start([S], boxes[1][:1]),
        lambda: tr.stop([1, 1]),
        lambda: tr.get([S + 3]),
        lambda: c.track_step([]),
    ]
    for f in cases:
        assert code(f) == INVALID
        unchanged()
    # and a plain detect batch on the same context still gives its own earlier result
    a = model.detect_batch(list(frames[2]), boxes[2])
    assert np.array_equal(bits(a), bits(model.detect_batch(list(frames[2]), boxes[2])))
    tr.stop([6])
    assert tr.get([6])[1][0] == 0
    assert code(tr.step, [6], [frames[1][6]]) == INVALID


def test_tracking_accuracy_on_synthetic_video(model):
    frames, gt, boxes = synth.make_tracks(16, 30, seed=79)
    S = frames.shape[1]
    c = model.optimised_model.ctx
    tr = model.tracker(S, init="realign")
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    e_track, e_detect, restarts = [], [], 0
    for t in range(frames.shape[0]):
        res, lost = tr.step(ids, list(frames[t]))
        c.set_targets(gt[t][:, SEL])
        e_track.append(c.normalised_errors(fetch=False)[1])
        if lost.any():
            restarts += int((lost != 0).sum())
            tr.start(ids[lost != 0], boxes[t][lost != 0])
        model.detect_batch(list(frames[t]), boxes[t])
        c.set_targets(gt[t][:, SEL])
        e_detect.append(c.normalised_errors(fetch=False)[1])
    ratio = float(np.mean(e_track) / np.mean(e_detect))
    print(f"30 frames x {S} streams, realign: mean normalised error tracked {np.mean(e_track):.4f}, detect from the true box "
          f"{np.mean(e_detect):.4f}, ratio {ratio:.3f}, restarts {restarts}")
    assert ratio <= ACCURACY_RATIO


def test_track_to_pose(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    keep = [i for i, lid in enumerate(P.EXAMPLE_IBUG_IDS) if lid in IDS]
    pose_ids = [P.EXAMPLE_IBUG_IDS[i] for i in keep]
    pts = P.EXAMPLE_POINTS[keep]
    proj = ModelProjection(np.concatenate([pts.T, np.ones((1, len(pts)), np.float32)]), 1800.0)
    xs = np.zeros((2000, 6), np.float32)
    xs[:, :3] = np.random.default_rng(305).uniform(-30, 30, (2000, 3))
    xs[:, 5] = -2000.0
    pose_sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 2.0, True)) for _ in range(3)])
    pose_sdo.train(xs, np.tile(P.EXAMPLE_X0, (2000, 1)), proj(xs), proj)
    tr = model.tracker(S, init="realign")
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    prev, _ = tr.step(ids, list(frames[0]))
    res, _ = tr.step(ids, list(frames[1]))
    poses = model.estimate_pose(pose_sdo, proj, pose_ids)
    assert poses.shape == (S, 6) and np.isfinite(poses).all()
    again = detect_from(model, T.realign(prev, MEAN), list(frames[1]))
    assert np.array_equal(bits(again), bits(res))
    assert np.array_equal(bits(model.estimate_pose(pose_sdo, proj, pose_ids)), bits(poses))


def test_cpp_tracker_matches_python(model, tmp_path):
    frames, _, boxes = synth.make_tracks(6, 16, seed=80)
    frames = frames.copy()
    frames[6, 2] = 128                                                  # a blank frame for stream 2: it may be lost and restarted
    n_frames, S, H, W = frames.shape
    d = str(tmp_path)
    B.write_model(d, L, model.hog_params, MEAN, IDS, regressors=[r.x for r in model.optimised_model.regressors])
    frames.tofile(os.path.join(d, "frames.u8"))
    boxes.astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{S} {n_frames} {H} {W} {S}\n")
    B.run(B.gpu_driver("track_gpu", tmp_path), [d], 300)
    # the same loop through the Python Tracker
    tr = model.tracker(S)
    ids = np.arange(S)
    have = np.zeros(S, bool)
    lms, masks = [], []
    for t in range(n_frames):
        if (~have).any():
            tr.start(ids[~have], boxes[t][~have])
        res, lost = tr.step(ids, list(frames[t]))
        have = lost == 0
        lms.append(res)
        masks.append(lost)
    cpp_l = np.fromfile(os.path.join(d, "cpp_landmarks.f32"), np.float32).reshape(n_frames, S, 2 * L)
    cpp_m = np.fromfile(os.path.join(d, "cpp_lost.i32"), np.int32).reshape(n_frames, S)
    assert np.array_equal(bits(cpp_l), bits(np.stack(lms)))
    assert np.array_equal(cpp_m, np.stack(masks))
