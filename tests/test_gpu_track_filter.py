"""The tracker's temporal landmark filter on the device (csrc/sdm_track_filter.hip, include/sdm.h "Tracking, filtered",
detection_model.tracker(smooth=...)): tracking itself is untouched by it, bit for bit; the filtered rows, the slots' filter state and
the current rows against the numpy restatement (tests/track_filter_ref.py) fed with the raw rows, at every landmark count at which
track_filter_kernel's lane loop takes another number of turns; lost rows, restarts and plain steps in between; the hand-off to the
crops and the pose; the refusals."""
import numpy as np
import pytest

import landmark_count_cases as K
import pose_f64 as P
import track_filter_ref as F
from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, ModelProjection, Regulariser, SdmError,
                                   SupervisedDescentOptimiser, detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
f32 = np.float32
IDS = ibug.RCR22_IDS
L22 = len(IDS)
MEAN = ibug.select_mean(IDS)
MIN_SIZE, MAX_SCALE = 8.0, 1.5
SMOOTH = (1.0, 5.0, 1.5)
DT = 1.0 / 30.0
INVALID = -1
HP = HoGParam(1, 5, 6, 4, 0.6)
OUTSIDE = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


@pytest.fixture(scope="module")
def model(built):
    """An RCR-22 cascade trained as tests/test_gpu_track.py trains its own."""
    images, boxes, gt = synth.make_faces(600, seed=9200, chunk=32)
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=9201)
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in params])
    sdo.train(x_star, x0, None, HogTransform(images, params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, MEAN, IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


@pytest.fixture(scope="module")
def video():
    return synth.make_tracks(8, 24, seed=77)


def state_of(tr, ids):
    """everything a refused or a plain call must leave alone: slots, filter state, current rows"""
    return tr.get(ids) + tr.get_filtered(ids) + (tr.ctx.get_x(),)


def same_state(a, b):
    return all(np.array_equal(bits(u), bits(v)) if u.dtype == np.float32 else np.array_equal(u, v) for u, v in zip(a, b))


# ---- 1. tracking is untouched --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("init", ["previous", "realign", "upright"])
def test_tracking_is_untouched(model, video, init):
    frames, _, boxes = video
    n_frames, S = frames.shape[:2]
    ids = np.arange(S)
    kw = dict(init=init, min_size=MIN_SIZE, max_scale_change=MAX_SCALE, **(dict(chip=288) if init == "upright" else {}))
    dts = np.random.default_rng(5).uniform(1 / 60, 1 / 15, (n_frames, S)).astype(f32)

    def run(smooth):
        tr = model.tracker(S, smooth=smooth, **kw)
        have = np.zeros(S, bool)
        log, filtered = [], []
        for t in range(n_frames):
            if (~have).any():
                tr.start(ids[~have], boxes[t][~have])
            if smooth is None:
                raw, lost = tr.step(ids, list(frames[t]))
            else:
                out, lost, raw = tr.step(ids, list(frames[t]), dt=dts[t])
                filtered.append(out)
                assert same(tr.ctx.get_x(), out)
            extra = tr.ctx.upright_get() if init == "upright" else ()
            log.append((raw, lost) + tr.get(ids) + tuple(extra))
            have = lost == 0
        return log, filtered

    plain, _ = run(None)
    smoothed, filtered = run(SMOOTH)
    for t, (a, b) in enumerate(zip(plain, smoothed)):
        assert same_state(a, b), t
    moved = int(sum((bits(f) != bits(b[0])).any(1).sum() for f, b in zip(filtered, smoothed)))
    restarts = int(sum((b[1] != 0).sum() for b in smoothed))
    print(f"{init}: {n_frames} frames x {S} streams, raw rows, masks, slots and statuses bit-equal; the filter moved {moved} rows, "
          f"restarts {restarts}")
    assert moved >= (n_frames - 1) * S // 2
    model.tracker(S)                                                   # (a plain tracker again: upright and the filter off)


# ---- 2. parity -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_templates(None)
    if getattr(gpu_ctx, "track_upright", False):
        gpu_ctx.track_configure_upright(False)
    yield gpu_ctx
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_sample_image_index(None)


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("L", [2, 22, 32, 33, 72])
def test_parity_with_the_restatement(ctx, video, L, n):
    """2L = 4, 44, 64 (exactly one pass of the lanes), 66 (the first wrap) and 144 (three passes, the C-ABI's limit); a one-level
    cascade with a random regressor (the rows jitter from frame to frame, which is what the filter is for); no SMALL and no SCALE
    rule, since a set of 2 landmarks has no height."""
    frames, _, boxes = video
    n_frames, S = frames.shape[:2]
    _, re, le = K.landmark_set(L)
    mean = K.mean(L)
    c = ctx
    c.set_model_geometry(L, re, le, [HP])
    Fd = c.feature_dim(0)
    rng = np.random.default_rng(600 + L)
    c.set_regressor(0, rng.normal(0, 3e-3 * (22.0 / L) ** 0.5, (Fd, 2 * L)).astype(f32))
    c.track_configure(S, mean, 1, 0.0, 0.0)
    c.track_configure_filter(*SMOOTH)
    ref = F.OneEuro(S, L, *SMOOTH)
    every = np.arange(S)
    live = every if n == 8 else np.array([5])
    c.track_start(live, boxes[0][live])
    assert not c.track_get_filtered(every)[2].any()
    filtered_rows, lost_rows = 0, 0
    for t in range(n_frames):
        ids = rng.permutation(live)
        if n == 8 and t % 5 == 3:
            ids = ids[:3]                                              # a subset: the other slots' filter state keeps its bits
        dt = rng.uniform(1 / 120, 1 / 10, ids.size).astype(f32)
        c.upload_images(list(frames[t]))
        c.set_sample_image_index(ids)                                  # (stream s reads image s)
        before = c.track_get_filtered(every)
        was_primed = ref.primed[ids] != 0
        out, lost, raw = c.track_step_filtered(ids, dt)
        want = ref.step(ids, raw, lost, dt)
        assert same(out, want), (t, np.argwhere(bits(out) != bits(want))[:4])
        assert same(c.get_x(), out)
        assert same(c.track_get(ids)[0], raw)                          # the slots stay raw
        after = c.track_get_filtered(every)
        for got, exp in zip(after, ref.get(every)):
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), t
        others = np.setdiff1d(every, ids)
        assert all(np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32)) for a, b in zip(after, before))
        filtered_rows += int((was_primed & (lost == 0)).sum())
        lost_rows += int((lost != 0).sum())
        if lost.any():
            again = ids[lost != 0]
            c.track_start(again, boxes[t][again])
            ref.unprime(again)
    print(f"L {L} n {n}: {filtered_rows} filtered rows and the state behind them bit-equal to the restatement, {lost_rows} lost rows")
    assert filtered_rows >= (n_frames - 1) * n // 2 and ref.guards == [0, 0]
    c.track_configure_filter(None)


# ---- 3. lost and restart -------------------------------------------------------------------------------------------------------------

def test_lost_restart_and_plain_steps(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    tr = model.tracker(S, init="previous", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, smooth=SMOOTH)
    ref = F.OneEuro(S, L22, *SMOOTH)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    for t in (0, 1):
        out, lost, raw = tr.step(ids, list(frames[t]), dt=DT)
        assert not lost.any() and same(out, ref.step(ids, raw, lost, DT))
    assert not same(out, raw) and tr.get_filtered(ids)[2].all()
    # stream 0: its frame cropped to the left 64 columns -- the face is now beyond the right edge
    assert (raw[0, :L22].min() + raw[0, :L22].max()) / 2 > 64
    crop = np.ascontiguousarray(frames[2][0][:, :64])
    before = tr.get_filtered(ids)
    out, lost, raw = tr.step([0, 1, 2], [crop, frames[2][1], frames[2][2]], dt=DT)
    assert lost[0] & OUTSIDE and not lost[1:].any()
    assert same(out[0], raw[0])                                        # the lost row passes through ...
    fr, dr, primed = tr.get_filtered(ids)
    assert primed.tolist() == [0] + [1] * (S - 1) and not fr[0].any() and not dr[0].any()      # ... and its state is dropped
    assert same(out, ref.step([0, 1, 2], raw, lost, DT)) and not same(out[1:], raw[1:])       # the neighbours are filtered as ever
    assert all(np.array_equal(a[3:].view(np.uint32), b[3:].view(np.uint32)) for a, b in zip((fr, dr, primed), before))
    for got, exp in zip((fr, dr, primed), ref.get(ids)):
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # a lost stream is refused, filtered or not, and nothing changes
    state = state_of(tr, ids)
    assert code(tr.step, [0], [frames[2][0]], dt=DT) == INVALID and code(tr.step, [3, 0], list(frames[2][[3, 0]]), dt=DT) == INVALID
    assert same_state(state_of(tr, ids), state)
    # restarted, its first filtered row is the raw row; restarting a tracked stream empties its filter too
    tr.start([0, 4], boxes[2][[0, 4]])
    ref.unprime([0, 4])
    assert tr.get_filtered(ids)[2].tolist() == [0, 1, 1, 1, 0, 1, 1, 1]
    out, lost, raw = tr.step([4, 0], list(frames[2][[4, 0]]), dt=DT)
    assert not lost.any() and same(out, raw) and same(out, ref.step([4, 0], raw, lost, DT))
    assert tr.get_filtered(ids)[2].all()
    # plain steps between filtered ones leave the filter's state alone
    kept = tr.get_filtered(ids)
    for t in (3, 4):
        plain, lost = tr.step(ids, list(frames[t]))
        assert not lost.any() and same(tr.ctx.get_x(), plain)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(tr.get_filtered(ids), kept))
    out, lost, raw = tr.step(ids, list(frames[5]), dt=3 * DT)          # (dt: the time since the last FILTERED step)
    assert same(out, ref.step(ids, raw, lost, f32(3 * DT))) and not same(out, raw)


# ---- 4. hand-off ---------------------------------------------------------------------------------------------------------------------

def test_crops_and_pose_follow_the_filtered_rows(model, video):
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
    tr = model.tracker(S, init="realign", smooth=SMOOTH)
    c = tr.ctx
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    for t in range(3):
        out, lost, raw = tr.step(ids, list(frames[t]), dt=DT)
    assert not lost.any() and not same(out, raw)
    _, m_f, flags_f = model.aligned_crops_tensor(32, dtype="uint8")
    pose_f = model.estimate_pose(pose_sdo, proj, pose_ids)
    c.set_x(out)
    _, m_s, flags_s = model.aligned_crops_tensor(32, dtype="uint8")
    assert same(m_f, m_s) and np.array_equal(flags_f, flags_s)
    assert same(pose_f, model.estimate_pose(pose_sdo, proj, pose_ids))
    c.set_x(raw)                                                       # and they are not the raw rows'
    assert not same(model.aligned_crops_tensor(32, dtype="uint8")[1], m_f)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(model, video):
    frames, _, boxes = video
    S = frames.shape[1]
    fresh = Context(0)
    try:
        fresh.set_model_geometry(L22, *ibug.eye_indices(IDS), model.hog_params)
        assert code(fresh.track_configure_filter, 1.0, 5.0) == INVALID                      # before sdm_track_configure
        fresh.track_configure(4, MEAN, 1, 8.0, 1.5)
        assert code(fresh.track_step_filtered, [0], DT) == INVALID                          # no filter configured
        assert code(fresh.track_get_filtered, [0]) == INVALID
        fresh.track_configure_filter(1.0, 5.0)
        assert fresh.track_get_filtered([0, 3])[2].tolist() == [0, 0]
        fresh.track_configure_filter(None)
        assert code(fresh.track_get_filtered, [0]) == INVALID                               # OFF
        fresh.track_configure_filter(1.0, 5.0)
        fresh.track_configure(4, MEAN, 1, 8.0, 1.5)
        assert code(fresh.track_get_filtered, [0]) == INVALID                               # a later sdm_track_configure switches it off
    finally:
        fresh.close()
    tr = model.tracker(S, smooth=SMOOTH)
    c = tr.ctx
    ids = np.arange(S)
    tr.start(ids[:6], boxes[0][:6])
    for t in (0, 1):
        tr.step(ids[:6], list(frames[t][:6]), dt=DT)
    tr.start([6], boxes[1][6:7])
    state = state_of(tr, ids)
    assert state[4][:6].all() and not state[4][6:].any()
    i2 = np.array([0, 1], np.int32)
    lib, h = c._lib, c._h
    nan, inf = float("nan"), float("inf")
    cases = [
        lambda: tr.step([0, S], list(frames[2][:2]), dt=DT),            # what sdm_track_step refuses: an id out of range,
        lambda: tr.step([0, 1, 0], list(frames[2][:3]), dt=DT),         # a duplicate,
        lambda: tr.step([0, 7], list(frames[2][:2]), dt=DT),            # a free slot,
        lambda: tr.step(ids[:7], list(frames[2][:6]), dt=DT),           # fewer images than rows
        lambda: c.track_step_filtered([], DT),
        lambda: c.track_configure_filter(0.0, 5.0), lambda: c.track_configure_filter(-1.0, 5.0),
        lambda: c.track_configure_filter(nan, 5.0), lambda: c.track_configure_filter(inf, 5.0),
        lambda: c.track_configure_filter(1.0, -0.5), lambda: c.track_configure_filter(1.0, nan),
        lambda: c.track_configure_filter(1.0, inf),
        lambda: c.track_configure_filter(1.0, 5.0, 0.0), lambda: c.track_configure_filter(1.0, 5.0, -2.0),
        lambda: c.track_configure_filter(1.0, 5.0, nan), lambda: c.track_configure_filter(1.0, 5.0, inf),
    ] + [(lambda v=v: tr.step([0, 1], list(frames[2][:2]), dt=[DT, v])) for v in (0.99e-4, 1.01e4, 0.0, -DT, nan, inf)]
    for k, f in enumerate(cases):
        assert code(f) == INVALID, k
        assert same_state(state_of(tr, ids), state), k
    c.upload_images(list(frames[2][:2]))
    c.set_sample_image_index(None)
    assert lib.sdm_track_configure_filter(h, 7, 1.0, 5.0, 1.0) == INVALID                   # an unknown mode
    assert lib.sdm_track_step_filtered(h, i2.ctypes.data, 2, None, None, None, None) == INVALID      # dt_seconds NULL
    assert same_state(state_of(tr, ids), state)
    # the same step with its times at the bounds is taken; every output of the step and of the get may be NULL
    assert lib.sdm_track_step_filtered(h, i2.ctypes.data, 2, np.array([1e-4, 1e4], f32).ctypes.data, None, None, None) == 0
    assert lib.sdm_track_get_filtered(h, i2.ctypes.data, 2, None, None, None) == 0
    c.N = 2                                                            # (what Context.track_step_filtered notes behind the call)
    assert same(c.get_x(), tr.get_filtered([0, 1])[0]) and not same(c.get_x(), tr.get([0, 1])[0])
