"""The tracker's motion-compensated initialisation on the device (csrc/sdm_track_motion.hip, include/sdm.h "Tracking,
motion-compensated", detection_model.tracker(motion=...)): the slots' grids and reference chips and every step's search against the
numpy restatement (tests/track_motion_ref.py) on frames cut out of larger noise buffers -- gray, NV12 luma and converted BGR, ragged
sizes, rows sharing an image, an exact translation --; every step against detect from the restated, shifted initialisation, bit for
bit, in the previous, realign and upright modes; the state rules; the filtered step; the accuracy on a fast synthetic video; the
refusals."""
import numpy as np
import pytest

import track_filter_ref as F
import track_motion_ref as R
import track_ref as T
import upright_ref as U
from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, Regulariser, SdmError, SupervisedDescentOptimiser,
                                   detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
f32 = np.float32
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
MIN_SIZE, MAX_SCALE = 8.0, 1.5
INVALID = -1
MOTION = (8, 1.25, 64)
# the "fast" video: make_tracks(..., size=384, max_step=FAST_STEP), the smallest step of {3, 10, 20, 30, 40} pixels per frame and axis
# at which the plain realign tracker's error is at least 3 x its own at 3 pixels or it loses a stream (the quality table)
FAST_STEP = 20
# the motion-on tracker's normalised error over detect's from each frame's true box on that video: measured 9.012 (0.1856 against 0.0206)
# (profiles/track_motion_quality.json); the bound is the measurement plus 0.10
MOTION_ACCURACY_RATIO = 9.11


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
    yield detection_model(sdo, MEAN, IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


@pytest.fixture(scope="module")
def fast_video():
    """8 streams x 7 frames in 384 x 384: streams 0 - 3 move by up to FAST_STEP pixels per frame, streams 4 - 7 by up to 3"""
    fast = synth.make_tracks(4, 7, seed=91, size=384, max_step=float(FAST_STEP))
    slow = synth.make_tracks(4, 7, seed=92, size=384)
    return tuple(np.concatenate([a, b], axis=1) for a, b in zip(fast, slow))


def detect_from(dm, init, images, idx=None):
    return dm.optimised_model.test(np.asarray(init, f32), None,
                                   HogTransform(images, dm.hog_params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))


def aligned(boxes):
    return np.stack([synth.align_mean(MEAN, tuple(int(v) for v in b)) for b in boxes])


def motion_equal(tr, ids, ref):
    m, g, ch = tr.motion(ids)
    rm, rg, rch = ref.get(ids)
    assert np.array_equal(m, rm), (m, rm)
    assert np.array_equal(g, rg), (g, rg)
    assert np.array_equal(ch, rch)


# ---- 1, 2. grids, chips and the search against the restatement ------------------------------------------------------------------------

class Placed:
    """frames cut out of larger noise buffers on the device, whose other bytes keep their noise: gray and NV12 luma in place, BGR
    converted by the context.  at(dx, dy): the frame list with every frame's window moved by (-dx, -dy) -- the content by (dx, dy)."""
    PAD = 72

    def __init__(self, specs, seed):
        import torch
        rng = np.random.default_rng(seed)
        self.specs, self.host, self.dev = specs, [], []
        for kind, w, h in specs:
            rows = h * 3 // 2 if kind == "nv12" else h
            shape = (rows + 2 * self.PAD, w + 2 * self.PAD + 6) + ((3,) if kind == "bgr" else ())
            # smooth structure plus noise, so that a search has something to find
            yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
            base = 128 + 60 * np.sin(xx / 9.0 + rng.uniform(0, 6)) * np.cos(yy / 7.0 + rng.uniform(0, 6))
            base = base[..., None] if kind == "bgr" else base
            a = np.clip(base + rng.normal(0, 12, shape), 0, 255).astype(np.uint8)
            self.host.append(a)
            self.dev.append(torch.from_numpy(a).cuda())

    def at(self, dx=0, dy=0):
        out = []
        for (kind, w, h), t in zip(self.specs, self.dev):
            px = 3 if kind == "bgr" else 1
            stride = t.shape[1] * px
            out.append((t.data_ptr() + (self.PAD - dy) * stride + (self.PAD - dx) * px, w, h, stride, kind))
        return out

    def grays(self, c, dx=0, dy=0):
        """the frames as the image set holds them: a region of the host copy, or the context's conversion"""
        out = []
        for i, ((kind, w, h), a) in enumerate(zip(self.specs, self.host)):
            y0, x0 = self.PAD - dy, self.PAD - dx
            out.append(c.download_image(i) if kind == "bgr" else np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]))
        return out


PLACED = {1: [("gray", 200, 180)],
          3: [("gray", 231, 197), ("nv12", 160, 120), ("bgr", 96, 80)],
          65: [("gray", 384, 384), ("nv12", 322, 200), ("bgr", 96, 80), ("gray", 257, 301), ("gray", 100, 384)]}


@pytest.mark.parametrize("n", [1, 3, 65])
def test_grids_chips_and_search_equal_the_restatement(model, n):
    specs = PLACED[n]
    pl = Placed(specs, 700 + n)
    rng = np.random.default_rng(40 + n)
    idx = (np.arange(n) % len(specs)).astype(np.int32)
    boxes = np.empty((n, 4), np.int32)
    for i in range(n):
        _, w, h = specs[idx[i]]
        s = int(rng.integers(min(w, h) // 3, min(w, h) * 2 // 3))
        boxes[i] = (rng.integers(0, w - s + 1), rng.integers(0, h - s + 1), s, s)
    boxes[0] = (specs[0][1] // 2 - 26, specs[0][2] // 2 - 30, 52, 52)   # row 0: a small face in the middle, its chip wholly inside its frame
    W, H = np.array([specs[j][1] for j in idx]), np.array([specs[j][2] for j in idx])
    c = model.optimised_model.ctx
    tr = model.tracker(n, init="realign", min_size=0.0, max_scale_change=0.0, motion=(8, 1.25, 0))
    ref = R.Motion(n, 8, 1.25, 0)
    ids = np.arange(n)
    motion_equal(tr, ids, ref)                                         # nothing stored, nothing searched
    tr.start(ids, boxes)
    res, lost = tr.step(ids, pl.at(), image_index=idx)
    grays = pl.grays(c)
    assert not ref.search_step(ids, np.zeros(n, bool), grays, idx).any()
    assert same(res, detect_from(model, aligned(boxes), grays, idx))   # (a started row is not shifted)
    ref.store_step(ids, res, lost, grays, idx)
    motion_equal(tr, ids, ref)
    # the next frames: every window moved so that row 0's content moves by exactly (3 k, -2 k) of its grid, then by (-5, 7) pixels
    k0, ox0, oy0 = (int(v) for v in ref.grid[0])
    # (the chip and its translated copy lie inside row 0's frame: nothing of either is the 0 of a tap outside)
    assert lost[0] == 0 and 0 <= ox0 and ox0 + 35 * k0 <= specs[0][1] and 0 <= oy0 - 2 * k0 and oy0 + 32 * k0 <= specs[0][2]
    exact = 0
    for step, (dx, dy) in enumerate(((3 * k0, -2 * k0), (-5, 7))):
        tracked = lost == 0
        prev = res
        res, lost = tr.step(ids[tracked], pl.at(dx, dy), image_index=idx[tracked])
        grays = pl.grays(c, dx, dy)
        shifts = ref.search_step(ids[tracked], np.ones(int(tracked.sum()), bool), grays, idx[tracked])
        if step == 0 and tracked[0]:
            assert tuple(ref.last[0]) == (3 * k0, -2 * k0, 0, ref.last[0, 3], k0, 1) and ref.last[0, 3] > 0
            exact += 1
        init = T.realign(R.shifted(prev[tracked], shifts), MEAN)
        assert same(res, detect_from(model, init, grays, idx[tracked]))
        assert np.array_equal(lost, T.lost_mask(init, res, W[tracked], H[tracked], 0.0))
        ref.store_step(ids[tracked], res, lost, grays, idx[tracked])
        motion_equal(tr, ids, ref)
        ids, idx, W, H = ids[tracked], idx[tracked], W[tracked], H[tracked]
        print(f"n = {n}, step {step}: {ids.size} rows searched, {int((shifts != 0).any(1).sum())} shifted, cell sizes "
              f"{sorted(set(ref.grid[ids, 0].tolist()))}, lost {int((lost != 0).sum())}")
    assert exact == 1
    model.tracker(n)


# ---- 3. every step is detect from the restated, shifted initialisation ----------------------------------------------------------------

def shifted_steps(model, fast_video, mode):
    """6 frames of the fast video, every step checked; the raw rows of every frame"""
    frames, _, boxes = fast_video
    n_frames, S = 6, frames.shape[1]
    ids = np.arange(S)
    plain = model.tracker(S, init=mode, min_size=MIN_SIZE, max_scale_change=MAX_SCALE)
    plain.start(ids, boxes[0])
    plain.step(ids, list(frames[0]))
    plain_1 = plain.step(ids, list(frames[1]))
    tr = model.tracker(S, init=mode, min_size=MIN_SIZE, max_scale_change=MAX_SCALE, motion=MOTION)
    ref = R.Motion(S, *MOTION)
    tr.start(ids, boxes[0])
    prev, lost = tr.step(ids, list(frames[0]))
    ref.store_step(ids, prev, lost, frames[0])
    started = lost != 0
    shifted_rows, rows_log = 0, [prev]
    for t in range(1, n_frames):
        if started.any():
            tr.start(ids[started], boxes[t - 1][started])
            ref.invalidate(ids[started])
            prev = prev.copy()
            prev[started] = aligned(boxes[t - 1][started])
        shifts = ref.search_step(ids, ~started, frames[t])
        moved = R.shifted(prev, shifts)
        init = moved if mode == "previous" else T.realign(moved, MEAN)
        init[started] = prev[started]
        res, lost = tr.step(ids, list(frames[t]))
        assert same(res, detect_from(model, init, list(frames[t]))), t
        assert np.array_equal(lost, T.lost_mask(init, res, 384, 384, MIN_SIZE, MAX_SCALE, RE, LE)), t
        ref.store_step(ids, res, lost, frames[t])
        motion_equal(tr, ids, ref)
        if t == 1:                                                    # rows that were not shifted: a tracker without motion, bit for bit
            still = ~(shifts != 0).any(1)
            assert still.any() and same(res[still], plain_1[0][still]) and np.array_equal(lost[still], plain_1[1][still])
        shifted_rows += int((shifts != 0).any(1).sum())
        started = lost != 0
        prev = res
        rows_log.append(res)
    print(f"{mode}: {n_frames - 1} steps of {S} streams bit-identical to detect from the shifted initialisation; {shifted_rows} rows shifted")
    assert shifted_rows >= n_frames - 1
    model.tracker(S)
    return rows_log


@pytest.mark.parametrize("mode", ["previous", "realign"])
def test_every_step_is_detect_from_its_shifted_initialisation(model, fast_video, mode):
    shifted_steps(model, fast_video, mode)


def test_upright_step_reads_the_shifted_landmarks(model, fast_video):
    frames, _, boxes = fast_video
    S, chip, guard = frames.shape[1], 288, 36
    ids = np.arange(S)
    c = model.optimised_model.ctx
    tr = model.tracker(S, init="upright", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, chip=chip, guard=guard, motion=(8, 1.25, 0))
    ref = R.Motion(S, 8, 1.25, 0)
    tr.start(ids, boxes[0])
    prev, lost = tr.step(ids, list(frames[0]))
    assert not lost.any()
    ref.store_step(ids, prev, lost, frames[0])
    shifted_rows = 0
    for t in (1, 2):
        shifts = ref.search_step(ids, np.ones(S, bool), frames[t])
        moved = R.shifted(prev, shifts)
        Mr, Wr = U.track_setup(moved, RE, LE, chip)
        init = U.track_init(moved, Wr, MEAN)
        res, lost = tr.step(ids, list(frames[t]))
        M, flags, chips = c.upright_get(chips=True)
        assert same(M, Mr), t
        rchips = np.stack([U.chips(frames[t][i], m, chip) for i, m in enumerate(Mr)])
        assert np.array_equal(chips, rchips), t
        assert same(res, U.back(Mr, detect_from(model, init, list(rchips)))), t
        assert np.array_equal(lost, T.lost_mask(init, res, 384, 384, MIN_SIZE, MAX_SCALE, RE, LE)), t
        assert not lost.any()
        ref.store_step(ids, res, lost, frames[t])
        motion_equal(tr, ids, ref)
        shifted_rows += int((shifts != 0).any(1).sum())
        prev = res
    print(f"upright: 2 steps of {S} streams, {shifted_rows} rows shifted")
    assert shifted_rows >= 2
    model.tracker(S)


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------------

def test_state_rules(model, fast_video):
    frames, _, boxes = fast_video
    S = 4
    ids = np.arange(S)
    c = model.optimised_model.ctx
    tr = model.tracker(S, init="realign", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, motion=MOTION)
    ref = R.Motion(S, *MOTION)
    tr.start(ids, boxes[0][:S])
    res, lost = tr.step(ids, list(frames[0][:S]))
    ref.store_step(ids, res, lost, frames[0][:S])
    motion_equal(tr, ids, ref)
    assert ref.valid.all()
    # start invalidates the slots it names, and a STARTED row is not searched
    tr.start([1], boxes[1][1:2])
    ref.invalidate([1])
    motion_equal(tr, ids, ref)
    assert not tr.motion([1])[1].any() and tr.motion([0])[1].any()
    res, lost = tr.step(ids, list(frames[1][:S]))
    ref.search_step(ids, np.array([True, False, True, True]), frames[1][:S])
    ref.store_step(ids, res, lost, frames[1][:S])
    motion_equal(tr, ids, ref)
    m = tr.motion(ids)[0]
    assert m[1, 5] == 0 and not m[1].any() and (m[[0, 2, 3], 5] == 1).all() and not lost.any()
    # a lost row invalidates: stream 2's frame cut to its left 48 columns, the face beyond the right edge
    assert (res[2, :L].min() + res[2, :L].max()) / 2 > 48
    crop = np.ascontiguousarray(frames[2][2][:, :48])
    res2, lost2 = tr.step([2, 3], [crop, frames[2][3]])
    assert lost2[0] & T.OUTSIDE and lost2[1] == 0
    ref.search_step([2, 3], [True, True], [crop, frames[2][3]])
    ref.store_step([2, 3], res2, lost2, [crop, frames[2][3]])
    motion_equal(tr, ids, ref)
    assert not tr.motion([2])[1].any() and tr.motion([3])[1].any()
    # OFF frees the state: the inspection is refused, the steps go on without a search
    c.track_configure_motion(None)
    assert code(c.track_get_motion, [0]) == INVALID
    tr.step([0, 3], list(frames[2][[0, 3]]))
    # on again: every slot invalid, whatever it held
    c.track_configure_motion(*MOTION)
    assert not any(a.any() for a in c.track_get_motion(ids))
    # sdm_track_configure switches the mode off
    plain = model.tracker(S)
    assert code(c.track_get_motion, [0]) == INVALID
    with pytest.raises(ValueError):
        plain.motion([0])


# ---- 5. the filtered step ---------------------------------------------------------------------------------------------------------------

def test_filtered_step_with_motion(model, fast_video):
    frames, _, boxes = fast_video
    n_frames, S = 6, frames.shape[1]
    ids = np.arange(S)
    smooth, dt = (1.0, 5.0, 1.5), f32(1.0 / 15.0)
    raw_rows = shifted_steps(model, fast_video, "realign")
    tr = model.tracker(S, init="realign", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, motion=MOTION, smooth=smooth)
    flt = F.OneEuro(S, L, *smooth)
    started = np.ones(S, bool)
    for t in range(n_frames):
        if started.any():
            tr.start(ids[started], boxes[max(t - 1, 0)][started])
            flt.unprime(ids[started])
        out, lost, raw = tr.step(ids, list(frames[t]), dt=dt)
        assert same(raw, raw_rows[t]), t                                # the raw rows are those of the step without the filter
        assert same(out, flt.step(ids, raw, lost, np.full(S, dt, f32))), t
        assert same(tr.ctx.get_x(), out)
        started = lost != 0
    fr, d, primed = tr.get_filtered(ids)
    rf, rd, rp = flt.get(ids)
    assert same(fr, rf) and same(d, rd) and np.array_equal(primed, rp)
    model.tracker(S)


# ---- 6. accuracy ----------------------------------------------------------------------------------------------------------------------

def run_video(model, video, motion):
    """(mean normalised error of the tracker, of detect from each frame's true box, streams lost)"""
    frames, gt, boxes = video
    S = frames.shape[1]
    c = model.optimised_model.ctx
    tr = model.tracker(S, init="realign", motion=motion)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    e_track, e_detect, n_lost = [], [], 0
    for t in range(frames.shape[0]):
        res, lost = tr.step(ids, list(frames[t]))
        c.set_targets(gt[t][:, SEL])
        e_track.append(c.normalised_errors(fetch=False)[1])
        if lost.any():
            n_lost += int((lost != 0).sum())
            tr.start(ids[lost != 0], boxes[t][lost != 0])
        model.detect_batch(list(frames[t]), boxes[t])
        c.set_targets(gt[t][:, SEL])
        e_detect.append(c.normalised_errors(fetch=False)[1])
    return float(np.mean(e_track)), float(np.mean(e_detect)), n_lost


def test_accuracy_on_the_fast_video(model):
    video = synth.make_tracks(16, 30, size=384, max_step=float(FAST_STEP))
    e_plain, e_detect, lost_plain = run_video(model, video, None)
    e_motion, e_detect2, lost_motion = run_video(model, video, True)
    assert e_detect == e_detect2
    ratio = e_motion / e_detect
    print(f"30 frames x 16 streams, up to {FAST_STEP} px per frame: mean normalised error plain {e_plain:.4f} ({lost_plain} lost), motion on "
          f"{e_motion:.4f} ({lost_motion} lost), detect from the true box {e_detect:.4f}, ratio {ratio:.3f}")
    assert ratio <= MOTION_ACCURACY_RATIO
    assert e_plain >= 2.0 * e_motion or lost_plain > 0
    model.tracker(16)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(model, fast_video):
    frames, _, boxes = fast_video
    S = 4
    ids = np.arange(S)
    c = model.optimised_model.ctx
    fresh = Context(0)                                                 # before sdm_track_configure: a context of its own
    try:
        assert code(fresh.track_configure_motion, 8, 1.25, 32) == INVALID
        assert code(fresh.track_configure_motion, None) == INVALID
        assert code(fresh.track_get_motion, [0]) == INVALID
    finally:
        fresh.close()
    tr = model.tracker(S, init="realign", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, motion=MOTION)
    tr.start(ids, boxes[0][:S])
    tr.step(ids, list(frames[0][:S]))
    tr.step(ids[:3], list(frames[1][:3]))
    state = tr.get(ids) + tr.motion(ids) + (c.get_x(),)

    def unchanged():
        now = tr.get(ids) + tr.motion(ids) + (c.get_x(),)
        for a, b in zip(state, now):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()

    lib, h = c._lib, c._h
    cases = [
        lambda: c.track_configure_motion(0, 1.25, 32), lambda: c.track_configure_motion(17, 1.25, 32),
        lambda: c.track_configure_motion(8, 0.49, 32), lambda: c.track_configure_motion(8, 4.01, 32),
        lambda: c.track_configure_motion(8, float("nan"), 32), lambda: c.track_configure_motion(8, float("inf"), 32),
        lambda: c.track_configure_motion(8, 1.25, -1), lambda: c.track_configure_motion(8, 1.25, 256),
        lambda: c.track_get_motion([S]), lambda: c.track_get_motion([-1]), lambda: c.track_get_motion([0, 0]),
        lambda: c.track_get_motion([]),
        lambda: tr.step([0, S], list(frames[2][:2])), lambda: tr.step([0, 0], list(frames[2][:2])),
    ]
    for f in cases:
        assert code(f) == INVALID
        unchanged()
    assert lib.sdm_track_configure_motion(h, 2, 8, 1.25, 32) == INVALID                      # an unknown mode
    assert lib.sdm_track_configure_motion(h, -1, 8, 1.25, 32) == INVALID
    unchanged()
    # the limits themselves are taken
    for ok in ((1, 0.5, 0), (16, 4.0, 255)):
        c.track_configure_motion(*ok)
    model.tracker(S)
