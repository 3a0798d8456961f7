"""The upright path's one-wave-per-row kernels (csrc/sdm_upright.hip) at L = 33, 65 and 68: upright_setup_kernel strides a row's
coordinates (and, for a tracked slot, its landmarks: the chip centre and the realign box) over 64 lanes, upright_back_kernel maps a
row back and ORs NEAR_EDGE over its landmarks, and at RCR-22 neither loop takes a second turn.  Chip 64, guard 8.

* detect_batch(..., roll=...) on ragged frames as tests/test_gpu_upright.py runs it: matrices, chips, flags and results bit for bit
  tests/upright_ref.py's;
* NEAR_EDGE from the landmark of the highest index alone, at the guard's threshold: a regressor that is zero except the bias row
  moves that landmark by exactly bias x IED in the chip (as in tests/test_gpu_track_landmark_counts.py); its twin row, where the
  same landmark stays inside, has no flag;
* upright tracker steps whose rows' LAST landmark is the sole x-minimum and y-maximum: the chip centre, the chip and the realign box
  of a tracked slot hang on the last turn of the loops wherever L > 64."""
import numpy as np
import pytest

import landmark_count_cases as K
import track_ref as T
import upright_ref as U
from superviseddescent_amd import Context, HoGParam, HogTransform, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, synth
from upright_cases import BOXES, IDX, ROLLS, ragged_frames

pytestmark = pytest.mark.gpu
f32 = np.float32
CHIP, GUARD = 64, 8
COUNTS = [33, 65, 68]
HP = HoGParam(1, 5, 6, 4, 0.6)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def detect_from(dm, init, chips):
    hog = HogTransform(list(chips), dm.hog_params, dm.landmark_ids, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, None)
    return dm.optimised_model.test(np.asarray(init, np.float32), None, hog)


def last_out(mean, L):
    """the mean's last landmark as its sole x-minimum and y-maximum"""
    mean = mean.copy()
    mean[L - 1] = mean[:L].min() - f32(0.125)
    mean[2 * L - 1] = mean[L:].max() + f32(0.125)
    return mean


@pytest.fixture(scope="module", params=COUNTS, ids=[f"L{L}" for L in COUNTS])
def model(request, built, gpu_ctx):
    """one level, random regressor; its bias row moves the last landmark of every result out to the left and down"""
    L = request.param
    ids, re, le = K.landmark_set(L)
    rng = np.random.default_rng(4321 + L)
    reg = LinearRegressor()
    R = rng.normal(0, 3e-3 * (22.0 / L) ** 0.5, (L * HP.patch_dim + 1, 2 * L)).astype(np.float32)
    R[-1, L - 1] += 1.5
    R[-1, 2 * L - 1] -= 1.5
    reg.x = R
    dm = detection_model(SupervisedDescentOptimiser([reg], ctx=gpu_ctx), last_out(K.mean(L), L), ids, [HP], ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    yield dm, L, re, le
    if getattr(gpu_ctx, "track_upright", False):
        gpu_ctx.track_configure_upright(False)
    gpu_ctx.set_sample_image_index(None)


def test_chips_matrices_flags_and_detect_on_the_chips(model):
    dm, L, re, le = model
    frames, grays, keep = ragged_frames()
    c = dm.optimised_model.ctx
    res = dm.detect_batch(frames, BOXES, IDX, roll=ROLLS, chip=CHIP, guard=GUARD)
    M, flags, chips = c.upright_get(chips=True)
    grays[3] = c.download_image(3)
    Mr, _, cb = U.detect_setup(BOXES, ROLLS, CHIP)
    assert np.array_equal(bits(M), bits(Mr))
    for r_ in range(len(BOXES)):
        assert np.array_equal(chips[r_], U.chips(grays[IDX[r_]], M[r_], CHIP)), r_
    q = dm.detect_batch(list(chips), cb)
    assert q.shape == (len(BOXES), 2 * L)
    assert np.array_equal(bits(res), bits(U.back(M, q)))
    sizes = [(gr.shape[1], gr.shape[0]) for gr in grays]
    expect = U.flags(M, q, CHIP, GUARD, [sizes[i][0] for i in IDX], [sizes[i][1] for i in IDX])
    assert np.array_equal(flags, expect)
    assert (flags & U.PARTIAL).any() and not (flags & U.PARTIAL).all()
    # the last landmark is where the bias row put it: left of and below every other, in the chip
    assert ((q[:, L - 1:L] < q[:, :L - 1]).all(1) & (q[:, 2 * L - 1:] > q[:, L:2 * L - 1]).all(1)).all()


def grid_mean(L):
    """a mean on a dyadic grid inside [-0.25, 0.25]^2, the eyes 0.5 apart at L - 5 ... L - 2, the last landmark in the middle"""
    k = np.arange(L)
    mx = (((k * 5) % 15 - 7) / 32.0).astype(f32)
    my = (((k * 7) % 13 - 6) / 32.0).astype(f32)
    mx[0], my[0], mx[1], my[1] = -0.25, -0.25, 0.25, 0.25
    mx[L - 5:L - 1] = [-0.25, -0.25, 0.25, 0.25]
    my[L - 5:L - 1] = [-0.125, 0.0, -0.125, 0.0]
    mx[L - 1] = my[L - 1] = 0.0
    return np.concatenate([mx, my]).astype(f32)


@pytest.fixture(scope="module")
def own_ctx(built):
    """a context of its own for the hand-made geometry below: the models of this module keep theirs on the shared one"""
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("L", COUNTS)
def test_near_edge_from_the_last_landmark_alone(own_ctx, L):
    """Chip 64, guard 8: a landmark is near the edge below 8 and above 55.  Boxes of 32 put the body at 24 ... 40 in the chip, the
    eyes 16 apart, the last landmark at 32; a bias of 1.5 takes it to exactly 8 (no flag), 1.5625 to 7 (NEAR_EDGE), and in the twin row
    -- a box of 16, the eyes 8 apart -- the same biases leave it at 20 and 19.5.  Then the same towards the far side: 55 and 56."""
    c = own_ctx
    re, le = [L - 5, L - 4], [L - 3, L - 2]
    hp = HoGParam(1, 5, 6, 4, 0.5)
    c.set_detect_path(fused=True, split_store=False)
    c.set_model_geometry(L, re, le, [hp])
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (120, 160), dtype=np.uint8), rng.integers(0, 256, (131, 97), dtype=np.uint8)]
    c.upload_images(frames)
    c.set_templates(None)
    c.upright_configure(CHIP, GUARD)
    boxes = np.array([[60, 40, 32, 32], [68, 48, 16, 16], [30, 50, 32, 32], [38, 58, 16, 16], [64, 44, 32, 32]], np.int32)
    image = np.array([0, 0, 1, 1, 0], np.int32)
    rolls = np.array([0.0, 0.0, 90.0, 90.0, 17.3], f32)
    mean = grid_mean(L)
    F = c.feature_dim(0)
    Mr, _, cb = U.detect_setup(boxes, rolls, CHIP)
    q0 = np.stack([synth.align_mean(mean, tuple(int(v) for v in b)) for b in cb])
    ied = T.ied(q0, re, le)
    assert ied.tolist() == [16.0, 8.0, 16.0, 8.0, 16.0]
    big = ied == 16.0
    W, H = [(160, 97)[i] for i in image], [(120, 131)[i] for i in image]
    seen = set()
    for coord, bias, at, near in ((L - 1, 1.5, 8.0, False), (L - 1, 1.5625, 7.0, True), (2 * L - 1, 1.5, 8.0, False), (2 * L - 1, 1.5625, 7.0, True),
                                  (L - 1, -1.4375, 55.0, False), (L - 1, -1.5, 56.0, True), (2 * L - 1, -1.4375, 55.0, False), (2 * L - 1, -1.5, 56.0, True)):
        R = np.zeros((F, 2 * L), f32)
        R[F - 1, coord] = bias
        c.set_regressor(0, R)
        c.set_sample_image_index(image)
        res = c.detect_batch_upright(mean, boxes, rolls)
        M, flags = c.upright_get()
        q = q0.copy()
        q[:, coord] = q0[:, coord] - f32(bias) * ied.astype(f32)
        assert (q[big, coord] == at).all() and np.array_equal(U.near_edge(q, CHIP, GUARD), big & near)
        assert np.array_equal(bits(M), bits(Mr))
        assert np.array_equal(bits(res), bits(U.back(Mr, q)))           # the premise: the rows are the stated ones
        assert np.array_equal(bits(c.get_x()), bits(res))
        assert np.array_equal(flags, U.flags(Mr, q, CHIP, GUARD, W, H))
        assert np.array_equal(flags, np.where(big & near, U.NEAR_EDGE, 0))      # the last landmark alone; the twins carry no flag
        seen |= set(flags.tolist())
    assert seen == {0, U.NEAR_EDGE}
    c.set_sample_image_index(None)


def test_upright_tracker_steps(model):
    dm, L, re, le = model
    c = dm.optimised_model.ctx
    mean = dm.mean
    S, n_frames = 8, 3
    frames, _, _ = synth.make_tracks(S, n_frames, seed=181)
    rng = np.random.default_rng(182)
    boxes = np.concatenate([rng.integers(96, 128, (S, 2)), rng.integers(34, 44, (S, 1)).repeat(2, 1)], 1).astype(np.int32)
    ids = np.arange(S)
    tr = dm.tracker(S, init="upright", min_size=0.0, max_scale_change=0.0, chip=CHIP, guard=GUARD)
    tr.start(ids, boxes)
    res, lost = tr.step(ids, list(frames[0]))
    M0, _ = dm.upright_info()
    ref = dm.detect_batch(list(frames[0]), boxes, roll=0.0, chip=CHIP, guard=GUARD)
    assert np.array_equal(bits(res), bits(ref)) and not lost.any()
    assert np.array_equal(bits(M0), bits(dm.upright_info()[0]))
    tr = dm.tracker(S, init="upright", min_size=0.0, max_scale_change=0.0, chip=CHIP, guard=GUARD)
    tr.start(ids, boxes)
    assert np.array_equal(bits(tr.step(ids, list(frames[0]))[0]), bits(res))
    prev = res
    for t in range(1, n_frames):
        # the last landmark alone sets the left and the lower side of the enclosing box: the chip centre and the realign box follow it
        assert ((prev[:, L - 1:L] < prev[:, :L - 1]).all(1) & (prev[:, 2 * L - 1:] > prev[:, L:2 * L - 1]).all(1)).all()
        without = np.delete(prev, [L - 1, 2 * L - 1], 1)
        assert all(U.centre_of(a) != U.centre_of(b) for a, b in zip(prev, without))
        Mr, Wr = U.track_setup(prev, re, le, CHIP)
        init = U.track_init(prev, Wr, mean)
        res, lost = tr.step(ids, list(frames[t]))
        M, flags, chips = c.upright_get(chips=True)
        lm, st = tr.get(ids)
        assert np.array_equal(bits(lm), bits(res)) and np.array_equal(bits(c.get_x()), bits(res))      # (the step's rows, in frame coordinates)
        assert np.array_equal(bits(M), bits(Mr)), t
        rchips = np.stack([U.chips(frames[t][i], m, CHIP) for i, m in enumerate(Mr)])
        assert np.array_equal(chips, rchips), t
        q = detect_from(dm, init, rchips)
        assert np.array_equal(bits(res), bits(U.back(Mr, q))), t
        assert np.array_equal(lost, T.lost_mask(init, res, 256, 256, 0.0, 0.0, re, le)), t
        assert np.array_equal(flags, U.flags(Mr, q, CHIP, GUARD, 256, 256)), t
        assert not lost.any(), t
        prev = res
