"""The tracker's one-wave-per-row kernels (csrc/sdm_track.hip) at rows of more than 64 coordinates, and of more than 64 landmarks:
track_gather_kernel, track_commit_kernel and row_bounds stride a row over the 64 lanes of a wave, and at RCR-22 (2L = 44) none of
their loops takes a second turn.

* L = 32, 33, 64, 65, 68, 72 in both init modes: every step is detect_batch from its restated initialisation bit for bit, the lost
  mask is tests/track_ref.py's, the slots return the rows.  The LAST landmark of every result row is its sole x-minimum and
  y-maximum (the regressor's bias row moves it there) and so is the mean's, so the enclosing box -- the realign, the centre and
  size rules -- hangs on the last turn of row_bounds wherever L > 64.
* every SDM_TRACK_LOST_* bit on its own, set and clear, at its threshold: a one-level cascade whose regressor is zero except the
  bias row moves a row by exactly bias x IED; with a mean on a dyadic grid, boxes of 128 x 128 and eyes 64 pixels apart the result
  row is exact, and the test states it in numpy float32 and first asserts that the device returned those bits.  The deciding
  landmark is the last one (SMALL, OUTSIDE), the eyes sit at L - 5 ... L - 2 (SCALE), the overflowing coordinate lies in the first,
  second and third turn of the non-finite scan (NONFINITE)."""
import numpy as np
import pytest

import landmark_count_cases as K
import track_ref as T
from superviseddescent_amd import HoGParam, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
HP = HoGParam(1, 5, 6, 4, 0.6)
MIN_SIZE, MAX_SCALE = 8.0, 1.5
PREVIOUS, REALIGN = 0, 1
TRACKED, LOST = 2, 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_templates(None)
    if getattr(gpu_ctx, "track_upright", False):
        gpu_ctx.track_configure_upright(False)
    yield gpu_ctx
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_sample_image_index(None)


@pytest.fixture(scope="module")
def video():
    return synth.make_tracks(8, 3, seed=177)


def aligned(mean, boxes):
    return np.stack([synth.align_mean(mean, tuple(int(v) for v in b)) for b in boxes])


def detect_from(c, init):
    c.set_x(init)
    return c.detect_batch()


@pytest.mark.parametrize("mode", [PREVIOUS, REALIGN], ids=["previous", "realign"])
@pytest.mark.parametrize("L", [32, 33, 64, 65, 68, 72])
def test_every_step_is_detect_from_its_initialisation(ctx, video, L, mode):
    frames, _, boxes = video
    n_frames, S = frames.shape[:2]
    _, re, le = K.landmark_set(L)
    mean = K.mean(L)
    # the mean's last landmark is its sole x-minimum and y-maximum ...
    mean[L - 1] = mean[:L].min() - f32(0.125)
    mean[2 * L - 1] = mean[L:].max() + f32(0.125)
    c = ctx
    c.set_model_geometry(L, re, le, [HP])
    F = c.feature_dim(0)
    R = np.random.default_rng(4321 + L).normal(0, 3e-3 * (22.0 / L) ** 0.5, (F, 2 * L)).astype(np.float32)
    # ... and the bias row moves every result's there: x by -1.5 IED, y by +1.5 IED (IED ~ 60 pixels, a face ~ 140)
    R[F - 1, L - 1] += 1.5
    R[F - 1, 2 * L - 1] -= 1.5
    c.set_regressor(0, R)
    c.track_configure(S, mean, mode, MIN_SIZE, MAX_SCALE)
    ids = np.arange(S)
    c.track_start(ids, boxes[0])
    lm, st = c.track_get(ids)
    assert (st == 1).all() and np.array_equal(bits(lm), bits(aligned(mean, boxes[0])))
    started = np.ones(S, bool)
    prev = aligned(mean, boxes[0])
    sole, masks_seen = 0, 0
    for t in range(n_frames):
        init = prev.copy() if mode == PREVIOUS else T.realign(prev, mean)
        init[started] = prev[started]
        c.upload_images(list(frames[t]))
        c.set_sample_image_index(None)
        res, lost = c.track_step(ids)
        assert np.array_equal(bits(c.get_x()), bits(res))
        lm, st = c.track_get(ids)
        assert np.array_equal(bits(lm), bits(res)), t
        assert np.array_equal(st, np.where(lost != 0, LOST, TRACKED)), t
        assert np.array_equal(bits(res), bits(detect_from(c, init))), t
        assert np.array_equal(lost, T.lost_mask(init, res, 256, 256, MIN_SIZE, MAX_SCALE, re, le)), t
        # the premise: the last landmark alone holds the box's left and lower edge
        sole += int(((res[:, L - 1:L] < res[:, :L - 1]).all(1) & (res[:, 2 * L - 1:] > res[:, L:2 * L - 1]).all(1)).sum())
        masks_seen |= int(np.bitwise_or.reduce(lost))
        started = lost != 0
        prev = res.copy()
        if started.any():
            c.track_start(ids[started], boxes[t][started])
            prev[started] = aligned(mean, boxes[t][started])
    assert sole == n_frames * S
    print(f"L {L} mode {mode}: {n_frames} steps of {S} streams bit-identical to detect_batch; lost bits seen {masks_seen}")


# ---- the lost rule, bit by bit ---------------------------------------------------------------------------------------------------------

# ragged frames: (width, height) of images 0, 1, 2
SIZES = [(160, 120), (96, 200), (131, 77)]
HP_LOST = HoGParam(1, 5, 6, 4, 0.25)            # (patches of a quarter IED: a half-width of 64 pixels at the 1024-pixel boxes)


def grid_mean(L, last=(0.0, 0.0)):
    """A mean on a dyadic grid inside [-0.375, 0.375]^2: landmarks 0 and 1 hold the corners, the eyes sit at L - 5 ... L - 2, 0.5
    apart on one line, the last landmark at ``last``.  In a box (bx, by, 128, 128) align_mean is exact: the body spans
    [b + 16, b + 112], the inter-eye distance is 64, the last landmark lies at b + 64 + 128 last."""
    mx, my = np.empty(L, f32), np.empty(L, f32)
    k = np.arange(L)
    mx[:] = ((k * 5) % 23 - 11) / 32.0
    my[:] = ((k * 7) % 19 - 9) / 32.0
    mx[0], my[0], mx[1], my[1] = -0.375, -0.375, 0.375, 0.375
    mx[L - 5:L - 1] = [-0.25 - 1 / 64, -0.25 + 1 / 64, 0.25 - 1 / 64, 0.25 + 1 / 64]
    my[L - 5:L - 1] = -0.125
    mx[L - 1], my[L - 1] = last
    return np.concatenate([mx, my]).astype(f32)


def eyes(L):
    return [L - 5, L - 4], [L - 3, L - 2]


class Stage:
    """one landmark count on one detect path: steps of freshly started streams under a bias-row regressor"""

    def __init__(self, c, L, path):
        self.c, self.L, self.re_le = c, L, eyes(L)
        rng = np.random.default_rng(7)
        self.images = [rng.integers(0, 256, (h, w), dtype=np.uint8) for w, h in SIZES]
        c.set_detect_path(fused={"fused": True if 2 * L <= 64 else "wide", "unfused": False}[path])
        c.set_model_geometry(L, *self.re_le, [HP_LOST])
        c.upload_images(self.images)
        self.F = c.feature_dim(0)

    def step(self, mean, bias, boxes, image, min_size=MIN_SIZE, max_scale=MAX_SCALE):
        """Rows started from ``boxes`` on the images ``image``, one step.  Returns (init rows, the result rows as stated here, lost
        masks) after asserting the premise -- the device's rows are the stated ones, bit for bit -- the slots and the mask rule."""
        c, L = self.c, self.L
        re, le = self.re_le
        boxes, image = np.asarray(boxes, np.int32).reshape(-1, 4), np.asarray(image, np.int32)
        n = len(boxes)
        R = np.zeros((self.F, 2 * L), f32)
        R[self.F - 1] = bias
        c.set_regressor(0, R)
        c.track_configure(n, mean, PREVIOUS, min_size, max_scale)
        ids = np.arange(n)
        c.track_start(ids, boxes)
        c.set_sample_image_index(image)
        res, lost = c.track_step(ids)
        x0 = aligned(mean, boxes)
        ied = T.ied(x0, re, le)
        assert set(ied.tolist()) <= {64.0, 512.0}
        with np.errstate(over="ignore", invalid="ignore"):
            x1 = (x0 - np.asarray(bias, f32)[None, :] * ied.astype(f32)[:, None]).astype(f32)
        assert np.array_equal(bits(res), bits(x1)), np.argwhere(bits(res) != bits(x1))[:4]
        lm, st = c.track_get(ids)
        assert np.array_equal(bits(lm), bits(x1)) and np.array_equal(st, np.where(lost != 0, LOST, TRACKED))
        W, H = np.array([SIZES[i][0] for i in image]), np.array([SIZES[i][1] for i in image])
        assert np.array_equal(lost, T.lost_mask(x0, x1, W, H, min_size, max_scale, re, le))
        self.last = (x0, x1, W, H, min_size, max_scale)
        return x0, x1, lost

    def mask64(self):
        x0, x1, W, H, min_size, max_scale = self.last
        return T.lost_mask64(x0, x1, W, H, min_size, max_scale, *self.re_le)


STAGES = [(33, "fused"), (33, "unfused"), (65, "fused"), (65, "unfused"), (72, "fused"), (72, "unfused")]


@pytest.fixture(params=STAGES, ids=[f"L{L}-{p}" for L, p in STAGES])
def stage(ctx, request):
    return Stage(ctx, *request.param)


def zero(L):
    return np.zeros(2 * L, f32)


def test_small_at_its_threshold(stage):
    """min_size 128: the body spans 96 pixels; the last landmark, moved out by the bias, makes the extent exactly 128 (tracked) or
    the next float32 below 128 (SMALL), in x and separately in y (the other extent is 144 throughout, by its last coordinate too)."""
    L, below = stage.L, np.nextafter(f32(128), f32(0))
    box = [[0, 0, 128, 128]]
    for axis in (0, 1):
        b = zero(L)
        b[axis * L + L - 1] = 1.25                               # the last landmark: 64 -> -16, the far edge of the body is 112
        b[(1 - axis) * L + L - 1] = 1.5                          # the other axis: 64 -> -32
        seen = []
        for tweak, extent in ((0.0, f32(128)), (2.0 ** -24, below)):      # (the last landmark starts 2^-17 pixels further in)
            last = [0.0, 0.0]; last[axis] = tweak
            x0, x1, lost = stage.step(grid_mean(L, last), b, box, [0], min_size=128.0)
            c, o = x1[0, axis * L:(axis + 1) * L], x1[0, (1 - axis) * L:(2 - axis) * L]
            assert c.argmin() == L - 1 and (c[:L - 1] > c[L - 1]).all() and c[:L - 1].max() - c[:L - 1].min() == 96
            assert f32(c.max() - c.min()) == extent and f32(o.max() - o.min()) == 144
            seen.append(int(lost[0]))
        assert seen == [0, T.SMALL]
    assert np.array_equal(stage.mask64(), [T.SMALL])


def test_outside_at_the_frame_edges(stage):
    """The centre of the enclosing box exactly 0 and exactly the largest float32 below the width / height: inside.  Exactly the
    width, exactly the height, just below 0: OUTSIDE.  The frames are ragged, so the same row is inside on one image and outside on
    another; the box's near edge is the last landmark's."""
    L = stage.L
    b = zero(L)
    b[L - 1], b[2 * L - 1] = 1.25, -1.25                          # last landmark: x 64 -> -16 (x-minimum), y 64 -> 144 (y-maximum)
    # centre (bx + 48, by + 80)
    (w0, h0), (w1, h1), (w2, h2) = SIZES
    rows = [((-48, 20), 0, 0), ((w0 - 48, 20), 0, T.OUTSIDE), ((w2 - 48, -10), 2, T.OUTSIDE), ((w2 - 48, -10), 0, 0),
            ((10, -80), 1, 0), ((10, h1 - 80), 1, T.OUTSIDE), ((10, h0 - 80), 0, T.OUTSIDE), ((10, h0 - 80), 1, 0)]
    boxes = [[x, y, 128, 128] for (x, y), _, _ in rows]
    x0, x1, lost = stage.step(grid_mean(L), b, boxes, [im for _, im, _ in rows])
    assert np.array_equal(lost, [want for _, _, want in rows])
    assert (x1[:, L - 1:L] < x1[:, :L - 1]).all() and (x1[:, 2 * L - 1:] > x1[:, L:2 * L - 1]).all()
    cx = (x1[:, :L].min(1) + x1[:, :L].max(1)) * f32(0.5)
    cy = (x1[:, L:].min(1) + x1[:, L:].max(1)) * f32(0.5)
    assert cx[0] == 0.0 and cx[1] == w0 and cx[2] == w2 and cy[4] == 0.0 and cy[5] == h1 and cy[6] == h0
    assert np.array_equal(stage.mask64(), lost)
    # just below 0: the last landmark 2^-17 pixels further out
    x0, x1, lost = stage.step(grid_mean(L, (-2.0 ** -24, 0.0)), b, [[-48, 20, 128, 128]], [0])
    assert f32(x1[0, :L].min() + x1[0, :L].max()) * f32(0.5) == -2.0 ** -18 and lost[0] == T.OUTSIDE
    b2 = zero(L)
    b2[L - 1], b2[2 * L - 1] = 1.25, 1.25                         # the last landmark the near edge in y too: 64 -> -16
    x0, x1, lost = stage.step(grid_mean(L, (0.0, -2.0 ** -24)), b2, [[10, -48, 128, 128]], [1])
    assert f32(x1[0, L:].min() + x1[0, L:].max()) * f32(0.5) == -2.0 ** -18 and lost[0] == T.OUTSIDE
    # the largest float32 below the width / the height: near edge 16 - 2^-15 (the last landmark), far edge 2 W - 16
    for axis, im in ((0, 0), (1, 1)):
        size = SIZES[im][axis]
        far = 2 * size - 16
        origin = far - 112
        near = f32(16) - f32(2.0 ** -15)
        start = f32(near + f32(80))                               # where the last landmark starts: the bias takes 80 off
        m_last = f32(f32(f32(start - f32(origin)) / f32(128)) - f32(0.5))
        last = [0.0, 0.0]; last[axis] = float(m_last)
        box = [20, 20, 128, 128]; box[axis] = origin
        bb = zero(L); bb[axis * L + L - 1] = 1.25
        x0, x1, lost = stage.step(grid_mean(L, last), bb, [box], [im])
        c = x1[0, axis * L:(axis + 1) * L]
        assert c.argmin() == L - 1 and c[L - 1] == near and c.max() == far
        centre = f32(c.min() + c.max()) * f32(0.5)
        assert centre == np.nextafter(f32(size), f32(0)) and lost[0] == 0
        box[axis] = origin + 1                                    # one pixel on: the centre is beyond the size
        x0, x1, lost = stage.step(grid_mean(L, last), bb, [box], [im])
        c = x1[0, axis * L:(axis + 1) * L]
        assert f32(c.min() + c.max()) * f32(0.5) >= size and lost[0] == T.OUTSIDE


def test_scale_at_its_threshold(stage):
    """max_scale_change 2: the inter-eye distance 64 -> exactly 128 and exactly 32 is tracked, one step of the bias grid beyond
    either is SCALE; max_scale_change 0 switches the rule off."""
    L = stage.L
    (r0, r1), (l0, l1) = eyes(L)
    box, im = [[16, 8, 128, 128]], [0]
    step = 1.0 + 2.0 ** -10

    def run(right, left, k=2.0):
        b = zero(L)
        b[[r0, r1]] = right
        b[[l0, l1]] = left
        x0, x1, lost = stage.step(grid_mean(L), b, box, im, max_scale=k)
        assert T.ied(x0, *eyes(L))[0] == 64.0
        return T.ied(x1, *eyes(L))[0], int(lost[0])

    assert run(0.5, -0.5) == (128.0, 0)                           # growing: r = s k exactly
    r, m = run(0.5, [-0.5, -0.5 * step])
    assert 128.0 < r < 128.1 and m == T.SCALE
    assert np.array_equal(stage.mask64(), [T.SCALE])
    assert run(-0.25, 0.25) == (32.0, 0)                          # shrinking: r k = s exactly
    r, m = run(-0.25, [0.25, 0.25 * step])
    assert 31.9 < r < 32.0 and m == T.SCALE
    assert np.array_equal(stage.mask64(), [T.SCALE])
    assert run(0.5, [-0.5, -0.5 * step], k=0.0)[1] == 0           # the rule switched off
    assert run(-0.25, [0.25, 0.25 * step], k=0.0)[1] == 0
    assert run(0.0, 0.0) == (64.0, 0)


def test_nonfinite_in_every_turn_of_the_scan(stage):
    """A bias of 2^120 overflows float32 where the inter-eye distance is 2^9 (boxes of 1024) and not where it is 2^6 (boxes of 128):
    the overflowing rows are NONFINITE alone, whatever else their box would say, and their slots keep the row."""
    L = stage.L
    boxes = [[16, 8, 128, 128], [-400, -300, 1024, 1024], [20, 10, 128, 128], [5000, 10, 1024, 1024]]
    big = np.array([False, True, False, True])
    coords = [5, 65] + ([129] if 2 * L > 129 else [])             # first, second and third turn of `for (j = lane; j < 2L; j += 64)`
    for j in coords:
        assert j // 64 == coords.index(j) and j not in sum(eyes(L), []) and j - L not in sum(eyes(L), [])
        b = zero(L)
        b[j] = 2.0 ** 120
        x0, x1, lost = stage.step(grid_mean(L), b, boxes, [0, 1, 2, 0])
        assert np.array_equal(np.isinf(x1).any(1), big) and np.isinf(x1[big, j]).all() and np.isfinite(np.delete(x1, j, 1)).all()
        assert (lost[big] == T.NONFINITE).all()
        assert (lost[~big] & T.NONFINITE == 0).all() and np.isfinite(x1[~big]).all()
        assert np.array_equal(stage.mask64(), lost)
    # and no bias at all: the same rows are finite, the 128-pixel faces tracked
    x0, x1, lost = stage.step(grid_mean(L), zero(L), boxes, [0, 1, 2, 0])
    assert np.array_equal(bits(x1), bits(x0)) and (lost[~big] == 0).all() and (lost & T.NONFINITE == 0).all()
