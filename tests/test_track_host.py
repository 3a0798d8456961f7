"""No-GPU checks of the tracker's host side: the float32 restatement of its realign and lost rules (tests/track_ref.py) against
plain float64 versions, the synthetic video generator synth.make_tracks, and the C-ABI declarations of sdm_track_*."""
import hashlib
import os
import re

import numpy as np

import track_ref as T
from superviseddescent_amd import _lib, ibug, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ibug.RCR22_IDS
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)


def random_rows(n, seed):
    rng = np.random.default_rng(seed)
    boxes = np.stack([rng.integers(-20, 200, n), rng.integers(-20, 200, n), rng.integers(20, 200, n), rng.integers(20, 200, n)], 1)
    rows = np.stack([synth.align_mean(MEAN, b) for b in boxes])
    return (rows + rng.normal(0, 3, rows.shape)).astype(np.float32)


def test_realign_float32_matches_float64():
    prev = random_rows(500, 1)
    r32, r64 = T.realign(prev, MEAN), T.realign64(prev, MEAN)
    assert r32.dtype == np.float32
    scale = np.abs(r64).max(1, keepdims=True)
    assert (np.abs(r32 - r64) / scale).max() < 1e-6
    # the enclosing box of the result is the enclosing box of the previous row (the mean's extremes land on its edges)
    L = len(IDS)
    for a, b in ((r32, prev),):
        assert np.allclose(a[:, :L].min(1), b[:, :L].min(1), atol=1e-4) and np.allclose(a[:, :L].max(1), b[:, :L].max(1), atol=1e-3)
        assert np.allclose(a[:, L:].min(1), b[:, L:].min(1), atol=1e-4) and np.allclose(a[:, L:].max(1), b[:, L:].max(1), atol=1e-3)
    # a row that is already an aligned mean comes back (to rounding) as itself
    box_row = synth.align_mean(MEAN, (40, 50, 120, 130))
    assert np.abs(T.realign(box_row, MEAN)[0] - box_row).max() < 1e-4


def away_from_thresholds(init, res, W, H, min_size, k):
    """rows whose every lost quantity is at least 1e-3 (relative) away from its threshold"""
    L = res.shape[1] // 2
    x, y = res[:, :L].astype(np.float64), res[:, L:].astype(np.float64)
    w, h = x.max(1) - x.min(1), y.max(1) - y.min(1)
    cx, cy = (x.min(1) + x.max(1)) / 2, (y.min(1) + y.max(1)) / 2
    ok = (np.abs(w - min_size) > 1e-3 * min_size) & (np.abs(h - min_size) > 1e-3 * min_size)
    ok &= (np.abs(cx) > 1e-3) & (np.abs(cx - W) > 1e-3) & (np.abs(cy) > 1e-3) & (np.abs(cy - H) > 1e-3)
    a, b = T.ied(res, RE, LE), T.ied(init, RE, LE)
    ok &= (np.abs(a / b - k) > 1e-3) & (np.abs(b / a - k) > 1e-3)
    return ok


def test_lost_rule_float32_matches_float64():
    rng = np.random.default_rng(2)
    init = random_rows(2000, 3)
    # results: moved, rescaled about their centre, some collapsed or blown up, a few non-finite
    s = rng.choice([0.05, 0.6, 1.0, 1.3, 2.5], size=(2000, 1)).astype(np.float32)
    L = len(IDS)
    res = init.copy()
    for lo in (0, L):
        c = res[:, lo:lo + L].mean(1, keepdims=True)
        res[:, lo:lo + L] = (res[:, lo:lo + L] - c) * s + c + rng.normal(0, 40, (2000, 1)).astype(np.float32)
    res[::97, 5] = np.nan
    res[::101, L + 3] = np.inf
    W, H = rng.integers(150, 300, 2000), rng.integers(150, 300, 2000)
    for min_size, k in ((30.0, 1.5), (8.0, 1.2), (60.0, 0.0)):
        m32 = T.lost_mask(init, res, W, H, min_size, k, RE, LE)
        m64 = T.lost_mask64(init, res, W, H, min_size, k, RE, LE)
        keep = away_from_thresholds(init, np.nan_to_num(res), W, H, min_size, k if k > 0 else 2.0) | ~np.isfinite(res).all(1)
        assert keep.sum() > 1500
        assert np.array_equal(m32[keep], m64[keep])
        for bit in (T.NONFINITE, T.SMALL, T.OUTSIDE) + ((T.SCALE,) if k > 0 else ()):
            assert ((m32 & bit) != 0).any(), bit                   # every rule fires somewhere ...
        assert (m32 == 0).any()                                    # ... and some rows are tracked
        assert set(np.unique(m32[~np.isfinite(res).all(1)])) == {T.NONFINITE}
        if k == 0:
            assert not (m32 & T.SCALE).any()


def tracks_digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_make_tracks_is_deterministic_and_stays_in_the_frame():
    frames, gt, boxes = synth.make_tracks(6, 12, seed=11)
    assert frames.shape == (12, 6, synth.IMAGE_SIZE, synth.IMAGE_SIZE) and frames.dtype == np.uint8
    assert gt.shape == (12, 6, 136) and boxes.shape == (12, 6, 4) and boxes.dtype == np.int32
    again = synth.make_tracks(6, 12, seed=11)
    assert tracks_digest(frames, gt, boxes) == tracks_digest(*again)
    assert tracks_digest(frames, gt, boxes) != tracks_digest(*synth.make_tracks(6, 12, seed=12))
    assert (gt >= 0).all() and (gt < synth.IMAGE_SIZE).all()
    # the boxes move a few pixels and scale a few percent per frame; the ground truth is the aligned mean of the box + a fixed shape
    d = np.abs(np.diff(boxes.astype(np.int64), axis=0))
    assert d[..., :2].max() <= 5 and d[..., :2].max() >= 1
    ratio = boxes[1:, :, 2] / boxes[:-1, :, 2]
    assert (np.abs(ratio - 1) <= 0.04).all() and (ratio != 1).any()
    shape = gt - np.stack([np.stack([synth.align_mean(ibug.MEAN_IBUG_LFPW_68, b) for b in fb]) for fb in boxes])
    assert np.abs(shape - shape[0:1]).max() < 1e-4
    # every frame is a new image (noise), the same stream keeps its face
    assert not np.array_equal(frames[0, 0], frames[1, 0])


def test_make_faces_is_unchanged():
    """make_tracks shares make_faces' drawing code: the existing generator's output for the seeds the suite uses stays byte-identical."""
    expect = {(96, 101): "aaa4addf20d367a58f29e15e2d34a6bcfa801f3d762219dac70357e11b6c8603",
              (64, 303): "fca61ea796a71da55ba817c3bdcb3384ad698171862ecb57dcf0373c2b7b1947",
              (300, synth.SEED): "f56fd52d6c8176a0cf5241457085881fb37311ff9b113c969153f32a70db5254"}
    for (n, seed), digest in expect.items():
        assert tracks_digest(*synth.make_faces(n, seed=seed)) == digest, (n, seed)


def test_track_entry_points_are_declared_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdm.h")).read(), flags=re.S)
    names = ["sdm_track_configure", "sdm_track_start", "sdm_track_stop", "sdm_track_step", "sdm_track_get"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt) and n in _lib.EXPORTED
    consts = dict(re.findall(r"#define (SDM_TRACK_\w+) (\d+)", txt))
    for k, v in consts.items():
        assert getattr(_lib, k) == int(v), k
    assert len(consts) == 10
    assert (T.NONFINITE, T.SMALL, T.OUTSIDE, T.SCALE) == (_lib.SDM_TRACK_LOST_NONFINITE, _lib.SDM_TRACK_LOST_SMALL,
                                                          _lib.SDM_TRACK_LOST_OUTSIDE, _lib.SDM_TRACK_LOST_SCALE)
