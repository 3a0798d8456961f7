"""Upright-normalised detect and tracking without a GPU: the C-ABI's declarations, the restated rules (tests/upright_ref.py) against
plain geometry, and the closed loop -- roll from the previous frame's eye line, upright chip, realign in the chip, cascade, map back
-- run with the CPU oracle on a video of turning faces.  This proves the rule set, not the kernels (tests/test_gpu_upright.py)."""
import os
import re

import numpy as np

import align_ref as A
import track_ref as T
import upright_cases as C
import upright_ref as U
from superviseddescent_amd import _lib, ibug, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdm_upright_configure", "sdm_detect_batch_upright", "sdm_upright_get", "sdm_track_configure_upright", "sdm_track_start_rolled"]
# the bound of tests/test_gpu_upright.py::test_tracking_accuracy_on_turning_faces: the worst frame's mean error over frame 0's
# (here, with a compact three-level cascade on the oracle: 1.13, 0.0317 against 0.0281 over 12 frames)
TRACK_RATIO = 1.35


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "sdm.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in _lib.EXPORTED, n
    assert re.search(r"#define\s+SDM_UPRIGHT_PARTIAL\s+1\b", text) and re.search(r"#define\s+SDM_UPRIGHT_NEAR_EDGE\s+2\b", text)
    assert (_lib.SDM_UPRIGHT_PARTIAL, _lib.SDM_UPRIGHT_NEAR_EDGE) == (U.PARTIAL, U.NEAR_EDGE) == (1, 2)


def test_roll_is_exact_at_right_angles():
    assert U.roll_cs(0) == (1.0, 0.0) and U.roll_cs(90) == (0.0, 1.0) and U.roll_cs(180) == (-1.0, 0.0)
    assert U.roll_cs(-90) == (0.0, -1.0) and U.roll_cs(270) == (0.0, -1.0) and U.roll_cs(360) == (1.0, 0.0) and U.roll_cs(-450) == (0.0, -1.0)
    c, s = U.roll_cs(30)
    assert abs(c - np.sqrt(3) / 2) < 1e-15 and abs(s - 0.5) < 1e-15          # clockwise on screen: the eye line points down-right


def test_w_inverts_m_over_a_1024_chip():
    """1e-4 px where every coordinate the matrices hold or produce stays below 1 024 (float32 spacing 6e-5 there): the rounding of the
    two translations, half a spacing each, and of c and s (1.2e-7 x at most 724 px from the chip centre) share that bound.  A centre
    further out has coarser float32 translations -- the spacing doubles at every power of two -- and the bound doubles with it."""
    chip = 1024
    g = np.linspace(0, chip - 1, 33)
    q = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    worst = 0.0
    for roll in (0, 0.5, 17.3, -33, 45, 90, 135, -150, 180, 271, 360.5):
        for ix, iy in ((160, 120), (511, 383), (3, 1900), (-40, 77)):
            M, W = U.matrices(*U.roll_cs(roll), ix, iy, chip)
            p = A.apply(M, q)                        # float64 on the float32 matrices
            err = np.abs(A.apply(W, p) - q).max()
            reach = max(np.abs(p).max(), abs(M[0, 2]), abs(M[1, 2]), abs(W[0, 2]), abs(W[1, 2]), chip)
            bound = 1e-4 * 2.0 ** max(0, int(np.ceil(np.log2(reach / 1024.0))))
            worst = max(worst, err / bound)
            assert err < bound, (roll, ix, iy, err, bound)
    print("W(M(q)) - q over a 1 024 chip: worst %.2f of the bound" % worst)


def test_chips_at_right_angles_are_copies_and_rotations():
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, (131, 97), dtype=np.uint8)
    for chip in (32, 64, 97):
        hc = chip // 2
        for box in ((20, 30, 40, 50), (-10, 100, 33, 61), (70, -5, 51, 30)):
            ix, iy = box[0] + box[2] // 2, box[1] + box[3] // 2
            # the frame padded with zeros, so that the chip region can be sliced: region[i, j] = frame[iy - hc + i, ix - hc + j]
            pad = 2 * chip
            big = np.zeros((frame.shape[0] + 2 * pad, frame.shape[1] + 2 * pad), np.uint8)
            big[pad:pad + frame.shape[0], pad:pad + frame.shape[1]] = frame
            M, _, _ = U.detect_setup([box], [0], chip)
            assert np.array_equal(U.chips(frame, M[0], chip), big[pad + iy - hc:pad + iy - hc + chip, pad + ix - hc:pad + ix - hc + chip])
            for roll, k in ((90, 1), (180, 2), (270, 3), (-90, 3)):
                M, _, _ = U.detect_setup([box], [roll], chip)
                # chip pixel (j, i) reads the frame at centre + R (j - hc, i - hc): the region of side 2 hc + 1 about the centre, turned
                # k quarter turns counter-clockwise as an array (np.rot90), holds the chip in its first `chip` rows and columns
                region = big[pad + iy - hc:pad + iy + hc + 1, pad + ix - hc:pad + ix + hc + 1]
                assert np.array_equal(U.chips(frame, M[0], chip), np.rot90(region, k)[:chip, :chip]), (chip, box, roll)


def test_chip_box_init_is_align_mean_minus_the_integer_offset():
    mean = ibug.select_mean(ibug.RCR22_IDS)
    rng = np.random.default_rng(2)
    for _ in range(200):
        chip = int(rng.integers(32, 1025))
        w, h = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        x, y = int(rng.integers(-50, 2000)), int(rng.integers(-50, 2000))
        cb = U.chip_box((x, y, w, h), chip)
        assert cb[2:] == (w, h)
        dx, dy = x - cb[0], y - cb[1]
        assert (dx, dy) == (x + w // 2 - chip // 2, y + h // 2 - chip // 2)
        a = synth.align_mean(mean, cb)
        b = synth.align_mean(mean, (x, y, w, h)).astype(np.float64)
        b[:22] -= dx
        b[22:] -= dy
        ulp = np.spacing(np.maximum(np.abs(synth.align_mean(mean, (x, y, w, h))), np.abs(a)).astype(np.float32))
        assert (np.abs(a - b) <= ulp).all()


def test_near_edge_rule():
    q = np.array([[10, 20, 10, 20], [3.9, 20, 10, 20], [10, 60.1, 10, 20], [10, 20, 10, np.nan], [4, 59, 4, 59]], np.float32)
    assert list(U.near_edge(q, 64, 4)) == [False, True, True, True, False]
    assert list(U.near_edge(q, 64, 0)) == [False, False, False, True, False]


def upright_step(run, frames, M, init):
    """chips of the rows' frames through M -> run(chips, init) -> the result in frame coordinates"""
    chip_stack = np.stack([U.chips(f, m, CHIP) for f, m in zip(frames, M)])
    return U.back(M, run(chip_stack, init))


CHIP = 288


def test_closed_loop_follows_turning_faces_on_the_oracle(built):
    from oracle import sdm_oracle as orc
    ids = ibug.RCR22_IDS
    re_, le_ = ibug.eye_indices(ids)
    mean = ibug.select_mean(ids)
    sel = np.array([ibug.IBUG68_IDS.index(i) for i in ids] + [68 + ibug.IBUG68_IDS.index(i) for i in ids])
    # a compact cascade trained with roll U(-12, 12) degrees: 300 faces x 4 rows
    rng = np.random.default_rng(31)
    images, boxes, gt = C.make_rolled_faces(300, rng.uniform(-12, 12, 300), seed=32)
    x_star, x0, idx = synth.make_samples(boxes, gt, ids, n_perturb=3, seed=33)
    params = [orc.HoGParam(1, 3, 12, 4, 1.0), orc.HoGParam(1, 3, 10, 4, 0.7), orc.HoGParam(1, 3, 8, 4, 0.4)]
    sdo = orc.SupervisedDescentOptimiser([orc.LinearRegressor(orc.Regulariser(orc.Regulariser.MATRIX_NORM, 1.5, False)) for _ in params],
                                         orc.InterEyeDistanceNormalisation(re_, le_))
    sdo.train(x_star, x0, None, orc.HogTransform(images, params, re_, le_, idx, n_threads=8))

    def run(chip_stack, init):
        return sdo.test(init, None, orc.HogTransform(np.ascontiguousarray(chip_stack), params, re_, le_, None, n_threads=8))

    def err(x, g):
        return float(orc.normalised_landmark_errors(x, g, re_, le_).mean())

    S, n_frames = 8, 12
    frames, gts, vboxes, rolls = C.make_rolled_tracks(S, n_frames, 2.5, seed=34)
    M, _, cb = U.detect_setup(vboxes, 0, CHIP)
    init = np.stack([synth.align_mean(mean, b) for b in cb])
    prev = upright_step(run, frames[0], M, init)
    e = [err(prev, gts[0][:, sel])]
    est = []
    for t in range(1, n_frames):
        M, W = U.track_setup(prev, re_, le_, CHIP)
        init = U.track_init(prev, W, mean)
        res = upright_step(run, frames[t], M, init)
        assert not T.lost_mask(init, res, 320, 320, 8.0, 1.5, re_, le_).any()
        e.append(err(res, gts[t][:, sel]))
        est.append(np.rad2deg(np.arctan2(M[:, 1, 0], M[:, 0, 0])).mean())
        prev = res
    print("closed loop on the oracle: error per frame " + " ".join("%.4f" % v for v in e))
    print("estimated roll per frame " + " ".join("%.1f" % v for v in est) + " (true %.1f .. %.1f)" % (rolls[1], rolls[-1]))
    assert max(e) <= TRACK_RATIO * e[0]
    # the estimated roll is one frame's turn behind the true roll
    assert np.abs(np.array(est) - rolls[:-1]).max() < 2.5
