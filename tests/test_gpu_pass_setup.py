"""The pass set-up of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_pass_setup.txt): a wave
requests what depends on (level, pass, lane) only -- its lane_tab entry, the fold weights, the pass's four words, the band-weight
rows -- before the geometry's arithmetic, takes the pass's words from ONE 16-byte load and picks its segment's by selects, and clears
its column rows with stores at constant offsets.  Checked against the CPU oracle at the shapes where a set-up can go wrong: the
integer decisions (sdm_get_patch_indices) are the oracle's, the feature rows read through the raw cells (hog_split_store) are inside
the standing bounds of the packed mode (pixel_kernel_cases.check_cells), and a four-level detect with random regressors is, bit for
bit, the same four levels stepped one at a time.

Shapes: 1, 3 and 7 faces on 256 x 256 noise images and two ragged sets of frames with differing sizes and strides; L = 5, 22, 32
and 33 (2L = 64 and 66: either side of the fused detect's limit); all four shipped levels; eye counts (1, 1), (2, 2), (3, 3), (4, 4)
and (1, 4): the reciprocal and the division branch of the eye centres.  The face counts make a workgroup's four waves straddle two
faces and leave the last workgroup partial (asserted from the plans, tests/test_gpu_fold_overlap.py).  Rows: landmarks on x.5 (cvRound
ties), negative coordinates, patches off every border, small and large faces.  L = 1 has one landmark for both eyes, so its inter-eye
distance is zero: with it and with a tiny face SDM_ERR_EMPTY_PATCH must still be reported.

Half-width sweep: eyes on a horizontal line, the left one at x = 0 so that the float difference IS the right eye's x, chosen so
that rel * IED / 2 lands on k + 1/2, within a few float steps of it either side, and 2^-10 either side of it, for several k at each
level's rel (k = 127 reaches the end of the taps table): h must be the oracle's round() in double, ties included.

The detect-against-stepped-levels comparison runs the same kernel on both sides: it pins the launch sequence, not the set-up.  What
can see a set-up error are the index and the feature comparisons with the oracle."""
import numpy as np
import pytest

from oracle import sdm_oracle as orc
from pixel_kernel_cases import (EYE_CASES, L22, LE22, RE22, RELS, SHIPPED, SIZES, cells_features, check_cells,
                                detect_equals_stepped_levels, edge_rows, face, noise, options, oracle_indices, oracle_per_row,
                                tie_sweep_rows)  # noqa: F401
from superviseddescent_amd import SdmError


def _check_against_the_oracle(gpu_ctx, x, L, re, le, row_images, what, stepped=True):
    """Feature rows of the four levels through the raw cells and the patch indices of each against the oracle (`row_images`: one
    image per row of x), then a four-level detect against the same levels stepped one at a time."""
    gpu_ctx.set_option("hog_split_store", 1)
    for lv in range(4):
        got, idx = cells_features(gpu_ctx, x, lv)
        want, widx = oracle_per_row(row_images, x, re, le, lv)
        assert np.array_equal(widx, oracle_indices(x, L, re, le, RELS[lv])), (what, lv)
        check_cells(got, idx, want, widx, "%s, level %d" % (what, lv))
    if stepped:
        detect_equals_stepped_levels(gpu_ctx, x, L, seed=6)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(EYE_CASES))
def test_set_up_against_the_oracle(gpu_ctx, options, case):
    L, re, le = EYE_CASES[case]
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    rows = edge_rows(L, re, le, seed=1000 + L + len(re) * 7 + len(le))
    for n, pick in ((1, slice(1, 2)), (3, slice(2, 5)), (7, slice(0, 7))):
        images = noise(n, seed=40 + n)
        gpu_ctx.upload_images(images)
        gpu_ctx.set_sample_image_index(None)
        _check_against_the_oracle(gpu_ctx, rows[pick], L, re, le, images, "%s, %d faces" % (case, n))


@pytest.mark.gpu
@pytest.mark.parametrize("frames", ["four-by-half-width", "seven-edge-rows"])
def test_ragged_frames_with_differing_strides(gpu_ctx, options, frames):
    """Frames of differing sizes and pitches, the samples in another order than the frames: the image borders stay per patch."""
    import torch
    if frames == "four-by-half-width":       # RCR-22's eyes, one face per frame placed by its half-width
        L, re, le = L22, RE22, LE22
        sizes = [(256, 256, 256), (200, 240, 320), (256, 130, 384), (131, 133, 192)]      # h, w, pitch
        order, seed = np.array([3, 1, 0, 2], np.int32), 591
        x = np.stack([face(L, re, le, h0, c, seed=600 + i, spread=40.0)
                      for i, (h0, c) in enumerate(((24, (60, 70)), (31, (130, 90)), (40, (128, 128)), (27, (70, 120))))])
    else:                                    # three landmarks per eye, the edge rows at half size, and the stepped detect
        L, re, le = EYE_CASES["L22-eyes3+3"]
        sizes = [(256, 256, 256), (200, 240, 320), (256, 130, 384), (97, 256, 257), (256, 256, 512), (255, 201, 300), (131, 133, 192)]
        order, seed = np.array([3, 1, 6, 0, 2, 5, 4], np.int32), 78
        x = edge_rows(L, re, le, seed=77)
        x[:, :L] *= np.float32(0.5)                          # (the smallest frame is 131 x 133)
        x[:, L:] *= np.float32(0.5)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    rng = np.random.default_rng(seed)
    host = [rng.integers(0, 256, (h, pitch)).astype(np.uint8) for h, _, pitch in sizes]
    keep = [torch.from_numpy(a).cuda() for a in host]
    gpu_ctx.set_frames_device([t[:, :w] for t, (_, w, _) in zip(keep, sizes)])
    gpu_ctx.set_sample_image_index(order)
    _check_against_the_oracle(gpu_ctx, x, L, re, le, [host[i][:, :sizes[i][1]] for i in order], "ragged, " + frames,
                              stepped=frames == "seven-edge-rows")
    gpu_ctx.upload_images(noise(1, seed=1))                  # (the frames go out of scope)


@pytest.mark.gpu
def test_empty_patch_is_still_reported(gpu_ctx, options):
    gpu_ctx.upload_images(noise(3, seed=9))

    def codes(x, detect=True):
        """The status of the four levels' feature rows through the raw cells, then of a four-level detect."""
        out = []
        gpu_ctx.set_option("hog_split_store", 1)
        for lv in range(4):
            gpu_ctx.set_x(x)
            try:
                gpu_ctx.hog_features(lv, fetch=True)
                out.append(0)
            except SdmError as e:
                out.append(e.code)
        gpu_ctx.set_option("hog_split_store", 0)
        if detect:
            gpu_ctx.set_x(x)
            try:
                gpu_ctx.detect_batch()
                out.append(0)
            except SdmError as e:
                out.append(e.code)
        return out

    # one landmark: both eye centres are that landmark, the inter-eye distance is 0
    gpu_ctx.set_model_geometry(1, [0], [0], SHIPPED)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, np.zeros((gpu_ctx.feature_dim(lv), 2), np.float32))
    assert codes(np.array([[100.25, 90.5], [3.0, 250.0], [128.0, 128.0]], np.float32)) == [-4] * 5
    # a face of two pixels between two good ones: rel * IED / 2 < 1 / 2 at every level
    L, re, le = EYE_CASES["L22-eyes3+3"]
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, np.zeros((gpu_ctx.feature_dim(lv), 2 * L), np.float32))
    x = edge_rows(L, re, le, seed=5)[:3]
    x[1] = (128.0 + (x[1] - 128.0) * np.float32(0.01)).astype(np.float32)
    assert all(float(np.float32(r)) * orc.get_ied(x[1], re, le) / 2.0 < 0.49 for r in RELS)
    assert codes(x) == [-4] * 5
    # and the same context goes on working
    assert codes(edge_rows(L, re, le, seed=5)[:3]) == [0] * 5
    # the same with RCR-22's eyes and faces of half-widths 30, 36 and 41, the feature rows alone
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(noise(3, seed=611))
    good = np.stack([face(L22, RE22, LE22, h0, (128, 128), seed=620 + i) for i, h0 in enumerate((30, 36, 41))])
    bad = good.copy()
    bad[1] = (128.0 + (bad[1] - 128.0) * np.float32(0.01)).astype(np.float32)
    assert all(r * orc.get_ied(bad[1], RE22, LE22) / 2.0 < 0.49 for r in RELS)
    assert codes(bad, detect=False) == [-4] * 4
    assert codes(good, detect=False) == [0] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_half_width_sweep_around_the_ties(gpu_ctx, options, level):
    L, re, le = 5, [0], [1]
    rel, S = RELS[level], SIZES[level]
    ks = sorted({0, 1, 3, S // 2 - 1, S // 2, S // 2 + 1, S, 100, 126, 127})
    x, ds, t = tie_sweep_rows(rel, ks)
    # the sweep is the one intended: t on a tie, within a float step of it on either side, and on both sides of the guard's edges
    frac = t - np.floor(t)
    assert (frac == 0.5).sum() >= len(ks) // 2 and (t[frac == 0.5] < 128).all()
    dist = np.abs(frac.astype(np.float64) - 0.5)
    assert ((dist > 0) & (dist < 2.0 ** -12)).any() and ((dist > 2.0 ** -10) & (dist < 1.01 * 2.0 ** -10)).any() \
        and ((dist < 2.0 ** -10) & (dist > 0.99 * 2.0 ** -10)).any()
    want_h = np.floor(np.float64(np.float32(rel)) * ds.astype(np.float64) / 2.0 + 0.5).astype(np.int64)
    assert np.array_equal(want_h, [int(np.floor(float(np.float32(rel)) * orc.get_ied(r, re, le) / 2.0 + 0.5)) for r in x])
    assert want_h.min() == 0 and want_h.max() == 128
    keep = want_h >= 1                                       # (h = 0 is the empty patch: reported, see test_empty_patch_is_still_reported)
    x, want_h = x[keep], want_h[keep]
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    gpu_ctx.upload_images(noise(4, seed=31))
    gpu_ctx.set_sample_image_index((np.arange(x.shape[0]) % 4).astype(np.int32))

    options("hog_split_store", 1)
    f, idx = cells_features(gpu_ctx, x, level)
    print("level %d: %d rows, h %d .. %d" % (level, x.shape[0], want_h.min(), want_h.max()))
    assert np.isfinite(f).all() and np.array_equal(idx[:, 0], want_h)
    assert np.array_equal(idx[:, 1:], [[orc.cv_round(c) for c in r] for r in x])
