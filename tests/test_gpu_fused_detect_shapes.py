"""The fused descriptor x regressor launch (csrc/sdm_desc.hip, desc_kernel<..., FUSED>) and the sum over the landmarks behind it
(csrc/sdm_apply.hip, apply_reduce_kernel) at every shape they serve, not only RCR-22's three column tiles and RCR-68's nine:

* every column-tile count NT = ceil(2L / 16) = 1 ... 9 at both of its edges, on both wave layouts -- KPARTS = 2 x 4 waves
  (4 orientations, 32 faces per workgroup: a second round of tiles from NT = 5, a third at NT = 9) and KPARTS = 4 x 2 waves
  (9 orientations, 16 faces per workgroup: rounds from NT = 3, five of them at NT = 9);
* the partial sums of L = 24 | 25 landmarks, where apply_reduce_kernel's batches of 24 take a clamped second turn;
* N = 1, 31, 33 and 70 rows: a partial face tile for both tile sizes, one workgroup and several;
* one output column x 37 in the LAST column tile, so the tile's power-of-two scale is read by the last round, one x 1e-3.

A one-level cascade on rows that are given (teacher-forced): patch decisions bit for bit the oracle's for every face, fused against
the unfused path of the same context and against float64, run-to-run identical bits, and the launch observed to have run.  Then one
free-running three-level cascade of 30 landmarks per wave layout against the oracle cascade.  The bounds are those of
tests/test_gpu_fused_detect.py; measurements at these shapes: profiles/landmark_count_tests.txt.

These shapes showed that the 16-face (9-orientation) fused launch was not run-to-run deterministic once its grid had more workgroups
than the chip has compute units (csrc/sdm_desc.hip, launch_desc; profiles/landmark_count_tests.txt, "Run-to-run bits"): the last test
repeats such grids."""
import os

import numpy as np
import pytest

import landmark_count_cases as K
from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, SdmError, ibug, synth

gpu = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
LAYOUTS = {"uoctti16-kparts2": (1, 5, 6, 4, 0.6), "uoctti31-kparts4": (1, 5, 8, 9, 0.7), "dalaltriggs36-kparts4": (0, 5, 8, 9, 0.7)}
L_DEFAULT = [2, 8, 9, 16, 17, 24, 25, 32]                       # fused by default (2L <= 64): both edges of NT = 1 ... 4, and 24 | 25
L_WIDE = [33, 40, 41, 48, 56, 57, 64, 65, 72]                   # fused on request: NT = 5 ... 9 and the C-ABI's limit
L_NINE = [8, 9, 17, 25, 33, 41, 56, 57, 65, 72]                 # the 9-orientation layouts: one L per NT (1 ... 9), and 72
ROWS = (1, 31, 33, 70)
CASES = [("uoctti16-kparts2", L) for L in L_DEFAULT + L_WIDE] + [(lay, L) for lay in ("uoctti31-kparts4", "dalaltriggs36-kparts4") for L in L_NINE]
# three free-running levels per wave layout
FREE = {"kparts2": [(1, 5, 10, 4, 0.7), (1, 5, 8, 4, 0.4), (1, 5, 6, 4, 0.25)],
        "kparts4": [(1, 5, 10, 9, 0.7), (1, 5, 8, 9, 0.4), (1, 5, 6, 9, 0.25)]}
FREE_L, FREE_N, FREE_SEED = 30, 70, 421
FLIP_SHARE = 0.02                                                # test_fused_detect_against_unfused_and_oracle's own share


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def faces(n, seed, off_canvas=True):
    """n synthetic faces at 256 x 256 and the rows of all 68 landmarks they start from; a few rows moved so that patches straddle
    or leave the image (row 0 stays: the batch of one row is an ordinary face)"""
    images, boxes, gt = synth.make_faces(n, seed=seed)
    _, x0, _ = synth.make_samples(boxes, gt, ibug.IBUG68_IDS, n_perturb=0, seed=seed + 1)
    if off_canvas:
        x0 = x0.copy()
        x0[1:4, :68] -= 150.0
        x0[4:7, 68:] += 170.0
    return images, x0


@pytest.fixture(scope="module")
def one_level_faces():
    return faces(max(ROWS), 401)


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    yield gpu_ctx
    gpu_ctx.set_detect_path(fused=True, split_store=False)


def random_regressor(F, L, level=0, seed=5):
    """as random_model of test_gpu_fused_detect.py, the large column in the last column tile"""
    rng = np.random.default_rng(seed + 1000 * level + L)
    R = (rng.standard_normal((F, 2 * L)) * (0.004 * (22.0 / L) ** 0.5 / (level + 1))).astype(np.float32)
    R[:, 2 * L - 1] *= 37.0
    R[:, 1] *= 1e-3
    return R


def fused_mode(L):
    return True if 2 * L <= 64 else "wide"


def assert_no_feature_rows(c):
    """A fused level writes no feature rows, so sdm_apply has nothing to apply afterwards; a level that fell back to feature rows
    + apply GEMM leaves them (shown on the unfused run of every case)."""
    with pytest.raises(SdmError):
        c.apply(0)


@gpu
@pytest.mark.parametrize("layout,L", CASES, ids=[f"{lay}-L{L}" for lay, L in CASES])
def test_fused_level_at_every_column_tile_count(ctx, one_level_faces, layout, L):
    images, x68 = one_level_faces
    hp, ohp = HoGParam(*LAYOUTS[layout]), orc.HoGParam(*LAYOUTS[layout])
    _, re, le = K.landmark_set(L)
    x_all = K.rows(x68, L)
    ctx.set_model_geometry(L, re, le, [hp])
    ctx.upload_images(images)
    ctx.set_sample_image_index(None)
    F = ctx.feature_dim(0)
    assert F == L * hp.patch_dim + 1
    R = random_regressor(F, L)
    ctx.set_regressor(0, R)
    ofeat, oidx = orc.hog_features_batch(images, None, x_all, re, le, ohp, n_threads=THREADS, want_idx=True)
    ied = 1.0 / orc.InterEyeDistanceNormalisation(re, le)(x_all)[:, :1].astype(np.float64)
    want = x_all.astype(np.float64) - (ofeat.astype(np.float64) @ R.astype(np.float64)) * ied
    for n in ROWS:
        x0 = x_all[:n]
        ctx.set_detect_path(fused=False)
        ctx.set_x(x0); x_unfused = ctx.detect_batch()
        assert np.array_equal(ctx.patch_indices(), oidx[:n])
        ctx.apply(0)                                                   # (the unfused level left its feature rows)
        ctx.set_detect_path(fused=fused_mode(L))
        ctx.set_x(x0); x_fused = ctx.detect_batch()
        assert np.array_equal(ctx.patch_indices(), oidx[:n])           # every face: none is left out of anything below
        assert_no_feature_rows(ctx)
        got = ctx.get_x()
        assert got.shape == (n, 2 * L) and np.isfinite(got).all() and np.array_equal(bits(got), bits(x_fused))
        ctx.set_x(x0); x_again = ctx.detect_batch()
        assert np.array_equal(bits(x_fused), bits(x_again))
        per_face = np.linalg.norm((x_fused - x_unfused).astype(np.float64), axis=1) / np.linalg.norm(x_unfused.astype(np.float64), axis=1)
        r64, u64 = rel_l2(x_fused, want[:n]), rel_l2(x_unfused, want[:n])
        print(f"{layout} L {L} NT {(2 * L + 15) // 16} N {n}: fused vs unfused median {np.median(per_face):.2e} max {per_face.max():.2e}; "
              f"vs float64 fused {r64:.2e} unfused {u64:.2e}")
        assert np.median(per_face) < 2e-7 and per_face.max() < 1e-4, (n, np.median(per_face), per_face.max())
        assert r64 < 1e-5, (n, r64)


def free_case():
    images, x68 = faces(FREE_N, FREE_SEED, off_canvas=False)
    return images, K.rows(x68, FREE_L)


def oracle_cascade(images, x0, re, le, params, Rs, accumulate_double):
    """the oracle's free-running cascade: (result rows, the patch decisions of every level)"""
    regs = []
    for R in Rs:
        r = orc.LinearRegressor(accumulate_double=accumulate_double); r.x = R; regs.append(r)
    ohog = orc.HogTransform(images, [orc.HoGParam(*p) for p in params], re, le, None, n_threads=THREADS)
    ohog.keep_idx = True
    x = orc.SupervisedDescentOptimiser(regs, orc.InterEyeDistanceNormalisation(re, le)).test(x0, None, ohog)
    return x, [ohog.idx_per_level[l].copy() for l in range(len(params))]


def free_regressors(params, L):
    return [random_regressor(L * HoGParam(*p).patch_dim + 1, L, level=l) for l, p in enumerate(params)]


@pytest.mark.parametrize("layout", list(FREE))
def test_free_running_seed_keeps_the_oracles_own_flips_rare(built, layout):
    """On the CPU: the oracle with a float32-accumulating predict against the double-accumulating one from the same rows.  Faces
    whose patch decisions differ between the two flip at a cvRound boundary on rounding noise alone; for the seed of the
    free-running case below they stay within the share that case allows."""
    params = FREE[layout]
    _, re, le = K.landmark_set(FREE_L)
    images, x0 = free_case()
    Rs = free_regressors(params, FREE_L)
    _, idx64 = oracle_cascade(images, x0, re, le, params, Rs, True)
    _, idx32 = oracle_cascade(images, x0, re, le, params, Rs, False)
    flipped = np.zeros(FREE_N, bool)
    for a, b in zip(idx64, idx32):
        flipped |= (a != b).any(1)
    print(f"{layout}: {int(flipped.sum())} of {FREE_N} faces flip an integer decision between float32 and double accumulation")
    assert flipped.mean() <= FLIP_SHARE


@gpu
@pytest.mark.parametrize("layout", list(FREE))
def test_fused_free_running_30_landmarks(ctx, layout):
    """Three free-running levels, L = 30 (four column tiles, partial sums in two batches), N = 70: the fused cascade against the
    oracle's within 1e-4; the faces whose integer patch decisions differ from the oracle's at some level are reported apart and
    may be at most 2 % of the rows."""
    params = FREE[layout]
    _, re, le = K.landmark_set(FREE_L)
    images, x0 = free_case()
    ctx.set_model_geometry(FREE_L, re, le, [HoGParam(*p) for p in params])
    ctx.upload_images(images)
    ctx.set_sample_image_index(None)
    Rs = free_regressors(params, FREE_L)
    for l, R in enumerate(Rs):
        ctx.set_regressor(l, R)
    x_orc, oidx = oracle_cascade(images, x0, re, le, params, Rs, True)
    ctx.set_x(x0)
    flipped = np.zeros(FREE_N, bool)
    for l in range(len(params)):
        ctx.detect_level(l)
        flipped |= (ctx.patch_indices() != oidx[l]).any(1)
        assert_no_feature_rows(ctx)
    x_levels = ctx.get_x()
    ctx.set_x(x0); x_fused = ctx.detect_batch()
    assert np.array_equal(bits(x_fused), bits(x_levels))              # (detect_level runs detect_batch's launches)
    assert x_fused.shape == (FREE_N, 2 * FREE_L) and np.isfinite(x_fused).all()
    keep = ~flipped
    rel = rel_l2(x_fused[keep], x_orc[keep])
    print(f"{layout}: fused vs oracle cascade rel-L2 {rel:.2e} on {int(keep.sum())} faces; faces with a flipped integer decision: {np.flatnonzero(flipped).tolist()}")
    assert flipped.mean() <= FLIP_SHARE
    assert rel < 1e-4


@gpu
@pytest.mark.parametrize("layout,L,n", [("uoctti31-kparts4", 22, 512), ("dalaltriggs36-kparts4", 72, 70), ("dalaltriggs36-kparts4", 9, 1024),
                                         ("uoctti16-kparts2", 22, 1024)], ids=lambda v: str(v))
def test_fused_repeats_are_bit_identical_on_grids_larger_than_the_chip(ctx, one_level_faces, layout, L, n):
    """ceil(n / 16) x L (9 orientations) or ceil(n / 32) x L (4 orientations) workgroups, 360 ... 1 408 of them: more than the 256
    compute units, so workgroups follow one another on a CU.  Twelve repeats give the first run's bits, and those are the unfused
    path's within the bounds above.  (Before the 16-face instances were given a CU each, every repeat of the first case differed from
    the run before it in some face, by up to 1.4 pixels.)"""
    images, x68 = one_level_faces
    hp = HoGParam(*LAYOUTS[layout])
    _, re, le = K.landmark_set(L)
    index = (np.arange(n) % len(images)).astype(np.int32)
    x0 = K.rows(x68, L)[index]
    ctx.set_model_geometry(L, re, le, [hp])
    ctx.upload_images(images)
    ctx.set_sample_image_index(index)
    ctx.set_regressor(0, random_regressor(ctx.feature_dim(0), L))
    ctx.set_detect_path(fused=False)
    ctx.set_x(x0); x_unfused = ctx.detect_batch()
    ctx.set_detect_path(fused=fused_mode(L))
    ctx.set_x(x0); first = ctx.detect_batch()
    assert_no_feature_rows(ctx)
    for r in range(12):
        ctx.set_x(x0); again = ctx.detect_batch()
        differ = np.flatnonzero((bits(again) != bits(first)).any(1))
        assert differ.size == 0, (r, differ.tolist(), float(np.abs(again - first).max()))
    per_face = np.linalg.norm((first - x_unfused).astype(np.float64), axis=1) / np.linalg.norm(x_unfused.astype(np.float64), axis=1)
    assert np.median(per_face) < 2e-7 and per_face.max() < 1e-4
    ctx.set_sample_image_index(None)
