"""Inputs and checks shared by the tests of the detect path's pixel kernel (hog_packed_kernel, CELLS form, csrc/sdm_hog_packed.hip):
tests/test_gpu_row_carry.py, test_gpu_pair_carry.py, test_gpu_pass_setup.py and test_gpu_fold_overlap.py.  A change of that kernel adds
its cases to those modules on top of what is here; importable without a GPU.

  SHIPPED, O_SHIPPED, RELS, SIZES      the four shipped levels: library and oracle parameters, relative patch sizes, S = 55 / 50 / 40 / 30
  IDS22, L22, RE22, LE22               the RCR-22 landmark set and its eye indices
  EYE_CASES                            six (L, right-eye indices, left-eye indices): eye counts 1 + 4 .. 4 + 4, L = 5, 22, 32, 33
  PACKED_MAX_ABS, PACKED_REL_L2        the packed mode's standing bounds against the oracle (tests/test_gpu_parity.py::check_features)

  bits(a), noise(n, seed, h, w)        float32 as uint32; n noise images
  units_per_face(level, L)             (units of the level's plan per face, the plan)
  odd_units_count()                    the first landmark count whose level-0 units per face are no multiple of four
  face(L, re, le, h, centre, ...)      one row of landmarks whose half-width at `level` is h
  edge_rows(L, re, le, seed)           seven rows: cvRound ties, negative coordinates, patches off every border, small and large faces
  oracle_indices(x, L, re, le, rel)    sdm_get_patch_indices restated: round(rel * IED / 2) in double, cvRound of every coordinate
  tie_sweep_rows(rel, ks)              rows that put rel * IED / 2 on k + 1/2 and a few float steps either side
  smooth_faces(n), scaled_rows(x0, level)    synthetic faces; one row per half-width 1 .. S, then rows off each border
  pair_sweep_rows(x0)                  scaled_rows of level 0, then EXTRA_H (either side of the pair loop's range) off each border

  oracle(images, x, re, le, levels)    {level: (feature rows, patch indices)}, image i for row i
  oracle_per_row(row_images, ...)      the same for one level where the images differ in size (ragged frames): one image per row

  cells_features(ctx, x, level)        (feature rows through the raw cells, patch indices)
  check_cells(got, idx, want, widx, what)    the integer patch decisions are equal, the features inside the two bounds
  detect_equals_stepped_levels(ctx, x, L, seed)    a four-level detect_batch against the same levels stepped one at a time
  options                              fixture: SDM_HOG_COLUMNS, no sample index; yields ctx.set_option; puts the options back
"""
import numpy as np
import pytest

from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, ibug, synth
from superviseddescent_amd._lib import SDM_HOG_COLUMNS
from superviseddescent_amd.engine import hog_plan

SHIPPED = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
O_SHIPPED = [orc.HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
RELS = [float(np.float32(p.relative_patch_size)) for p in SHIPPED]
SIZES = [p.num_cells * p.cell_size for p in SHIPPED]          # S = 55, 50, 40, 30
IDS22 = ibug.RCR22_IDS
L22 = len(IDS22)
RE22, LE22 = ibug.eye_indices(IDS22)

# (L, right-eye indices, left-eye indices): the reciprocal and the division branch of the eye centres, 2L = 64 and 66 either side of
# the fused detect's limit
EYE_CASES = {
    "L5-eyes1+4": (5, [0], [1, 2, 3, 4]),
    "L5-eyes2+2": (5, [0, 1], [3, 4]),
    "L22-eyes3+3": (22, [2, 5, 7], [10, 11, 20]),
    "L22-eyes1+1": (22, [21], [0]),
    "L32-eyes4+4": (32, [0, 1, 2, 3], [28, 29, 30, 31]),
    "L33-eyes2+2": (33, [32, 4], [0, 16]),
}
ODD_COUNTS = (21, 23, 30, 33, 45, 68)          # candidates for a level-0 unit count that is no multiple of four (tests/landmark_count_cases.py)
EXTRA_H = (27, 28, 41, 42, 43)                 # either side of both ends of the pair loop's eligible range at level 0

# The packed mode's feature rows were never the oracle's bits (the separable column sums of its mode); this is the bound
# tests/test_gpu_parity.py::check_features holds them to, written once for the pixel kernel's tests.
PACKED_MAX_ABS = 1e-6
PACKED_REL_L2 = 5e-7


# ---------------------------------------------------------------------------------------------- input builders
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(n, seed, h=256, w=256):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w)).astype(np.uint8)


def units_per_face(level, L):
    p = SHIPPED[level]
    plan = hog_plan(p.num_cells, p.cell_size, p.num_bins, L)
    return plan["n_main"] * plan["P"] + plan["Pt"], plan


def odd_units_count():
    return next(L for L in ODD_COUNTS if units_per_face(0, L)[0] % 4 != 0)


def face(L, re, le, h, centre, seed, level=0, spread=60.0):
    """One row of 2L landmarks scattered around `centre`, the eyes on a tilted line, scaled about the centre so that the half-width
    rel * IED / 2 of `level` is h (the middle of its rounding interval)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.4, 0.4)
    xs, ys = rng.uniform(-spread, spread, L), rng.uniform(-spread, spread, L)
    for idx, sign in ((re, +1.0), (le, -1.0)):
        for i in idx:
            xs[i] = sign * 30.0 * np.cos(ang) + rng.uniform(-3, 3)
            ys[i] = sign * 30.0 * np.sin(ang) + rng.uniform(-3, 3)
    row = np.concatenate([xs, ys])
    k = (2.0 * h / RELS[level]) / orc.get_ied(row.astype(np.float32), re, le)
    row = np.concatenate([centre[0] + xs * k, centre[1] + ys * k]).astype(np.float32)
    assert int(np.floor(RELS[level] * orc.get_ied(row, re, le) / 2.0 + 0.5)) == h
    return row


def edge_rows(L, re, le, seed):
    """Seven rows of 2L landmarks: eye centres 20 .. 150 px apart on a tilted line, the rest scattered; then, row by row: landmarks on
    x.5 (cvRound ties), negative coordinates, patches off every border, small and large faces."""
    rng = np.random.default_rng(seed)
    rows = []
    for kind in range(7):
        ied = (66.0, 58.0, 47.0, 83.0, 20.0, 150.0, 71.0)[kind]
        ang = rng.uniform(-0.5, 0.5)
        cx, cy = ((128, 128), (128, 128), (20, 15), (236, 240), (128, 128), (128, 128), (250, 8))[kind]
        xs = cx + rng.uniform(-70, 70, L)
        ys = cy + rng.uniform(-70, 70, L)
        for idx, sign in ((re, +1.0), (le, -1.0)):
            for i in idx:
                xs[i] = cx + sign * 0.5 * ied * np.cos(ang) + rng.uniform(-3, 3)
                ys[i] = cy + sign * 0.5 * ied * np.sin(ang) + rng.uniform(-3, 3)
        if kind == 1:                                        # cvRound ties: every coordinate on x.5 (even and odd integer parts)
            xs, ys = np.floor(xs) + 0.5, np.floor(ys) + 0.5
        if kind == 2:                                        # negative coordinates, patches off the left and the top border
            xs[: (L + 1) // 2] -= 60.0
            ys[L // 2:] -= 45.0
            xs[0] = -0.5
        if kind == 3:                                        # off the right and the bottom border, one patch wholly outside
            xs[L - 1], ys[L - 1] = 700.0, 650.0
        rows.append(np.concatenate([xs, ys]).astype(np.float32))
    return np.stack(rows)


def oracle_indices(x, L, re, le, rel):
    out = np.zeros((x.shape[0], 1 + 2 * L), np.int32)
    for n in range(x.shape[0]):
        v = float(np.float32(rel)) * orc.get_ied(x[n], re, le) / 2.0
        out[n, 0] = int(np.floor(v + 0.5))                   # C's round() of a value >= 0
        out[n, 1:] = [orc.cv_round(c) for c in x[n]]
    return out


def tie_sweep_rows(rel, ks):
    """Rows of L = 5 landmarks, right eye = landmark 0 at (d, 128), left eye = landmark 1 at (0, 128): the float difference of the
    eye centres is d itself.  d runs over the float32 neighbours of the values that put t = rel / 2 * d on each target."""
    f32 = np.float32
    half = f32(f32(rel) * f32(0.5))
    rows, ds = [], []
    for k in ks:
        for target in (k + 0.5, k + 0.5 - 2.0 ** -10, k + 0.5 + 2.0 ** -10):
            d0 = f32(target / float(half))
            b0 = int(np.array(d0, f32).view(np.int32))
            for step in range(-3, 4):
                ds.append(np.array(b0 + step, np.int32).view(f32))
    ds = np.array(ds, f32)
    for d in ds:
        xs = np.array([d, 0.0, 100.0, 128.25, 160.5], f32)
        ys = np.array([128.0, 128.0, 90.0, 128.5, 170.0], f32)
        rows.append(np.concatenate([xs, ys]))
    t = (half * ds).astype(f32)
    return np.stack(rows).astype(f32), ds, t


def smooth_faces(n=192):
    images, boxes, gt = synth.make_faces(n, seed=2024)
    _, x0, _ = synth.make_samples(boxes, gt, IDS22, n_perturb=0, seed=2025)
    return images, x0


def _scaled(x0, s, rel, h, dx=0.0, dy=0.0):
    """The landmarks of face s scaled about their centroid so that round(rel * ied / 2) = h, the centroid at (128 + dx, 128 + dy)."""
    xs, ys = x0[s, :L22].astype(np.float64), x0[s, L22:].astype(np.float64)
    k = (2.0 * h / rel) / orc.get_ied(x0[s], RE22, LE22)
    return np.concatenate([128.0 + dx + (xs - xs.mean()) * k, 128.0 + dy + (ys - ys.mean()) * k]).astype(np.float32)


def scaled_rows(x0, level):
    """One row per half-width h = 1 .. S of the level, then rows hanging off each image border and one wholly outside, at half-widths
    around 2h = S."""
    rel, S = float(np.float32(SHIPPED[level].relative_patch_size)), SIZES[level]
    rows, hs = [], []
    for h in range(1, S + 1):
        rows.append(_scaled(x0, h % x0.shape[0], rel, h)); hs.append(h)
    for h in sorted({1, 3, (S - 1) // 2, S // 2, (S + 1) // 2, S // 2 + 1, S - 1, S}):
        for dx, dy in ((-126.0, 0.0), (126.0, 0.0), (0.0, -126.0), (0.0, 126.0), (-125.0, 127.0), (-700.0, -700.0)):
            rows.append(_scaled(x0, (7 * h) % x0.shape[0], rel, h, dx, dy)); hs.append(h)
    return np.stack(rows), np.array(hs)


def pair_sweep_rows(x0):
    """scaled_rows of level 0 (h = 1 .. 55, rows hanging off each border and wholly outside), then the half-widths either side of
    both ends of the pair loop's eligible range once more on another face, inside the image and hanging off each border."""
    x, hs = scaled_rows(x0, 0)
    rel = float(np.float32(SHIPPED[0].relative_patch_size))
    rows, more = [x], []
    for h in EXTRA_H:
        for s, (dx, dy) in enumerate(((0.0, 0.0), (3.0, -5.0), (-126.0, 0.0), (126.0, 0.0), (0.0, -126.0), (0.0, 126.0), (-125.0, 127.0))):
            rows.append(_scaled(x0, (11 * h + s) % x0.shape[0], rel, h, dx, dy)[None])
            more.append(h)
    return np.concatenate(rows), np.concatenate([hs, np.array(more)])


# ---------------------------------------------------------------------------------------------- oracle side
def oracle(images, x, re, le, levels=range(4)):
    return {lv: orc.hog_features_batch(images, None, x, re, le, O_SHIPPED[lv], want_idx=True) for lv in levels}


def oracle_per_row(row_images, x, re, le, level):
    """(feature rows, patch indices) of one level, `row_images[i]` the image of row i: the images may differ in size."""
    wants = [orc.hog_features_batch(np.ascontiguousarray(im)[None], None, x[i:i + 1], re, le, O_SHIPPED[level], want_idx=True)
             for i, im in enumerate(row_images)]
    return np.concatenate([w[0] for w in wants]), np.concatenate([w[1] for w in wants])


# ---------------------------------------------------------------------------------------------- GPU side
def cells_features(ctx, x, level):
    """Feature rows as the descriptor kernel's store form makes them of the raw cells (the caller sets option hog_split_store)."""
    ctx.set_x(x)
    got = ctx.hog_features(level, fetch=True)
    return got, ctx.patch_indices()


def check_cells(got, idx, want, widx, what):
    diff = float(np.abs(got - want).max())
    rel = float(np.linalg.norm((got - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
    print("%s: %d rows, h %d .. %d, features through the raw cells against the oracle max abs %.3g rel L2 %.3g"
          % (what, got.shape[0], idx[:, 0].min(), idx[:, 0].max(), diff, rel))
    assert np.array_equal(idx, widx), what                    # the integer patch decisions
    assert diff <= PACKED_MAX_ABS and rel <= PACKED_REL_L2, what


def detect_equals_stepped_levels(ctx, x, L, seed):
    """Random regressors of scale 1e-3, option hog_split_store off: a four-level detect_batch is, bit for bit, the same four levels
    stepped one at a time.  Both sides run the same kernels: this pins the launch sequence.  Returns the landmarks."""
    rng = np.random.default_rng(seed)
    ctx.set_option("hog_split_store", 0)
    for lv in range(4):
        ctx.set_regressor(lv, (rng.standard_normal((ctx.feature_dim(lv), 2 * L)) * 1e-3).astype(np.float32))
    ctx.set_x(x)
    final = ctx.detect_batch()
    ctx.set_x(x)
    for lv in range(4):
        ctx.detect_level(lv)
    assert np.isfinite(final).all() and not np.array_equal(final, x)
    assert np.array_equal(bits(final), bits(ctx.get_x()))
    return final


@pytest.fixture
def options(gpu_ctx):
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.set_sample_image_index(None)
    yield gpu_ctx.set_option
    gpu_ctx.set_option("hog_two_load", 0)
    gpu_ctx.set_option("hog_split_store", 0)
    gpu_ctx.set_sample_image_index(None)
