"""The band folds of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_fold_cost.txt).  A fold fetches
each of its operands with an LDS exchange with zero, which reads the column sum AND clears it for the band after next (lanes 8 .. 15
of a one-band fold, which would repeat bin row 7, stay out of it), and splits it into two float16 pieces with a conversion toward zero
and one mixed-precision multiply-add per value (the same bits as a mask, a subtraction and a conversion while a column sum is zero
or a float16-normal number).  Built for the same record and not shipped (scripts/experiments/hog_fold_items.patch): ONE row table per
workgroup where the units of a face are a multiple of its four waves -- the shapes below were chosen for it as well, and its mutant
(the shared table also where a workgroup holds units of two faces) fails test_per_wave_tables_where_a_workgroup_straddles_faces.
The mutant of the shipped kernel (half of a fold's operands read without being cleared) fails every comparison with the oracle here.

Nothing in a fold may move a bit, so everything here is checked against the CPU oracle inside the standing bounds of the packed mode
(tests/test_gpu_parity.py::check_features: <= 1e-6 absolute, relative L2 <= 5e-7) on NOISE images, where every bin row and every band
of a patch is populated and one wrong table entry or one dropped piece product changes cells; the integer patch decisions
(sdm_get_patch_indices) must be the oracle's.  The raw cells are read as the feature rows the descriptor kernel's store form makes
of them (option hog_split_store), as in tests/test_gpu_pass_setup.py and tests/test_gpu_pair_carry.py.

Shapes, small on purpose.  L = 22, three faces: the level-0 plan has 20 units per face (no workgroup holds units of two faces), the
other levels 18 / 15 / 11 (workgroups straddle faces and the last one is partial); the plans of levels 0 - 2 have a tail group
(22 = 2 x 9 + 4 at level 0) and patches cut by a pass boundary (a second part of cells), and level 0 has passes whose last eight
lanes hold no column -- all asserted from the plans.  The three faces have level-0 half-widths 30, 45 and 36: neighbouring workgroups
differ in the row table's contents AND in the row loop they take (45 is outside the pair loop's range 27 .. 41), so a workgroup
reading a neighbour's table, or a wave another wave's, cannot pass; the same faces under option hog_two_load must give the same
bits, and so must each face alone and the three in reverse order.  One landmark count whose level-0 units per face are NOT a
multiple of four, with one face and with three (a last workgroup partly past the last unit).  One case has patches partly and wholly
off the canvas: all-zero column sums through the operand split."""
import numpy as np
import pytest

import landmark_count_cases as lcc
from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, ibug
from superviseddescent_amd._lib import SDM_HOG_COLUMNS
from superviseddescent_amd.engine import hog_plan

SHIPPED = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
O_SHIPPED = [orc.HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
RELS = [float(np.float32(p.relative_patch_size)) for p in SHIPPED]
L22 = len(ibug.RCR22_IDS)
RE22, LE22 = ibug.eye_indices(ibug.RCR22_IDS)
FALLBACK_COUNTS = (21, 23, 30, 33, 45, 68, 5)          # candidates for a level-0 unit count that is no multiple of four (tests/landmark_count_cases.py)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 256, 256)).astype(np.uint8)


def _units_per_face(level, L):
    p = SHIPPED[level]
    plan = hog_plan(p.num_cells, p.cell_size, p.num_bins, L)
    return plan["n_main"] * plan["P"] + plan["Pt"], plan


def _face(L, re, le, h0, centre, seed, spread=60.0):
    """One row of 2L landmarks scattered around `centre`, the eyes on a tilted line, scaled about the centre so that the level-0
    half-width rel * IED / 2 is h0 (the middle of its rounding interval)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.4, 0.4)
    xs, ys = rng.uniform(-spread, spread, L), rng.uniform(-spread, spread, L)
    for idx, sign in ((re, +1.0), (le, -1.0)):
        for i in idx:
            xs[i] = sign * 30.0 * np.cos(ang) + rng.uniform(-3, 3)
            ys[i] = sign * 30.0 * np.sin(ang) + rng.uniform(-3, 3)
    row = np.concatenate([xs, ys])
    k = (2.0 * h0 / RELS[0]) / orc.get_ied(row.astype(np.float32), re, le)
    row = np.concatenate([centre[0] + xs * k, centre[1] + ys * k]).astype(np.float32)
    assert int(np.floor(RELS[0] * orc.get_ied(row, re, le) / 2.0 + 0.5)) == h0
    return row


def _oracle(images, x, re, le, levels=range(4)):
    return {lv: orc.hog_features_batch(images, None, x, re, le, O_SHIPPED[lv], want_idx=True) for lv in levels}


def _cells_features(gpu_ctx, x, level):
    gpu_ctx.set_x(x)
    got = gpu_ctx.hog_features(level, fetch=True)
    return got, gpu_ctx.patch_indices()


def _check(got, idx, want, widx, what):
    diff = float(np.abs(got - want).max())
    rel = float(np.linalg.norm((got - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
    print("%s: %d rows, h %d .. %d, features through the raw cells against the oracle max abs %.3g rel L2 %.3g"
          % (what, got.shape[0], idx[:, 0].min(), idx[:, 0].max(), diff, rel))
    assert np.array_equal(idx, widx), what                    # the integer patch decisions
    assert diff <= 1e-6 and rel <= 5e-7, what                 # tests/test_gpu_parity.py::check_features, packed mode


@pytest.fixture
def options(gpu_ctx):
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.set_sample_image_index(None)
    gpu_ctx.set_option("hog_split_store", 1)
    yield gpu_ctx.set_option
    gpu_ctx.set_option("hog_two_load", 0)
    gpu_ctx.set_option("hog_split_store", 0)
    gpu_ctx.set_sample_image_index(None)


@pytest.fixture(scope="module")
def three_faces():
    """Three faces of 22 landmarks with level-0 half-widths 30, 45 and 36 on noise, and the oracle of the four levels, computed once."""
    images = _noise(3, seed=411)
    x = np.stack([_face(L22, RE22, LE22, h0, c, seed=420 + i) for i, (h0, c) in enumerate(((30, (120, 131)), (45, (133, 122)), (36, (126, 128))))])
    return dict(images=images, x=x, want=_oracle(images, x, RE22, LE22))


def test_the_plans_are_the_ones_intended(built):
    """What the docstring says of the plans: which levels keep a workgroup inside one face at L = 22, the tail group, the cut patches, the passes of
    level 0 whose last eight lanes are empty, and a landmark count whose level-0 units per face are no multiple of four."""
    gpfs = []
    for lv in range(4):
        gpf, plan = _units_per_face(lv, L22)
        gpfs.append(gpf)
        assert lv == 3 or (plan["Gt"] > 0 and plan["Pt"] > 0 and plan["cut"].any()), lv      # (level 3: eleven groups of two whole patches)
    assert gpfs == [20, 18, 15, 11]
    assert gpfs[0] % 4 == 0 and all((3 * g) % 4 != 0 and g % 4 != 0 for g in gpfs[1:])      # straddling and partial workgroups at levels 1 - 3
    plan0 = _units_per_face(0, L22)[1]
    assert (plan0["G"], plan0["n_main"], plan0["Gt"]) == (9, 2, 4)
    assert (((plan0["pass_info"][:, 3] >> 16) & 0xff) == 7).any()
    assert any(_units_per_face(0, L)[0] % 4 != 0 for L in FALLBACK_COUNTS)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_cells_of_three_faces_against_the_oracle(gpu_ctx, options, three_faces, level):
    """All four shipped cell sizes (11 / 10 / 8 / 6); twice: the same bits."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"])
    got, idx = _cells_features(gpu_ctx, three_faces["x"], level)
    _check(got, idx, *three_faces["want"][level], "three faces, level %d" % level)
    again, _ = _cells_features(gpu_ctx, three_faces["x"], level)
    assert np.array_equal(_bits(got), _bits(again))


@pytest.mark.gpu
def test_neighbouring_workgroups_with_differing_row_tables(gpu_ctx, options, three_faces):
    """Level 0, a workgroup's four waves are units of one face: neighbouring workgroups differ in half-width and in the row loop they
    take."""
    x, (want, widx) = three_faces["x"], three_faces["want"][0]
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"])
    table, info = gpu_ctx.debug_hog_pair_taps(0)
    assert info["pair_instance"] and gpu_ctx.debug_hog_taps(0)[1]["cells_launch"]
    hs = widx[:, 0].tolist()
    assert hs == [30, 45, 36] and [int(table[h, 0, 2]) for h in hs] == [1, 0, 1]      # pair loop, two-load loop, pair loop
    got, idx = _cells_features(gpu_ctx, x, 0)
    _check(got, idx, want, widx, "differing neighbours")
    options("hog_two_load", 1)
    two, idx2 = _cells_features(gpu_ctx, x, 0)
    assert np.array_equal(idx2, widx) and np.array_equal(_bits(got), _bits(two))
    options("hog_two_load", 0)
    # each face alone (five whole workgroups), and in the other order: a face's cells do not depend on its neighbours
    for n in range(3):
        gpu_ctx.upload_images(three_faces["images"][n:n + 1])
        one, idx1 = _cells_features(gpu_ctx, x[n:n + 1], 0)
        assert np.array_equal(idx1, widx[n:n + 1]) and np.array_equal(_bits(one), _bits(got[n:n + 1])), n
    gpu_ctx.upload_images(three_faces["images"][::-1].copy())
    rev, _ = _cells_features(gpu_ctx, x[::-1].copy(), 0)
    assert np.array_equal(_bits(rev), _bits(got[::-1]))


@pytest.mark.gpu
def test_per_wave_tables_where_a_workgroup_straddles_faces(gpu_ctx, options):
    """A landmark count whose level-0 units per face are no multiple of four: the waves of a workgroup need tables of their own; one
    face and three (straddling workgroups, a last workgroup partly past the last unit)."""
    L = next(n for n in FALLBACK_COUNTS if _units_per_face(0, n)[0] % 4 != 0)
    gpf = _units_per_face(0, L)[0]
    assert gpf % 4 != 0 and (3 * gpf) % 4 != 0
    _, re, le = lcc.landmark_set(L)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    images = _noise(3, seed=431)
    x = np.stack([_face(L, re, le, h0, (128, 128), seed=440 + i) for i, h0 in enumerate((26, 38, 42))])
    want, widx = _oracle(images, x, re, le, levels=[0])[0]
    for n, pick in ((1, slice(1, 2)), (3, slice(0, 3))):
        gpu_ctx.upload_images(images[pick])
        got, idx = _cells_features(gpu_ctx, x[pick], 0)
        _check(got, idx, want[pick], widx[pick], "L = %d (%d units per face), %d faces" % (L, gpf, n))
        options("hog_two_load", 1)
        two, _ = _cells_features(gpu_ctx, x[pick], 0)
        options("hog_two_load", 0)
        assert np.array_equal(_bits(got), _bits(two))


@pytest.mark.gpu
def test_one_face_at_every_level(gpu_ctx, options, three_faces):
    """N = 1: five whole workgroups at level 0, a partial last workgroup at the others."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"][1:2])
    for lv in range(4):
        got, idx = _cells_features(gpu_ctx, three_faces["x"][1:2], lv)
        want, widx = three_faces["want"][lv]
        _check(got, idx, want[1:2], widx[1:2], "one face, level %d" % lv)


@pytest.mark.gpu
def test_patches_partly_and_wholly_off_the_canvas(gpu_ctx, options):
    """Zero column sums through the split: faces at two corners of the image, landmarks far outside it."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    images = _noise(3, seed=451)
    x = np.stack([_face(L22, RE22, LE22, 33, (18, 12), seed=460), _face(L22, RE22, LE22, 29, (244, 250), seed=461),
                  _face(L22, RE22, LE22, 40, (128, 128), seed=462)])
    others = [i for i in range(L22) if i not in RE22 + LE22]
    x[2, others[0]], x[2, L22 + others[0]] = 700.0, 650.0            # wholly outside, below and to the right
    x[2, others[1]], x[2, L22 + others[1]] = -300.5, 128.0           # wholly outside, to the left
    x[2, others[2]], x[2, L22 + others[2]] = 128.0, -41.0            # the patch's last rows on the canvas
    gpu_ctx.upload_images(images)
    want = _oracle(images, x, RE22, LE22)
    for lv in range(4):
        got, idx = _cells_features(gpu_ctx, x, lv)
        _check(got, idx, *want[lv], "off the canvas, level %d" % lv)
    # the patches wholly outside are all-zero cells: the descriptor of zero cells
    P = want[0][0].shape[1] // L22
    assert not _cells_features(gpu_ctx, x, 0)[0][2, others[0] * P:(others[0] + 1) * P].any()


@pytest.mark.gpu
def test_detect_twice_is_the_same_bits(gpu_ctx, options, three_faces):
    options("hog_split_store", 0)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"])
    rng = np.random.default_rng(7)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, (rng.standard_normal((gpu_ctx.feature_dim(lv), 2 * L22)) * 1e-3).astype(np.float32))
    runs = []
    for _ in range(2):
        gpu_ctx.set_x(three_faces["x"])
        runs.append(gpu_ctx.detect_batch())
    assert np.isfinite(runs[0]).all() and not np.array_equal(runs[0], three_faces["x"])
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    # and the same four levels stepped one at a time
    gpu_ctx.set_x(three_faces["x"])
    for lv in range(4):
        gpu_ctx.detect_level(lv)
    assert np.array_equal(_bits(runs[0]), _bits(gpu_ctx.get_x()))
