"""The band folds of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_fold_overlap.txt).  The last
two bands of a pass are folded together behind the row loop, in one set of products (the pair fold): band C - 2 waits in its slot
while the rows of band C - 1 add zero to it.  Built for the same record and not in the tree
(scripts/experiments/hog_fold_overlap_items.patch): a fold cut into a take at the band boundary and a finish under the rows that
follow, a lane's cells address as a word of the plan, and the clamped horizontal taps from a second table; the shapes below were
chosen for them as well.  The record's mutants (the plan word of lane `lane ^ 1`; the closing pair fold storing a lane's four bins in the
other half of its cell) fail every comparison with the oracle here.

Nothing here may move a bit, so everything is checked against the CPU oracle inside the standing bounds of the packed mode
(tests/test_gpu_parity.py::check_features: <= 1e-6 absolute, relative L2 <= 5e-7) on NOISE images, where every bin row and every band
of a patch is populated and one cell stored to another cell's place changes features; the integer patch decisions
(sdm_get_patch_indices) must be the oracle's.  The raw cells are read as the feature rows the descriptor kernel's store form makes
of them (option hog_split_store), as in tests/test_gpu_fold_cost.py.

Shapes, small on purpose.  L = 22, three faces with level-0 half-widths 30, 45 and 36: the pair loop and the two-load loop in
neighbouring workgroups; the same faces under option hog_two_load (the third loop of every instance) must give the same bits, and
so must each face alone and the three in reverse order.  One face whose LEVEL-1 half-width is 28: the two-load loop inside an
instance that carries the one-load loop.  The plans hold a patch cut by a pass boundary (a second part of cells), a tail group and
a level-0 pass whose last eight lanes hold no column -- asserted from the plans.  L = 5 with one face: a last workgroup partly past
the last unit.  One landmark count whose level-0 units per face are no multiple of four.  Patches partly and wholly off the canvas:
all-zero operands.  One ragged set of frames with differing strides.  An empty patch is still reported.  A four-level detect equals
the same levels stepped one at a time."""
import numpy as np
import pytest

import landmark_count_cases as lcc
from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, SdmError, ibug
from superviseddescent_amd._lib import SDM_HOG_COLUMNS
from superviseddescent_amd.engine import hog_plan

SHIPPED = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
O_SHIPPED = [orc.HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
RELS = [float(np.float32(p.relative_patch_size)) for p in SHIPPED]
L22 = len(ibug.RCR22_IDS)
RE22, LE22 = ibug.eye_indices(ibug.RCR22_IDS)
ODD_COUNTS = (21, 23, 30, 33, 45, 68)          # candidates for a level-0 unit count that is no multiple of four


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 256, 256)).astype(np.uint8)


def _units_per_face(level, L):
    p = SHIPPED[level]
    plan = hog_plan(p.num_cells, p.cell_size, p.num_bins, L)
    return plan["n_main"] * plan["P"] + plan["Pt"], plan


def _face(L, re, le, h, centre, seed, level=0, spread=60.0):
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
    images = _noise(3, seed=511)
    x = np.stack([_face(L22, RE22, LE22, h0, c, seed=520 + i) for i, (h0, c) in enumerate(((30, (120, 131)), (45, (133, 122)), (36, (126, 128))))])
    return dict(images=images, x=x, want=_oracle(images, x, RE22, LE22))


def test_the_plans_are_the_ones_intended(built):
    """A patch cut by a pass boundary (a second part of cells), a tail group, a level-0 pass whose last eight lanes hold no
    column, a last workgroup partly past the last unit at L = 5, and a landmark count whose level-0 units are no multiple of four."""
    for lv in range(3):
        plan = _units_per_face(lv, L22)[1]
        assert plan["Gt"] > 0 and plan["Pt"] > 0 and plan["cut"].any(), lv
    plan0 = _units_per_face(0, L22)[1]
    assert (((plan0["pass_info"][:, 3] >> 16) & 0xff) == 7).any()
    assert any(_units_per_face(lv, 5)[0] % 4 != 0 for lv in range(4))
    assert any(_units_per_face(0, L)[0] % 4 != 0 for L in ODD_COUNTS)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_cells_of_three_faces_against_the_oracle(gpu_ctx, options, three_faces, level):
    """All four shipped cell sizes (11 / 10 / 8 / 6), in the loop each face's half-width picks and under hog_two_load: the same bits;
    each face alone and the three in reverse order: the same bits."""
    x, images = three_faces["x"], three_faces["images"]
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(images)
    got, idx = _cells_features(gpu_ctx, x, level)
    want, widx = three_faces["want"][level]
    _check(got, idx, want, widx, "three faces, level %d" % level)
    if level == 0:
        table, info = gpu_ctx.debug_hog_pair_taps(0)
        assert info["pair_instance"] and widx[:, 0].tolist() == [30, 45, 36]
        assert [int(table[h, 0, 2]) for h in (30, 45, 36)] == [1, 0, 1]      # pair loop, two-load loop, pair loop
    options("hog_two_load", 1)
    two, idx2 = _cells_features(gpu_ctx, x, level)
    options("hog_two_load", 0)
    assert np.array_equal(idx2, widx) and np.array_equal(_bits(got), _bits(two))
    for n in range(3):
        gpu_ctx.upload_images(images[n:n + 1])
        one, idx1 = _cells_features(gpu_ctx, x[n:n + 1], level)
        assert np.array_equal(idx1, widx[n:n + 1]) and np.array_equal(_bits(one), _bits(got[n:n + 1])), n
    gpu_ctx.upload_images(images[::-1].copy())
    rev, _ = _cells_features(gpu_ctx, x[::-1].copy(), level)
    assert np.array_equal(_bits(rev), _bits(got[::-1]))


@pytest.mark.gpu
def test_two_load_loop_inside_a_row_carry_instance(gpu_ctx, options):
    """Level 1 (cell 10, an instance with the one-load loop) at half-width 28: the patch is reduced, the wave takes the two-load loop;
    beside a face at half-width 20, which takes the one-load loop."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    images = _noise(2, seed=531)
    x = np.stack([_face(L22, RE22, LE22, 28, (128, 126), seed=540, level=1), _face(L22, RE22, LE22, 20, (125, 130), seed=541, level=1)])
    gpu_ctx.upload_images(images)
    table, info = gpu_ctx.debug_hog_taps(1)
    assert info["one_load_instance"] and int(table[28, 0, 7]) == 0 and int(table[20, 0, 7]) == 1
    want, widx = _oracle(images, x, RE22, LE22, levels=[1])[1]
    assert widx[:, 0].tolist() == [28, 20]
    got, idx = _cells_features(gpu_ctx, x, 1)
    _check(got, idx, want, widx, "level 1, half-widths 28 and 20")
    options("hog_two_load", 1)
    two, _ = _cells_features(gpu_ctx, x, 1)
    options("hog_two_load", 0)
    assert np.array_equal(_bits(got), _bits(two))
    for n in range(2):
        gpu_ctx.upload_images(images[n:n + 1])
        one, _ = _cells_features(gpu_ctx, x[n:n + 1], 1)
        assert np.array_equal(_bits(one), _bits(got[n:n + 1])), n
    gpu_ctx.upload_images(images[::-1].copy())
    rev, _ = _cells_features(gpu_ctx, x[::-1].copy(), 1)
    assert np.array_equal(_bits(rev), _bits(got[::-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["L5", "odd"])
def test_partial_and_straddling_workgroups(gpu_ctx, options, which):
    """L = 5 with one face (a last workgroup partly past the last unit), and a landmark count whose level-0 units per face are no
    multiple of four with three faces (workgroups holding units of two faces)."""
    if which == "L5":
        L, n = 5, 1
    else:
        L, n = next(c for c in ODD_COUNTS if _units_per_face(0, c)[0] % 4 != 0), 3
    _, re, le = lcc.landmark_set(L)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    images = _noise(n, seed=551)
    x = np.stack([_face(L, re, le, h0, (128, 128), seed=560 + i) for i, h0 in enumerate((38, 26, 42)[:n])])
    gpu_ctx.upload_images(images)
    want = _oracle(images, x, re, le)
    for lv in range(4):
        got, idx = _cells_features(gpu_ctx, x, lv)
        _check(got, idx, *want[lv], "L = %d, %d faces, level %d" % (L, n, lv))


@pytest.mark.gpu
def test_patches_partly_and_wholly_off_the_canvas(gpu_ctx, options):
    """Zero column sums through every fold: faces at two corners of the image, landmarks far outside it."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    images = _noise(3, seed=571)
    x = np.stack([_face(L22, RE22, LE22, 33, (18, 12), seed=580), _face(L22, RE22, LE22, 29, (244, 250), seed=581),
                  _face(L22, RE22, LE22, 40, (128, 128), seed=582)])
    others = [i for i in range(L22) if i not in RE22 + LE22]
    x[2, others[0]], x[2, L22 + others[0]] = 700.0, 650.0            # wholly outside, below and to the right
    x[2, others[1]], x[2, L22 + others[1]] = -300.5, 128.0           # wholly outside, to the left
    x[2, others[2]], x[2, L22 + others[2]] = 128.0, -41.0            # the patch's last rows on the canvas
    gpu_ctx.upload_images(images)
    want = _oracle(images, x, RE22, LE22)
    for lv in range(4):
        got, idx = _cells_features(gpu_ctx, x, lv)
        _check(got, idx, *want[lv], "off the canvas, level %d" % lv)
    P = want[0][0].shape[1] // L22
    assert not _cells_features(gpu_ctx, x, 0)[0][2, others[0] * P:(others[0] + 1) * P].any()


@pytest.mark.gpu
def test_ragged_frames_with_differing_strides(gpu_ctx, options):
    """Frames of differing sizes and pitches, the samples in another order than the frames: the image borders stay per patch."""
    import torch
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    sizes = [(256, 256, 256), (200, 240, 320), (256, 130, 384), (131, 133, 192)]      # h, w, pitch
    rng = np.random.default_rng(591)
    host = [rng.integers(0, 256, (h, pitch)).astype(np.uint8) for h, _, pitch in sizes]
    keep = [torch.from_numpy(a).cuda() for a in host]
    gpu_ctx.set_frames_device([t[:, :w] for t, (_, w, _) in zip(keep, sizes)])
    order = np.array([3, 1, 0, 2], np.int32)
    gpu_ctx.set_sample_image_index(order)
    x = np.stack([_face(L22, RE22, LE22, h0, c, seed=600 + i, spread=40.0)
                  for i, (h0, c) in enumerate(((24, (60, 70)), (31, (130, 90)), (40, (128, 128)), (27, (70, 120))))])
    for lv in range(4):
        got, idx = _cells_features(gpu_ctx, x, lv)
        wants = [orc.hog_features_batch(np.ascontiguousarray(host[f][:, :sizes[f][1]])[None], None, x[i:i + 1], RE22, LE22, O_SHIPPED[lv], want_idx=True)
                 for i, f in enumerate(order)]
        _check(got, idx, np.concatenate([w[0] for w in wants]), np.concatenate([w[1] for w in wants]), "ragged, level %d" % lv)
    gpu_ctx.upload_images(_noise(1, seed=1))                 # (the frames go out of scope)


@pytest.mark.gpu
def test_empty_patch_is_still_reported(gpu_ctx, options):
    """A face of two pixels between two good ones: rel * IED / 2 < 1 / 2 at every level; then the same context goes on working."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(_noise(3, seed=611))
    good = np.stack([_face(L22, RE22, LE22, h0, (128, 128), seed=620 + i) for i, h0 in enumerate((30, 36, 41))])
    bad = good.copy()
    bad[1] = (128.0 + (bad[1] - 128.0) * np.float32(0.01)).astype(np.float32)
    assert all(r * orc.get_ied(bad[1], RE22, LE22) / 2.0 < 0.49 for r in RELS)

    def codes(x):
        out = []
        for lv in range(4):
            gpu_ctx.set_x(x)
            try:
                gpu_ctx.hog_features(lv, fetch=True)
                out.append(0)
            except SdmError as e:
                out.append(e.code)
        return out
    assert codes(bad) == [-4] * 4
    assert codes(good) == [0] * 4


@pytest.mark.gpu
def test_detect_equals_the_levels_stepped_one_at_a_time(gpu_ctx, options, three_faces):
    options("hog_split_store", 0)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"])
    rng = np.random.default_rng(7)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, (rng.standard_normal((gpu_ctx.feature_dim(lv), 2 * L22)) * 1e-3).astype(np.float32))
    gpu_ctx.set_x(three_faces["x"])
    whole = gpu_ctx.detect_batch()
    assert np.isfinite(whole).all() and not np.array_equal(whole, three_faces["x"])
    gpu_ctx.set_x(three_faces["x"])
    for lv in range(4):
        gpu_ctx.detect_level(lv)
    assert np.array_equal(_bits(whole), _bits(gpu_ctx.get_x()))
