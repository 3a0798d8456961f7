"""The band folds of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_fold_cost.txt and
profiles/hog_fold_overlap.txt): the tests of BOTH records, the operand exchange and the closing pair fold.

The operand exchange (hog_fold_cost).  A fold fetches each of its operands with an LDS exchange with zero, which reads the column sum
AND clears it for the band after next (lanes 8 .. 15 of a one-band fold, which would repeat bin row 7, stay out of it), and splits it
into two float16 pieces with a conversion toward zero and one mixed-precision multiply-add per value (the same bits as a mask, a
subtraction and a conversion while a column sum is zero or a float16-normal number).  Built for the same record and not shipped
(scripts/experiments/hog_fold_items.patch): ONE row table per workgroup where the units of a face are a multiple of its four waves --
the shapes below were chosen for it as well, and its mutant (the shared table also where a workgroup holds units of two faces) fails
the level-0 case of test_partial_and_straddling_workgroups.  The mutant of the shipped kernel (half of a fold's operands read without
being cleared) fails every comparison with the oracle here.

The closing pair fold (hog_fold_overlap).  The last two bands of a pass are folded together behind the row loop, in one set of
products: band C - 2 waits in its slot while the rows of band C - 1 add zero to it.  Built for the same record and not in the tree
(scripts/experiments/hog_fold_overlap_items.patch): a fold cut into a take at the band boundary and a finish under the rows that
follow, a lane's cells address as a word of the plan, and the clamped horizontal taps from a second table; the shapes below were
chosen for them as well.  The record's mutants (the plan word of lane `lane ^ 1`; the closing pair fold storing a lane's four bins in
the other half of its cell) fail every comparison with the oracle here.

Nothing in a fold may move a bit, so everything is checked against the CPU oracle inside the standing bounds of the packed mode
(pixel_kernel_cases.PACKED_MAX_ABS, PACKED_REL_L2) on NOISE images, where every bin row and every band of a patch is populated and one
wrong table entry, one dropped piece product or one cell stored to another cell's place changes features; the integer patch decisions
(sdm_get_patch_indices) must be the oracle's.  The raw cells are read as the feature rows the descriptor kernel's store form makes
of them (option hog_split_store), as in tests/test_gpu_pass_setup.py and tests/test_gpu_pair_carry.py.

Shapes, small on purpose.  L = 22, three faces: the level-0 plan has 20 units per face (no workgroup holds units of two faces), the
other levels 18 / 15 / 11 (workgroups straddle faces and the last one is partial); the plans of levels 0 - 2 have a tail group
(22 = 2 x 9 + 4 at level 0) and patches cut by a pass boundary (a second part of cells), and level 0 has passes whose last eight
lanes hold no column -- all asserted from the plans.  The three faces have level-0 half-widths 30, 45 and 36: neighbouring workgroups
differ in the row table's contents AND in the row loop they take (45 is outside the pair loop's range 27 .. 41), so a workgroup
reading a neighbour's table, or a wave another wave's, cannot pass; the same faces under option hog_two_load (the third loop of every
instance) must give the same bits, and so must each face alone (five whole workgroups at level 0, a partial last workgroup at the
others) and the three in reverse order.  One face whose LEVEL-1 half-width is 28: the two-load loop inside an instance that carries
the one-load loop.  L = 5 with one face: a last workgroup partly past the last unit.  One landmark count whose level-0 units per face
are NOT a multiple of four, with one face and with three (straddling workgroups, a last workgroup partly past the last unit).  One
case has patches partly and wholly off the canvas: all-zero column sums through the operand split and every fold.  A four-level
detect, twice, equals the same levels stepped one at a time.  (Ragged frames and the empty patch: tests/test_gpu_pass_setup.py.)"""
import numpy as np
import pytest

import landmark_count_cases as lcc
from pixel_kernel_cases import (EYE_CASES, L22, LE22, ODD_COUNTS, RE22, SHIPPED, bits, cells_features, check_cells,
                                detect_equals_stepped_levels, face, noise, odd_units_count, options, oracle, units_per_face)  # noqa: F401


@pytest.fixture(scope="module")
def three_faces():
    """Three faces of 22 landmarks with level-0 half-widths 30, 45 and 36 on noise, and the oracle of the four levels, computed once."""
    images = noise(3, seed=511)
    x = np.stack([face(L22, RE22, LE22, h0, c, seed=520 + i) for i, (h0, c) in enumerate(((30, (120, 131)), (45, (133, 122)), (36, (126, 128))))])
    return dict(images=images, x=x, want=oracle(images, x, RE22, LE22))


def test_the_plans_are_the_ones_intended(built):
    """What the docstrings say of the plans: which levels keep a workgroup inside one face at L = 22, the tail group, the cut patches,
    the passes of level 0 whose last eight lanes are empty, a last workgroup partly past the last unit at L = 5, a landmark count whose
    level-0 units per face are no multiple of four, and (tests/test_gpu_pass_setup.py) 1, 3 and 7 faces against the units per face of
    its six cases: somewhere a workgroup of four waves holds units of two faces, and somewhere the last workgroup is partial."""
    gpfs = []
    for lv in range(4):
        gpf, plan = units_per_face(lv, L22)
        gpfs.append(gpf)
        assert lv == 3 or (plan["Gt"] > 0 and plan["Pt"] > 0 and plan["cut"].any()), lv      # (level 3: eleven groups of two whole patches)
    assert gpfs == [20, 18, 15, 11]
    assert gpfs[0] % 4 == 0 and all((3 * g) % 4 != 0 and g % 4 != 0 for g in gpfs[1:])      # straddling and partial workgroups at levels 1 - 3
    plan0 = units_per_face(0, L22)[1]
    assert (plan0["G"], plan0["n_main"], plan0["Gt"]) == (9, 2, 4)
    assert (((plan0["pass_info"][:, 3] >> 16) & 0xff) == 7).any()
    assert any(units_per_face(lv, 5)[0] % 4 != 0 for lv in range(4))
    assert any(units_per_face(0, L)[0] % 4 != 0 for L in ODD_COUNTS)
    gpf = units_per_face(0, odd_units_count())[0]
    assert gpf % 4 != 0 and (3 * gpf) % 4 != 0
    straddle = partial = 0
    for L, _, _ in EYE_CASES.values():
        for lv in range(4):
            gpf = units_per_face(lv, L)[0]
            for n in (3, 7):
                straddle += gpf % 4 != 0
                partial += (n * gpf) % 4 != 0
            partial += gpf % 4 != 0                           # one face
    assert straddle >= 8 and partial >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_cells_of_three_faces_against_the_oracle(gpu_ctx, options, three_faces, level):
    """All four shipped cell sizes (11 / 10 / 8 / 6), in the loop each face's half-width picks; twice, under hog_two_load, each face
    alone (N = 1: a face's cells do not depend on its neighbours) and the three in reverse order: the same bits.  At level 0 a
    workgroup's four waves are units of one face: neighbouring workgroups differ in half-width and in the row loop they take."""
    x, images = three_faces["x"], three_faces["images"]
    want, widx = three_faces["want"][level]
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(images)
    got, idx = cells_features(gpu_ctx, x, level)
    check_cells(got, idx, want, widx, "three faces, level %d" % level)
    if level == 0:
        table, info = gpu_ctx.debug_hog_pair_taps(0)
        assert info["pair_instance"] and gpu_ctx.debug_hog_taps(0)[1]["cells_launch"]
        hs = widx[:, 0].tolist()
        assert hs == [30, 45, 36] and [int(table[h, 0, 2]) for h in hs] == [1, 0, 1]      # pair loop, two-load loop, pair loop
    again, _ = cells_features(gpu_ctx, x, level)
    assert np.array_equal(bits(got), bits(again))
    options("hog_two_load", 1)
    two, idx2 = cells_features(gpu_ctx, x, level)
    options("hog_two_load", 0)
    assert np.array_equal(idx2, widx) and np.array_equal(bits(got), bits(two))
    for n in range(3):
        gpu_ctx.upload_images(images[n:n + 1])
        one, idx1 = cells_features(gpu_ctx, x[n:n + 1], level)
        check_cells(one, idx1, want[n:n + 1], widx[n:n + 1], "face %d alone, level %d" % (n, level))
        assert np.array_equal(bits(one), bits(got[n:n + 1])), n
    gpu_ctx.upload_images(images[::-1].copy())
    rev, _ = cells_features(gpu_ctx, x[::-1].copy(), level)
    assert np.array_equal(bits(rev), bits(got[::-1]))


@pytest.mark.gpu
def test_two_load_loop_inside_a_row_carry_instance(gpu_ctx, options):
    """Level 1 (cell 10, an instance with the one-load loop) at half-width 28: the patch is reduced, the wave takes the two-load loop;
    beside a face at half-width 20, which takes the one-load loop."""
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    images = noise(2, seed=531)
    x = np.stack([face(L22, RE22, LE22, 28, (128, 126), seed=540, level=1), face(L22, RE22, LE22, 20, (125, 130), seed=541, level=1)])
    gpu_ctx.upload_images(images)
    table, info = gpu_ctx.debug_hog_taps(1)
    assert info["one_load_instance"] and int(table[28, 0, 7]) == 0 and int(table[20, 0, 7]) == 1
    want, widx = oracle(images, x, RE22, LE22, levels=[1])[1]
    assert widx[:, 0].tolist() == [28, 20]
    got, idx = cells_features(gpu_ctx, x, 1)
    check_cells(got, idx, want, widx, "level 1, half-widths 28 and 20")
    options("hog_two_load", 1)
    two, _ = cells_features(gpu_ctx, x, 1)
    options("hog_two_load", 0)
    assert np.array_equal(bits(got), bits(two))
    for n in range(2):
        gpu_ctx.upload_images(images[n:n + 1])
        one, _ = cells_features(gpu_ctx, x[n:n + 1], 1)
        assert np.array_equal(bits(one), bits(got[n:n + 1])), n
    gpu_ctx.upload_images(images[::-1].copy())
    rev, _ = cells_features(gpu_ctx, x[::-1].copy(), 1)
    assert np.array_equal(bits(rev), bits(got[::-1]))


# (landmark count or "odd" = odd_units_count(), level-0 half-widths, face counts as slices of them, levels, noise seed, first face seed)
@pytest.mark.gpu
@pytest.mark.parametrize("L, hs, picks, levels, seeds", [
    # the waves of a workgroup need row tables of their own: one face and three at level 0
    pytest.param("odd", (26, 38, 42), (slice(1, 2), slice(0, 3)), (0,), (431, 440), id="odd-1and3faces-level0"),
    # a last workgroup partly past the last unit: one face
    pytest.param(5, (38,), (slice(0, 1),), (0, 1, 2, 3), (551, 560), id="L5"),
    # workgroups holding units of two faces, at every cell size: three faces
    pytest.param("odd", (38, 26, 42), (slice(0, 3),), (0, 1, 2, 3), (551, 560), id="odd"),
])
def test_partial_and_straddling_workgroups(gpu_ctx, options, L, hs, picks, levels, seeds):
    """Units per face that are no multiple of a workgroup's four waves; with hog_two_load: the same bits."""
    if L == "odd":
        L = odd_units_count()
    options("hog_split_store", 1)
    _, re, le = lcc.landmark_set(L)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    images = noise(len(hs), seed=seeds[0])
    x = np.stack([face(L, re, le, h0, (128, 128), seed=seeds[1] + i) for i, h0 in enumerate(hs)])
    wants = oracle(images, x, re, le, levels=levels)
    for pick in picks:
        gpu_ctx.upload_images(images[pick])
        for lv in levels:
            want, widx = wants[lv]
            got, idx = cells_features(gpu_ctx, x[pick], lv)
            check_cells(got, idx, want[pick], widx[pick], "L = %d (%d units per face), %d faces, level %d" % (L, units_per_face(lv, L)[0], x[pick].shape[0], lv))
            options("hog_two_load", 1)
            two, _ = cells_features(gpu_ctx, x[pick], lv)
            options("hog_two_load", 0)
            assert np.array_equal(bits(got), bits(two))


@pytest.mark.gpu
def test_patches_partly_and_wholly_off_the_canvas(gpu_ctx, options):
    """Zero column sums through the split and every fold: faces at two corners of the image, landmarks far outside it."""
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    images = noise(3, seed=571)
    x = np.stack([face(L22, RE22, LE22, 33, (18, 12), seed=580), face(L22, RE22, LE22, 29, (244, 250), seed=581),
                  face(L22, RE22, LE22, 40, (128, 128), seed=582)])
    others = [i for i in range(L22) if i not in RE22 + LE22]
    x[2, others[0]], x[2, L22 + others[0]] = 700.0, 650.0            # wholly outside, below and to the right
    x[2, others[1]], x[2, L22 + others[1]] = -300.5, 128.0           # wholly outside, to the left
    x[2, others[2]], x[2, L22 + others[2]] = 128.0, -41.0            # the patch's last rows on the canvas
    gpu_ctx.upload_images(images)
    want = oracle(images, x, RE22, LE22)
    for lv in range(4):
        got, idx = cells_features(gpu_ctx, x, lv)
        check_cells(got, idx, *want[lv], "off the canvas, level %d" % lv)
    # the patches wholly outside are all-zero cells: the descriptor of zero cells
    P = want[0][0].shape[1] // L22
    assert not cells_features(gpu_ctx, x, 0)[0][2, others[0] * P:(others[0] + 1) * P].any()


@pytest.mark.gpu
def test_detect_equals_the_levels_stepped_one_at_a_time(gpu_ctx, options, three_faces):
    """And a second detect gives the same bits."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(three_faces["images"])
    first = detect_equals_stepped_levels(gpu_ctx, three_faces["x"], L22, seed=7)
    gpu_ctx.set_x(three_faces["x"])
    assert np.array_equal(bits(first), bits(gpu_ctx.detect_batch()))
