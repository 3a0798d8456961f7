"""The band-slot weights of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_row_weights.txt).

The detect instances (cell sizes 11 / 10 / 8 / 6) no longer build and read a table of the weights {ws0, ws1} a pixel row multiplies its
gradient magnitude by: the pairs are compile-time constants from the ONE definition of them (csrc/sdm_kernels.h: packed_row_const, which
also fills the level's row table on the host), pinned in scalar registers; sdm_hog_plan_build compares the compiler's values with the
host's before it hands out a plan.

CPU part.  sdm_debug_hog_band_weights returns the compiler's values for the four cell sizes; they must be, bit for bit, a numpy
restatement of hog.c:697-704 that takes the steps fill_row_tab takes (float64 division and subtraction, float32 casts, vl_floor_f, zero
for the cell rows -1 and C, the pair swapped on odd bands) -- and the same for cell sizes 7, 9 and 12, which have no specialised instance:
there only the plan's guard uses the function.

GPU part.  L = 22 with RCR-22's eyes, 256 x 256 noise images, option hog_split_store on (the feature rows are made of the raw cells).
Batches of THREE faces: 18 / 15 / 11 units per face at levels 1 - 3, so a workgroup's four waves hold units of two faces and the last
workgroup is partial (at level 0 a face is 20 units, five whole workgroups: a plan property, asserted with the rest).  Per level nine rows
= three batches: pixel_kernel_cases.edge_rows (cvRound ties, negative coordinates, patches off every border, small and large faces) and
one face per row loop of the level's instance -- level 0: half-width 30 (pair loop) and 43 (two-load); level 1: 24 (one-load) and 28
(two-load); levels 2 and 3: one enlarged patch (one-load) and one reduced (two-load) each.  The weights do not depend on the half-width,
only which loop runs does: these are the smallest shapes that reach every row of every loop.  Checked: the feature rows and patch indices
against the CPU oracle inside the packed mode's standing bounds (check_cells); the same rows under option hog_two_load, bit for bit (both
loops read the constants); a four-level detect against the levels stepped one at a time.  One level with a cell size that has no
specialised instance (cell 9) stays inside the same bounds: the generic instance, which keeps its table, and the guard's other branch.

A test cannot see the parent's bits; the landmark dump of the two builds is compared in profiles/hog_row_weights.txt."""
import numpy as np
import pytest

from oracle import sdm_oracle as orc
from pixel_kernel_cases import (L22, LE22, RE22, RELS, SHIPPED, SIZES, bits, cells_features, check_cells, detect_equals_stepped_levels,
                                edge_rows, face, noise, options, units_per_face)  # noqa: F401
from superviseddescent_amd import HoGParam
from superviseddescent_amd.engine import hog_band_weights, hog_plan

C = 5
SPECIALISED = (11, 10, 8, 6)
OTHERS = (7, 9, 12)
# (half-width, centre) of the two faces added per level, one per row loop of the level's instance
LOOP_FACES = {
    0: ((30, (124, 130)), (43, (131, 125))),      # pair loop; two-load (outside the pair loop's range 27 .. 41)
    1: ((24, (127, 126)), (28, (129, 131))),      # one-load (48 < 50 columns: enlarged); two-load (56 > 50: reduced)
    2: ((15, (126, 129)), (26, (130, 127))),      # one-load (30 < 40); two-load (52 > 40)
    3: ((11, (128, 125)), (19, (125, 130))),      # one-load (22 < 30); two-load (38 > 30)
}


def restated(cell, cells):
    """hog.c:697-704 as fill_row_tab computes it: ([S][2] float32 {slot 0, slot 1}, [S] band)."""
    f32 = np.float32
    out, band = np.zeros((cells * cell, 2), f32), []
    for d in range(cells * cell):
        hx = f32((d + 0.5) / float(cell) - 0.5)               # float64 division and subtraction, one cast
        b = int(hx)                                           # C's (int): toward zero
        if not (hx >= 0.0 or f32(b) == hx):                   # vl_floor_f
            b -= 1
        w2 = f32(hx - f32(b))                                 # float32 subtraction
        w1 = f32(1.0 - float(w2))                             # float64 subtraction, cast
        wlo = w1 if b >= 0 else f32(0.0)                      # the cell rows -1 and C do not exist
        whi = w2 if b + 1 <= cells - 1 else f32(0.0)
        out[d] = (whi, wlo) if b & 1 else (wlo, whi)          # band b lives in slot b & 1
        band.append(b)
    return out, np.array(band)


@pytest.mark.parametrize("cell", SPECIALISED + OTHERS)
def test_band_weights_are_the_restated_arithmetic(built, cell):
    want, band = restated(cell, C)
    got = hog_band_weights(cell, C)
    assert got.shape == (C * cell, 2) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))
    # what the restatement must show for the checks above to mean something
    assert band.min() == -1 and band.max() == C - 1 and (np.diff(band) >= 0).all()
    first, last = band == -1, band == C - 1
    assert first.sum() == cell // 2 and last.sum() == cell - cell // 2
    # band -1 (odd: swapped) carries the weight of cell row 0 in slot 0 and zero for cell row -1; band C - 1 = 4 (even) zero for cell row C
    assert (bits(got[first, 1]) == 0).all() and (got[first, 0] > 0).all()
    assert (bits(got[last, 1]) == 0).all() and (got[last, 0] > 0).all()
    inner = ~first & ~last
    # (an odd cell size has a row on the centre of each cell: weights 1 and +0)
    assert (got[inner] >= 0).all() and not np.signbit(got).any() and np.abs(got[inner].sum(axis=1) - 1.0).max() <= 2.0 ** -23
    # odd bands carry the pair swapped: slot (b & 1) holds the weight of cell row b, which falls as the row moves down its band
    own = got[np.arange(C * cell), band & 1]
    for b in range(C):
        assert (np.diff(own[band == b]) < 0).all(), b
    # the plan's guard accepts the level (it compares these values with the level's row table)
    assert hog_plan(C, cell, 4, L22) is not None


def test_band_weights_arguments(built):
    from superviseddescent_amd import SdmError
    for cell, cells in ((0, 5), (11, 0), (13, 5), (11, 6)):
        with pytest.raises(SdmError):
            hog_band_weights(cell, cells)
    assert hog_band_weights(12, 5).shape == (60, 2) and hog_band_weights(8, 8).shape == (64, 2)


def test_the_batches_are_the_ones_intended(built):
    """Three faces: workgroups of four waves straddle faces and the last one is partial at levels 1 - 3; level 0 is whole workgroups."""
    gpfs = [units_per_face(lv, L22)[0] for lv in range(4)]
    assert gpfs == [20, 18, 15, 11]
    assert all(g % 4 != 0 and (3 * g) % 4 != 0 for g in gpfs[1:]) and gpfs[0] % 4 == 0
    for lv, pairs in LOOP_FACES.items():
        (h_a, _), (h_b, _) = pairs
        assert 2 * h_b > SIZES[lv] and (lv == 0 or 2 * h_a < SIZES[lv])      # reduced; enlarged
    assert SIZES[0] < 2 * LOOP_FACES[0][0][0] < 1.5 * SIZES[0] and 2 * LOOP_FACES[0][1][0] >= 1.5 * SIZES[0]


@pytest.fixture(scope="module")
def level_rows():
    """Per level: nine noise images, nine rows (seven edge rows, two loop faces), the oracle's feature rows and patch indices."""
    out = {}
    edges = edge_rows(L22, RE22, LE22, seed=811)
    for lv in range(4):
        images = noise(9, seed=820 + lv)
        faces = [face(L22, RE22, LE22, h, c, seed=830 + 2 * lv + i, level=lv) for i, (h, c) in enumerate(LOOP_FACES[lv])]
        # one loop face in each of the first two batches, between two edge rows
        x = np.stack([edges[0], faces[0], edges[1], edges[2], faces[1], edges[3], edges[4], edges[5], edges[6]])
        want, widx = orc.hog_features_batch(images, None, x, RE22, LE22, orc.HoGParam(*_params(lv)), want_idx=True)
        out[lv] = dict(images=images, x=x, want=want, widx=widx)
    return out


def _params(lv):
    p = SHIPPED[lv]
    return p.vlhog_variant, p.num_cells, p.cell_size, p.num_bins, p.relative_patch_size


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_cells_against_the_oracle_in_every_loop(gpu_ctx, options, level_rows, level):
    d = level_rows[level]
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    taps, info = gpu_ctx.debug_hog_taps(level)
    assert info["cells_launch"]
    h_a, h_b = (h for h, _ in LOOP_FACES[level])
    assert d["widx"][1, 0] == h_a and d["widx"][4, 0] == h_b
    if level == 0:
        pair, pinfo = gpu_ctx.debug_hog_pair_taps(0)
        assert pinfo["pair_instance"] and int(pair[h_a, 0, 2]) == 1 and int(pair[h_b, 0, 2]) == 0
    else:
        assert info["one_load_instance"] and int(taps[h_a, 0, 7]) == 1 and int(taps[h_b, 0, 7]) == 0
    for k in range(3):
        pick = slice(3 * k, 3 * k + 3)
        gpu_ctx.upload_images(d["images"][pick])
        got, idx = cells_features(gpu_ctx, d["x"][pick], level)
        check_cells(got, idx, d["want"][pick], d["widx"][pick], "level %d, faces %d .. %d" % (level, 3 * k, 3 * k + 2))
        options("hog_two_load", 1)
        two, idx2 = cells_features(gpu_ctx, d["x"][pick], level)
        options("hog_two_load", 0)
        assert np.array_equal(idx2, idx) and np.array_equal(bits(got), bits(two)), k


@pytest.mark.gpu
def test_detect_equals_the_levels_stepped_one_at_a_time(gpu_ctx, options, level_rows):
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    for lv in (0, 1):
        d = level_rows[lv]
        gpu_ctx.upload_images(d["images"][:3])
        detect_equals_stepped_levels(gpu_ctx, d["x"][:3], L22, seed=840 + lv)


@pytest.mark.gpu
def test_a_cell_size_without_a_specialised_instance(gpu_ctx, options):
    """Cell 9, 5 x 5 cells, 4 orientations, two faces (one enlarged patch, one reduced): the generic instance."""
    rel = RELS[1]
    params = (SHIPPED[1].vlhog_variant, C, 9, 4, SHIPPED[1].relative_patch_size)
    assert hog_plan(C, 9, 4, L22) is not None
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, [HoGParam(*params)])
    images = noise(2, seed=851)
    x = np.stack([face(L22, RE22, LE22, 20, (127, 129), seed=852, level=1), face(L22, RE22, LE22, 30, (130, 126), seed=853, level=1)])
    want, widx = orc.hog_features_batch(images, None, x, RE22, LE22, orc.HoGParam(*params), want_idx=True)
    assert widx[:, 0].tolist() == [20, 30] and float(np.float32(params[4])) == rel
    gpu_ctx.upload_images(images)
    assert gpu_ctx.debug_hog_taps(0)[1]["cells_launch"]
    got, idx = cells_features(gpu_ctx, x, 0)
    check_cells(got, idx, want, widx, "cell 9")
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
