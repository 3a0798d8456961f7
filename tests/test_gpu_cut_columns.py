"""Raw cells of cut patches with only the cell columns a part holds moved through memory (csrc/sdm_hog_plan.hip: plan_cut_columns;
the pixel kernel's guarded store, csrc/sdm_hog_packed.hip; load_cells of csrc/sdm_desc.hip, store form and fused form), in the layout
cells[sample][landmark][part][cell column][cell row][2O].  The host side of the plan: tests/test_hog_plan_columns.py.

A column that a part does not hold is neither written nor read, so a wrong jA or jB, a store bit on the wrong matrix column or a
cell at another cell's address leaves a cell of a cut patch without one of its parts, or with stale memory in it: everything below
runs on NOISE images, where every cell of every patch is populated, and is compared with the CPU oracle inside the packed mode's
standing bounds (pixel_kernel_cases.PACKED_MAX_ABS, PACKED_REL_L2: those of tests/test_gpu_fold_overlap.py) or bit for bit with
another path through the same kernels.

Shapes.  RCR-22 on 256 x 256, the four shipped levels (cells 11 / 10 / 8 cut 14 / 12 / 7 patches of 22, cell 6 none: asserted), 3, 17
and 33 faces: below a descriptor workgroup's tile of 32 faces, a second iteration of its waves with one real face, and one face
past a full tile.  Faces 1, 2 and 4 hang off the canvas and three landmarks of face 0 lie wholly or almost wholly outside it, so
kept columns hold exact zeros as well.  One ragged pair of frames (200 x 310 at a pitch of 320, and 256 x 256) runs once.  Per
level: the cells -> descriptor store form against the oracle; the fused launch against the unfused path inside the bound of
tests/test_gpu_desc_fetch.py; a four-level detect against the levels stepped one at a time, bit for bit; all of it again under option
hog_two_load with the same bits.  The mutant these comparisons catch (jB one column too far right): profiles/cut_columns.txt."""
import numpy as np
import pytest

from pixel_kernel_cases import (L22, LE22, RE22, SHIPPED, bits, cells_features, check_cells, detect_equals_stepped_levels, face, noise,
                                options, oracle, oracle_per_row)  # noqa: F401
from superviseddescent_amd.engine import hog_plan

ROWS = (3, 17, 33)
NMAX = max(ROWS)


def build_rows():
    """33 faces of 22 landmarks: level-0 half-widths 24 .. 45, faces 1, 2 and 4 at corners of the canvas, three landmarks of face 0
    wholly outside it or with only their last rows on it"""
    rows = []
    for i in range(NMAX):
        centre = {1: (18, 12), 2: (244, 250), 4: (250, 20)}.get(i, (120 + (7 * i) % 17, 136 - (5 * i) % 19))
        rows.append(face(L22, RE22, LE22, 24 + (5 * i) % 22, centre, seed=900 + i))
    x = np.stack(rows)
    others = [i for i in range(L22) if i not in RE22 + LE22]
    x[0, others[0]], x[0, L22 + others[0]] = 700.0, 650.0
    x[0, others[1]], x[0, L22 + others[1]] = -300.5, 128.0
    x[0, others[2]], x[0, L22 + others[2]] = 128.0, -41.0
    return x


@pytest.fixture(scope="module")
def faces():
    images = noise(NMAX, seed=881)
    x = build_rows()
    return dict(images=images, x=x, want=oracle(images, x, RE22, LE22))


def test_the_levels_cut_patches_and_skip_columns(built):
    ncut, nskip = [], []
    for p in SHIPPED:
        cols = np.asarray(hog_plan(p.num_cells, p.cell_size, p.num_bins, L22)["columns"])
        cut = cols[cols[:, 0] != 0]
        ncut.append(len(cut))
        nskip.append(int((p.num_cells - 1 - cut[:, 1]).sum() + cut[:, 2].sum()))
    assert ncut == [14, 12, 7, 0] and all(s > 0 for s in nskip[:3]) and nskip[3] == 0, (ncut, nskip)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_store_form_against_the_oracle(gpu_ctx, options, faces, level):
    """Cells -> descriptors (store form) of 3, 17 and 33 faces inside the packed mode's bounds; under hog_two_load the same bits."""
    want, widx = faces["want"][level]
    options("hog_split_store", 1)
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    for n in ROWS:
        gpu_ctx.upload_images(faces["images"][:n])
        got, idx = cells_features(gpu_ctx, faces["x"][:n], level)
        check_cells(got, idx, want[:n], widx[:n], "cut columns, %d faces, level %d" % (n, level))
        options("hog_two_load", 1)
        two, idx2 = cells_features(gpu_ctx, faces["x"][:n], level)
        options("hog_two_load", 0)
        assert np.array_equal(idx2, widx[:n]) and np.array_equal(bits(got), bits(two)), n


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_fused_against_unfused(gpu_ctx, options, faces, level):
    """One teacher-forced level: the fused launch (deferred second part) against the unfused path of the same context, per face
    inside the bound of tests/test_gpu_desc_fetch.py; the integer patch decisions are the oracle's; twice and under hog_two_load
    the same bits."""
    _, widx = faces["want"][level]
    gpu_ctx.set_model_geometry(L22, RE22, LE22, [SHIPPED[level]])
    F = gpu_ctx.feature_dim(0)
    rng = np.random.default_rng(3300 + level)
    R = (rng.standard_normal((F, 2 * L22)) * 0.004).astype(np.float32)
    R[:, 2 * L22 - 1] *= 37.0
    R[:, 1] *= 1e-3
    gpu_ctx.set_regressor(0, R)
    try:
        for n in ROWS:
            x0 = faces["x"][:n]
            gpu_ctx.upload_images(faces["images"][:n])
            gpu_ctx.set_detect_path(fused=False)
            gpu_ctx.set_x(x0); x_unfused = gpu_ctx.detect_batch()
            assert np.array_equal(gpu_ctx.patch_indices(), widx[:n])
            gpu_ctx.set_detect_path(fused=False, split_store=True)
            gpu_ctx.set_x(x0); x_split = gpu_ctx.detect_batch()
            gpu_ctx.set_detect_path(fused=True)
            gpu_ctx.set_x(x0); x_fused = gpu_ctx.detect_batch()
            assert np.array_equal(gpu_ctx.patch_indices(), widx[:n])
            assert np.isfinite(x_fused).all() and not np.array_equal(x_fused, x0)
            gpu_ctx.set_x(x0); x_again = gpu_ctx.detect_batch()
            assert np.array_equal(bits(x_fused), bits(x_again))
            options("hog_two_load", 1)
            gpu_ctx.set_x(x0); x_two = gpu_ctx.detect_batch()
            options("hog_two_load", 0)
            assert np.array_equal(bits(x_fused), bits(x_two))
            for what, ref in (("unfused", x_unfused), ("unfused through the cells' store form", x_split)):
                per_face = np.linalg.norm((x_fused - ref).astype(np.float64), axis=1) / np.linalg.norm(ref.astype(np.float64), axis=1)
                print("level %d, %d faces: fused against %s, per face median %.2e max %.2e" % (level, n, what, np.median(per_face), per_face.max()))
                assert np.median(per_face) < 2e-7 and per_face.max() < 1e-4, (what, n, np.median(per_face), per_face.max())
    finally:
        gpu_ctx.set_detect_path(fused=True, split_store=False)


@pytest.mark.gpu
def test_detect_equals_the_levels_stepped_one_at_a_time(gpu_ctx, options, faces):
    """Four levels, 33 faces; a second detect and one under hog_two_load give the same bits."""
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(faces["images"])
    first = detect_equals_stepped_levels(gpu_ctx, faces["x"], L22, seed=17)
    gpu_ctx.set_x(faces["x"])
    assert np.array_equal(bits(first), bits(gpu_ctx.detect_batch()))
    options("hog_two_load", 1)
    gpu_ctx.set_x(faces["x"])
    two = gpu_ctx.detect_batch()
    options("hog_two_load", 0)
    assert np.array_equal(bits(first), bits(two))


@pytest.mark.gpu
def test_ragged_pair_of_frames(gpu_ctx, options):
    """200 x 310 at a pitch of 320 bytes beside 256 x 256, the samples in the other order than the frames: the four levels' store form
    against the oracle."""
    import torch
    sizes = [(200, 310, 320), (256, 256, 256)]                # h, w, pitch
    order = np.array([1, 0], np.int32)
    x = np.stack([face(L22, RE22, LE22, 37, (128, 128), seed=971, spread=40.0), face(L22, RE22, LE22, 31, (170, 90), seed=972, spread=40.0)])
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    rng = np.random.default_rng(973)
    host = [rng.integers(0, 256, (h, pitch)).astype(np.uint8) for h, _, pitch in sizes]
    keep = [torch.from_numpy(a).cuda() for a in host]
    gpu_ctx.set_frames_device([t[:, :w] for t, (_, w, _) in zip(keep, sizes)])
    gpu_ctx.set_sample_image_index(order)
    options("hog_split_store", 1)
    try:
        for lv in range(4):
            got, idx = cells_features(gpu_ctx, x, lv)
            want, widx = oracle_per_row([host[i][:, :sizes[i][1]] for i in order], x, RE22, LE22, lv)
            check_cells(got, idx, want, widx, "ragged pair, level %d" % lv)
    finally:
        gpu_ctx.upload_images(noise(1, seed=1))               # (the frames go out of scope)
        gpu_ctx.set_sample_image_index(None)
