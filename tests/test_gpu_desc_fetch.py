"""The fused descriptor launch (csrc/sdm_desc.hip) on landmarks whose patch is cut by a pass boundary of the pixel kernel, at 32 faces
per workgroup -- the layout whose waves take TWO patches each, the second one prefetched while the first is worked on.  A cut patch
has a second part of raw cells; the fused form loads it with the prefetch and adds it where the next iteration takes the patch over
(the store form adds it as it arrives), and the wave's regressor fragments are fetched in one batch, the last, conditional k-step's
pair included (desc_kernel<..., ONE>).

tests/test_gpu_fused_detect_shapes.py runs this wave layout at cell 6, which cuts no patch, and meets cut patches only on the 16-face
layouts, which have one iteration.  Here: 4 orientations, UoCTTI, the shipped cells 11, 10 and 8 (their relative patch sizes), L = 9,
22 and 32 (one, three and four column tiles: all one tile per wave), and 17, 33 and 70 rows -- 17: the second iteration of wave 0
holds one real face, every other patch of that iteration repeats the last face; 33: a second workgroup per landmark with one face;
70: a partial third.  Some rows are moved off the canvas.  Every case first asserts from the launch plan that it has a cut and an
uncut landmark.

One teacher-forced level per case: the integer patch decisions are the oracle's, fused against the unfused path of the same context
and against float64, two runs bit for bit, and the fused launch observed to have run.  Bounds: those of
tests/test_gpu_fused_detect.py and tests/test_gpu_fused_detect_shapes.py.  Mutants that these cases catch: profiles/desc_fetch.txt."""
import os

import numpy as np
import pytest

import landmark_count_cases as K
from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, SdmError, ibug, synth
from superviseddescent_amd.engine import hog_plan

THREADS = min(16, os.cpu_count() or 1)
LEVELS = {11: (1, 5, 11, 4, 1.0), 10: (1, 5, 10, 4, 0.7), 8: (1, 5, 8, 4, 0.4)}      # ibug.SHIPPED_HOG_PARAMS, levels 0 - 2
COUNTS = (9, 22, 32)
ROWS = (17, 33, 70)
CASES = [(cell, L) for cell in LEVELS for L in COUNTS]


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def faces():
    """70 synthetic faces and the rows of all 68 landmarks; rows 1 - 3 moved left, 4 - 6 moved down, so that patches straddle or leave
    the image; rows 16 (the one real face of a second iteration at 17 rows) and 32 (the one face of a second workgroup) stay"""
    images, boxes, gt = synth.make_faces(max(ROWS), seed=431)
    _, x0, _ = synth.make_samples(boxes, gt, ibug.IBUG68_IDS, n_perturb=0, seed=432)
    x0 = x0.copy()
    x0[1:4, :68] -= 150.0
    x0[4:7, 68:] += 170.0
    return images, x0


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    yield gpu_ctx
    gpu_ctx.set_detect_path(fused=True, split_store=False)


def random_regressor(F, L, seed):
    rng = np.random.default_rng(seed)
    R = (rng.standard_normal((F, 2 * L)) * (0.004 * (22.0 / L) ** 0.5)).astype(np.float32)
    R[:, 2 * L - 1] *= 37.0           # (as tests/test_gpu_fused_detect_shapes.py: one power-of-two scale per column of the float16 planes)
    R[:, 1] *= 1e-3
    return R


def test_shipped_levels_are_the_cases():
    assert [tuple(p) for p in ibug.SHIPPED_HOG_PARAMS[:3]] == [LEVELS[c] for c in (11, 10, 8)]


@pytest.mark.parametrize("cell,L", CASES, ids=["cell%d-L%d" % c for c in CASES])
def test_case_has_cut_and_uncut_landmarks(built, cell, L):
    plan = hog_plan(5, cell, 4, L)
    assert plan is not None
    cut = np.asarray(plan["cut"])
    assert cut.shape == (L,) and (cut != 0).any() and (cut == 0).any(), cut.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("cell,L", CASES, ids=["cell%d-L%d" % c for c in CASES])
def test_fused_level_with_cut_landmarks_on_the_two_iteration_layout(ctx, faces, cell, L):
    images, x68 = faces
    plan = hog_plan(5, cell, 4, L)
    cut = np.asarray(plan["cut"])
    assert (cut != 0).any() and (cut == 0).any(), cut.tolist()         # a case without both is a bad input, to be replaced
    hp, ohp = HoGParam(*LEVELS[cell]), orc.HoGParam(*LEVELS[cell])
    _, re, le = K.landmark_set(L)
    x_all = K.rows(x68, L)
    ctx.set_model_geometry(L, re, le, [hp])
    ctx.upload_images(images)
    ctx.set_sample_image_index(None)
    F = ctx.feature_dim(0)
    assert F == L * hp.patch_dim + 1
    R = random_regressor(F, L, 7000 + 100 * cell + L)
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
        ctx.set_detect_path(fused=True)
        ctx.set_x(x0); x_fused = ctx.detect_batch()
        assert np.array_equal(ctx.patch_indices(), oidx[:n])           # every face: none is left out of anything below
        with pytest.raises(SdmError):                                  # the fused launch ran: no feature rows to apply
            ctx.apply(0)
        assert x_fused.shape == (n, 2 * L) and np.isfinite(x_fused).all()
        ctx.set_x(x0); x_again = ctx.detect_batch()
        assert np.array_equal(bits(x_fused), bits(x_again))
        per_face = np.linalg.norm((x_fused - x_unfused).astype(np.float64), axis=1) / np.linalg.norm(x_unfused.astype(np.float64), axis=1)
        r64, u64 = rel_l2(x_fused, want[:n]), rel_l2(x_unfused, want[:n])
        # the cut and the uncut landmarks' columns apart: the update of landmark l's coordinates sums over ALL landmarks' descriptors,
        # so both figures see both kinds; they are printed, the bounds are on the rows
        print(f"cell {cell} L {L} N {n} ({int((cut != 0).sum())} cut): fused vs unfused median {np.median(per_face):.2e} max {per_face.max():.2e}; "
              f"vs float64 fused {r64:.2e} unfused {u64:.2e}")
        assert np.median(per_face) < 2e-7 and per_face.max() < 1e-4, (n, np.median(per_face), per_face.max())
        assert r64 < 1e-5, (n, r64)
