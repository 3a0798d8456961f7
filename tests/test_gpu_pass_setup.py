"""The pass set-up of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, CELLS form; profiles/hog_pass_setup.txt): a wave
requests what depends on (level, pass, lane) only -- its lane_tab entry, the fold weights, the pass's four words, the band-weight
rows -- before the geometry's arithmetic, takes the pass's words from ONE 16-byte load and picks its segment's by selects, and clears
its column rows with stores at constant offsets.  Checked against the CPU oracle at the shapes where a set-up can go wrong: the
integer decisions (sdm_get_patch_indices) are the oracle's, the feature rows read through the raw cells (hog_split_store) are inside
the standing bounds of the packed mode (tests/test_gpu_parity.py::check_features), and a four-level detect with random regressors
is, bit for bit, the same four levels stepped one at a time.

Shapes: 1, 3 and 7 faces on 256 x 256 noise images and one ragged set of frames with differing sizes and strides; L = 5, 22, 32
and 33 (2L = 64 and 66: either side of the fused detect's limit); all four shipped levels; eye counts (1, 1), (2, 2), (3, 3), (4, 4)
and (1, 4): the reciprocal and the division branch of the eye centres.  The face counts make a workgroup's four waves straddle two
faces and leave the last workgroup partial (asserted from the plans).  Rows: landmarks on x.5 (cvRound ties), negative coordinates,
patches off every border, small and large faces.  L = 1 has one landmark for both eyes, so its inter-eye distance is zero: with it
and with a tiny face SDM_ERR_EMPTY_PATCH must still be reported.

Half-width sweep: eyes on a horizontal line, the left one at x = 0 so that the float difference IS the right eye's x, chosen so
that rel * IED / 2 lands on k + 1/2, within a few float steps of it either side, and 2^-10 either side of it, for several k at each
level's rel (k = 127 reaches the end of the taps table): h must be the oracle's round() in double, ties included.

The detect-against-stepped-levels comparison runs the same kernel on both sides: it pins the launch sequence, not the set-up.  What
can see a set-up error are the index and the feature comparisons with the oracle."""
import numpy as np
import pytest

from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, SdmError, ibug
from superviseddescent_amd._lib import SDM_HOG_COLUMNS
from superviseddescent_amd.engine import hog_plan

SHIPPED = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
RELS = [float(np.float32(p.relative_patch_size)) for p in SHIPPED]
SIZES = [p.num_cells * p.cell_size for p in SHIPPED]

# (L, right-eye indices, left-eye indices)
CASES = {
    "L5-eyes1+4": (5, [0], [1, 2, 3, 4]),
    "L5-eyes2+2": (5, [0, 1], [3, 4]),
    "L22-eyes3+3": (22, [2, 5, 7], [10, 11, 20]),
    "L22-eyes1+1": (22, [21], [0]),
    "L32-eyes4+4": (32, [0, 1, 2, 3], [28, 29, 30, 31]),
    "L33-eyes2+2": (33, [32, 4], [0, 16]),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(n, seed, h=256, w=256):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w)).astype(np.uint8)


def _rows(L, re, le, seed):
    """Seven rows of 2L landmarks: eye centres 20 .. 150 px apart on a tilted line, the rest scattered; then, row by row, the edge
    cases of the docstring."""
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


def _oracle_indices(x, L, re, le, rel):
    out = np.zeros((x.shape[0], 1 + 2 * L), np.int32)
    for n in range(x.shape[0]):
        v = float(np.float32(rel)) * orc.get_ied(x[n], re, le) / 2.0
        out[n, 0] = int(np.floor(v + 0.5))                   # C's round() of a value >= 0
        out[n, 1:] = [orc.cv_round(c) for c in x[n]]
    return out


O_SHIPPED = [orc.HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]


@pytest.fixture
def restore(gpu_ctx):
    yield
    gpu_ctx.set_option("hog_split_store", 0)
    gpu_ctx.set_sample_image_index(None)


def _check_against_the_oracle(gpu_ctx, x, L, re, le, oracle_images, what):
    """Feature rows of the four levels through the raw cells and the patch indices of each against the oracle (`oracle_images`: one
    image per row of x), then a four-level detect against the same levels stepped one at a time."""
    rng = np.random.default_rng(6)
    gpu_ctx.set_option("hog_split_store", 1)
    for lv in range(4):
        gpu_ctx.set_x(x)
        got = gpu_ctx.hog_features(lv, fetch=True)
        idx = gpu_ctx.patch_indices()
        assert np.array_equal(idx, _oracle_indices(x, L, re, le, RELS[lv])), (what, lv)
        want = np.concatenate([orc.hog_features_batch(im[None], None, x[i:i + 1], re, le, O_SHIPPED[lv]) for i, im in enumerate(oracle_images)])
        diff = float(np.abs(got - want).max())
        rel = float(np.linalg.norm((got - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
        print("%s level %d: %d rows, h %d .. %d, features against the oracle max abs %.3g rel L2 %.3g"
              % (what, lv, x.shape[0], idx[:, 0].min(), idx[:, 0].max(), diff, rel))
        assert diff <= 1e-6 and rel <= 5e-7, (what, lv)          # tests/test_gpu_parity.py::check_features, packed mode
    gpu_ctx.set_option("hog_split_store", 0)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, (rng.standard_normal((gpu_ctx.feature_dim(lv), 2 * L)) * 1e-3).astype(np.float32))
    gpu_ctx.set_x(x)
    final = gpu_ctx.detect_batch()
    gpu_ctx.set_x(x)
    for lv in range(4):
        gpu_ctx.detect_level(lv)
    assert np.isfinite(final).all() and np.array_equal(_bits(final), _bits(gpu_ctx.get_x())), what


def test_face_counts_straddle_and_leave_a_partial_workgroup(built):
    """1, 3 and 7 faces against the plans' units per face: somewhere a workgroup of four waves holds units of two faces, and somewhere
    the last workgroup is partial."""
    straddle = partial = 0
    for L, _, _ in CASES.values():
        for p in SHIPPED:
            plan = hog_plan(p.num_cells, p.cell_size, p.num_bins, L)
            gpf = plan["n_main"] * plan["P"] + plan["Pt"]
            for n in (3, 7):
                straddle += gpf % 4 != 0
                partial += (n * gpf) % 4 != 0
            partial += gpf % 4 != 0                           # one face
    assert straddle >= 8 and partial >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_set_up_against_the_oracle(gpu_ctx, restore, case):
    L, re, le = CASES[case]
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    rows = _rows(L, re, le, seed=1000 + L + len(re) * 7 + len(le))
    for n, pick in ((1, slice(1, 2)), (3, slice(2, 5)), (7, slice(0, 7))):
        images = _noise(n, seed=40 + n)
        gpu_ctx.upload_images(images)
        gpu_ctx.set_sample_image_index(None)
        _check_against_the_oracle(gpu_ctx, rows[pick], L, re, le, images, "%s, %d faces" % (case, n))


@pytest.mark.gpu
def test_ragged_frames_with_differing_strides(gpu_ctx, restore):
    import torch
    L, re, le = CASES["L22-eyes3+3"]
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    x = _rows(L, re, le, seed=77)
    x[:, :L] *= np.float32(0.5)                              # (the smallest frame is 131 x 133)
    x[:, L:] *= np.float32(0.5)
    sizes = [(256, 256, 256), (200, 240, 320), (256, 130, 384), (97, 256, 257), (256, 256, 512), (255, 201, 300), (131, 133, 192)]   # h, w, pitch
    rng = np.random.default_rng(78)
    host = [rng.integers(0, 256, (h, pitch)).astype(np.uint8) for h, _, pitch in sizes]
    keep = [torch.from_numpy(a).cuda() for a in host]
    gpu_ctx.set_frames_device([t[:, :w] for t, (_, w, _) in zip(keep, sizes)])
    order = np.array([3, 1, 6, 0, 2, 5, 4], np.int32)
    gpu_ctx.set_sample_image_index(order)
    _check_against_the_oracle(gpu_ctx, x, L, re, le, [np.ascontiguousarray(host[i][:, :sizes[i][1]]) for i in order], "ragged")
    gpu_ctx.upload_images(_noise(1, seed=1))                 # (the frames go out of scope)


@pytest.mark.gpu
def test_empty_patch_is_still_reported(gpu_ctx, restore):
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.upload_images(_noise(3, seed=9))
    gpu_ctx.set_sample_image_index(None)

    def codes(x):
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
    L, re, le = CASES["L22-eyes3+3"]
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    for lv in range(4):
        gpu_ctx.set_regressor(lv, np.zeros((gpu_ctx.feature_dim(lv), 2 * L), np.float32))
    x = _rows(L, re, le, seed=5)[:3]
    x[1] = (128.0 + (x[1] - 128.0) * np.float32(0.01)).astype(np.float32)
    assert all(float(np.float32(r)) * orc.get_ied(x[1], re, le) / 2.0 < 0.49 for r in RELS)
    assert codes(x) == [-4] * 5
    # and the same context goes on working
    assert codes(_rows(L, re, le, seed=5)[:3]) == [0] * 5


def _sweep_rows(rel, ks):
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


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_half_width_sweep_around_the_ties(gpu_ctx, restore, level):
    L, re, le = 5, [0], [1]
    rel, S = RELS[level], SIZES[level]
    ks = sorted({0, 1, 3, S // 2 - 1, S // 2, S // 2 + 1, S, 100, 126, 127})
    x, ds, t = _sweep_rows(rel, ks)
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
    gpu_ctx.set_hog_mode(SDM_HOG_COLUMNS)
    gpu_ctx.set_model_geometry(L, re, le, SHIPPED)
    gpu_ctx.upload_images(_noise(4, seed=31))
    gpu_ctx.set_sample_image_index((np.arange(x.shape[0]) % 4).astype(np.int32))

    gpu_ctx.set_option("hog_split_store", 1)
    gpu_ctx.set_x(x)
    f = gpu_ctx.hog_features(level, fetch=True)
    idx = gpu_ctx.patch_indices()
    print("level %d: %d rows, h %d .. %d" % (level, x.shape[0], want_h.min(), want_h.max()))
    assert np.isfinite(f).all() and np.array_equal(idx[:, 0], want_h)
    assert np.array_equal(idx[:, 1:], [[orc.cv_round(c) for c in r] for r in x])
