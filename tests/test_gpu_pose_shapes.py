"""Head pose on the device at every model size, level count and batch edge (csrc/sdm_pose.hip; the cases and the reasons for them:
tests/pose_cases.py, their conditions: tests/test_pose_cases_host.py).  tests/test_gpu_pose.py runs the cascade at K = 10, 9 and 5,
three levels and one regulariser: one of the Gram kernel's five instantiations, the resident path of the cascade kernel, a solve of
20 x 26.  Here every K of pose_cases.KS trains and runs against the float64 restatement (tests/pose_f64.py) under all four regulariser
settings, the staged cascade path meets the bit-level contracts, 16 levels run in one launch at K = 64, levels 5 ... 8 run without
levels 0 ... 4, the row counts sit at the kernels' block, chunk and reduce edges, and the gather reads landmark sets other than RCR-22's.

Bounds (pose_cases): features FEAT_TOL; R within 2^-23 of max |R64| of the float64 solve of the device's own rows; x_{k+1} and the
cascade within the project's 1e-7 of ||x*|| / 1e-5 of the angles' norm, or four times the float32 numpy restatement's own error on the
same case where that is larger (the factor covers the device's sinf / cosf and summation order, which numpy does not share).

What the device measured per K stands beside the bounds (pose_cases.DEVICE_MEASURED): features <= 3.1e-6 (K = 1; <= 1.3e-6 from K = 12
up), R <= 5.2e-8 of max |R64| -- the float32 rounding alone -- and x_{k+1} and the cascade at most 0.26 of their bounds.  That the
module can fail: profiles/pose_shape_mutants.txt.
"""
import numpy as np
import pytest

import landmark_count_cases as LC
import pose_cases as C
import pose_f64 as P
from superviseddescent_amd import Context, HoGParam, SdmError

pytestmark = pytest.mark.gpu
N = C.N_DEFAULT
STAGED_KS = [17, 33, 64]
REG_IDS = [f"{'matrixnorm' if t else 'manual'}{p:g}-{'all' if last else 'notlast'}" for t, p, last in C.REGULARISERS]


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    yield c
    c.close()


def code(fn, *a):
    with pytest.raises(SdmError) as e:
        fn(*a)
    return e.value.code


class Data:
    """targets, templates and model of one K: N rows unless asked otherwise (a longer set starts with the same rows)"""
    cache = {}

    def __init__(self, K, n):
        self.K, self.n, self.pts = K, n, C.points(K)
        self.x_star = C.poses(n, K)
        self.y = C.templates(self.x_star, self.pts)
        self.x0 = C.start(n)

    @classmethod
    def of(cls, K, n=N):
        if (K, n) not in cls.cache:
            cls.cache[K, n] = cls(K, n)
        return cls.cache[K, n]


def load(ctx, d, x=None, targets=True):
    ctx.pose_set_model(d.pts)
    ctx.pose_set_x(d.x0 if x is None else x)
    ctx.pose_set_templates(d.y)
    if targets:
        ctx.pose_set_targets(d.x_star)


def check_level(ctx, d, level, xk, reg, label):
    """One teacher-forced level from x_k (the rows are loaded): every check of the module's docstring.  Returns (R, x_{k+1})."""
    reg_type, param, last = reg
    n, pts = d.n, d.pts
    ctx.pose_set_x(xk)
    A32 = ctx.pose_features().astype(np.float64)              # the float32 rows the device's normal equations are formed from
    lam_rule = P.reference_lambda(A32.T @ A32, n, reg_type, param)
    R, lam = ctx.pose_train_level(level, reg_type, param, last)
    x_dev = ctx.pose_get_x()
    assert abs(lam - lam_rule) <= 4e-7 * lam_rule, (label, lam, lam_rule)
    # R: the float64 solve of the same float32 rows with the lambda the device used
    R64, cond = C.solve64(A32, xk.astype(np.float32) - d.x_star.astype(np.float32), lam, last)
    assert cond < C.COND_CAP, (label, cond)
    r_err = np.abs(R - R64).max() / np.abs(R64).max()
    # x_{k+1}: the float64 level from the same x_k, as tests/test_gpu_pose.py; the float32 restatement of the same case beside it
    _, _, x64 = C.level64(xk, d.x_star, d.y, pts, reg_type, param, last)
    _, _, x32 = C.level32(xk, d.x_star, d.y, pts, reg_type, param, last)
    full, ang = C.x_errors(x_dev, x64, d.x_star)
    b_full, b_ang = C.x_bounds(x32, x64, d.x_star)
    print(f"{label} level {level}: lambda {lam:.7g} (rule {lam_rule:.7g}), cond {cond:.3g}, R {r_err:.3e} (bound {C.R_TOL:.3e}), "
          f"x_k+1 {full:.3e} / {ang:.3e} (bounds {b_full:.3e} / {b_ang:.3e})")
    assert r_err <= C.R_TOL, (label, r_err)
    assert full < b_full and ang < b_ang, (label, full, ang, b_full, b_ang)
    assert np.array_equal(ctx.pose_get_regressor(level), R)
    # the same level again: the same bits
    ctx.pose_set_x(xk)
    R2, lam2 = ctx.pose_train_level(level, reg_type, param, last)
    assert np.array_equal(R2, R) and lam2 == lam and np.array_equal(ctx.pose_get_x(), x_dev)
    # the update training leaves is the test launch of this level
    ctx.pose_set_x(xk)
    ctx.pose_test(level, 1)
    assert np.array_equal(ctx.pose_get_x(), x_dev)
    return R, x_dev


TRAINED = {}


def trained(ctx, K):
    """the three float32 regressors of K trained on the device (MatrixNorm 2.0, every row), installed in ctx"""
    d = Data.of(K)
    if K not in TRAINED:
        load(ctx, d)
        TRAINED[K] = [ctx.pose_train_level(level, 1, 2.0, True)[0] for level in range(3)]
    ctx.pose_set_model(d.pts)
    for level, R in enumerate(TRAINED[K]):
        ctx.pose_set_regressor(level, R)
    return TRAINED[K]


def run(ctx, x, tmpl, first, n_levels):
    ctx.pose_set_x(x)
    ctx.pose_set_templates(tmpl)
    ctx.pose_test(first, n_levels)
    return ctx.pose_get_x()


def check_cascade(ctx, d, Rs, label, first=0):
    x_dev = run(ctx, d.x0, d.y, first, len(Rs))
    x64 = C.cascade64(d.x0, d.y, Rs, d.pts)
    full, ang = C.x_errors(x_dev, x64, d.x_star)
    b_full, b_ang = C.x_bounds(C.cascade32(d.x0, d.y, Rs, d.pts), x64, d.x_star)
    print(f"{label}: cascade of {len(Rs)} vs float64 {full:.3e} / {ang:.3e} (bounds {b_full:.3e} / {b_ang:.3e})")
    assert full < b_full and ang < b_ang, (label, full, ang, b_full, b_ang)
    return x_dev


@pytest.mark.parametrize("K", C.KS)
def test_features_at_every_K_and_row_count(ctx, K):
    pts = C.points(K)
    ctx.pose_set_model(pts)
    worst = 0.0
    for n in C.N_ROWS + [N]:                                  # (every n differs from the one before: no templates for the new rows)
        x, x_star = C.poses(n, 1000 + K), C.poses(n, K)
        ref = P.project(x, pts)
        ctx.pose_set_x(x)
        f = ctx.pose_features()                               # no templates: the projections themselves
        assert f.shape == (n, 2 * K)
        e0 = C.rel_err(f, ref).max()
        t = C.templates(x_star, pts)
        ctx.pose_set_templates(t)
        e1 = (np.abs(ctx.pose_features().astype(np.float64) - (ref - t)).max(1) / np.abs(ref).max(1)).max()
        worst = max(worst, e0, e1)
        assert e0 < C.FEAT_TOL and e1 < C.FEAT_TOL, (K, n, e0, e1)
    print(f"K={K}: device features vs float64 over N in {C.N_ROWS + [N]}, max relative error {worst:.3e}")


@pytest.mark.parametrize("reg", C.REGULARISERS, ids=REG_IDS)
@pytest.mark.parametrize("K", C.KS)
def test_teacher_forced_training_at_every_K(ctx, K, reg):
    d = Data.of(K)
    load(ctx, d)
    xk = d.x0
    for level in range(3):
        _, xk = check_level(ctx, d, level, xk, reg, f"K={K} {REG_IDS[C.REGULARISERS.index(reg)]}")


@pytest.mark.parametrize("K,n", [(K, n) for K in (13, 43) for n in C.N_GRAM] + [(64, 32769)])
def test_training_at_every_gram_block_count(ctx, K, n):
    d = Data.of(K, n)
    load(ctx, d)
    check_level(ctx, d, 0, d.x0, C.REGULARISERS[0], f"K={K} N={n} ({C.gram_blocks(n)} Gram blocks of {C.gram_rows(n)} rows)")


@pytest.mark.parametrize("K", C.KS)
def test_cascade_against_float64_at_every_K(ctx, K):
    Rs = trained(ctx, K)
    for n in [N] + (C.N_ROWS if K in (16, 17, 33, 64) else []):
        check_cascade(ctx, Data.of(K, n), Rs, f"K={K} N={n}")


@pytest.mark.parametrize("K", STAGED_KS)
def test_bit_contracts_on_the_staged_path(ctx, K):
    trained(ctx, K)
    d = Data.of(K)
    init = d.x0.copy()
    init[:, :3] = np.random.default_rng(42).uniform(-5, 5, (N, 3))
    fused = run(ctx, init, d.y, 0, 3)
    assert not np.array_equal(fused, init)
    ctx.pose_set_x(init)
    for level in range(3):
        ctx.pose_test(level, 1)
    assert np.array_equal(ctx.pose_get_x(), fused)
    for a, b in ((0, 17), (250, 270), (300, N)):              # other lanes; across the edge of the first block
        assert np.array_equal(run(ctx, init[a:b], d.y[a:b], 0, 3), fused[a:b]), (a, b)
    for i in range(N):
        assert np.array_equal(run(ctx, init[i:i + 1], d.y[i:i + 1], 0, 3)[0], fused[i]), i


def test_sixteen_levels_in_one_launch(built):
    K = C.MAX_K
    d = Data.of(K)
    Rs = C.random_regressors(K, C.MAX_LEVELS, d.y, d.pts, 7)
    c = Context(0)
    try:
        c.pose_set_model(d.pts)
        for level, R in enumerate(Rs):
            c.pose_set_regressor(level, R)
            assert np.array_equal(c.pose_get_regressor(level), R)
        fused = run(c, d.x0, d.y, 0, C.MAX_LEVELS)
        c.pose_set_x(d.x0)
        seen = []
        for level in range(C.MAX_LEVELS):
            c.pose_test(level, 1)
            seen.append(c.pose_get_x())
        assert np.array_equal(seen[-1], fused)
        steps = [np.abs(b - a).max() for a, b in zip([d.x0] + seen[:-1], seen)]
        assert all(0.0 < s < 1.0 for s in steps), steps      # every level moves the rows, none by a degree
        check_cascade(c, d, Rs[:3], f"K={K}, random regressors")
        assert np.array_equal(run(c, d.x0, d.y, 0, 3), seen[2])
    finally:
        c.close()


def test_first_level_offset(built):
    K = 33
    d = Data.of(K)
    Rs = C.random_regressors(K, 4, d.y, d.pts, 9)
    c = Context(0)
    try:
        c.pose_set_model(d.pts)
        for i, R in enumerate(Rs):
            c.pose_set_regressor(5 + i, R)
        fused = check_cascade(c, d, Rs, f"K={K}, levels 5 ... 8", first=5)
        c.pose_set_x(d.x0)
        for level in range(5, 9):
            c.pose_test(level, 1)
        assert np.array_equal(c.pose_get_x(), fused)
        assert np.array_equal(run(c, d.x0, d.y, 6, 2), run(c, run(c, d.x0, d.y, 6, 1), d.y, 7, 1))
        assert not np.array_equal(run(c, d.x0, d.y, 6, 2), run(c, d.x0, d.y, 5, 2))
        c.pose_set_x(d.x0)
        assert code(c.pose_test, 4, 2) == -1                  # level 4 has no regressor
        assert code(c.pose_test, 8, 2) == -1                  # nor has level 9
        assert np.array_equal(c.pose_get_x(), d.x0)           # a refused run leaves the rows alone
    finally:
        c.close()


GATHER = [(L, K) for L in (5, 33, 68, 72) for K in sorted({min(k, L) for k in (1, 17, 64)})]


@pytest.mark.parametrize("L,K", GATHER)
def test_gather_at_other_landmark_counts(built, L, K):
    """With every model point at the origin the projection is exactly 0, so -features is the gathered template itself (the trick
    of test_detect_to_pose_on_the_device): compared bit for bit with the float32 host formula."""
    rng = np.random.default_rng(1000 * L + K)
    _, re, le = LC.landmark_set(L)
    sizes = [(64, 48), (33, 71), (129, 20), (17, 17), (640, 481)]                   # (w, h): odd sizes have centres at .5
    images = [np.full((h, w), 7 * i, np.uint8) for i, (w, h) in enumerate(sizes)]
    n = 300                                                                           # two blocks of the gather
    img = ((7 * np.arange(n) + 3) % len(sizes)).astype(np.int32)                      # not the identity, every image used
    idx = [L - 1] + [int(i) for i in rng.permutation(L - 1)[:K - 1]]                  # the last landmark first: not ascending
    assert len(idx) == K == len(set(idx)) and (K < 2 or idx[0] > idx[1])
    x = rng.uniform(-50.0, 700.0, (n, 2 * L)).astype(np.float32)
    focal = 950.5
    c = Context(0)
    try:
        c.set_model_geometry(L, re, le, [HoGParam(1, 5, 6, 4, 0.6)])
        c.upload_images(images)
        c.set_sample_image_index(img)
        c.set_x(x)
        c.pose_set_model(np.zeros((K, 3), np.float32), focal)
        c.pose_templates_from_landmarks(idx, focal)
        c.pose_set_x(C.start(n))
        hw = np.array([sizes[i][0] for i in img], np.float32)[:, None] / np.float32(2.0)
        hh = np.array([sizes[i][1] for i in img], np.float32)[:, None] / np.float32(2.0)
        host = np.concatenate([(x[:, idx] - hw) / np.float32(focal), (x[:, [L + i for i in idx]] - hh) / np.float32(focal)], 1)
        assert host.dtype == np.float32 and np.array_equal(-c.pose_features(), host)
        assert code(c.pose_templates_from_landmarks, idx[:-1] + [L], focal) == -1    # an index past the landmark set
        assert code(c.pose_templates_from_landmarks, idx[:-1] + [-1], focal) == -1
        assert np.array_equal(-c.pose_features(), host)                               # a refused gather leaves the templates alone
    finally:
        c.close()
