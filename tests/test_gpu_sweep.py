"""Regulariser sweep of one level on one Gram product (include/sdm.h: sdm_train_level_sweep): K candidates, chosen by the mean
normalised error on held-out rows.  The comparison path is always the existing code, never the sweep itself:
  * candidate k's regressor and lambda against hog_features + gram_rhs + solve on a second context that holds the fit rows alone,
    bit for bit (MatrixNorm / Manual, regularise_last_row on / off, targets beyond float16's range: the bf16 repeat inside the sweep);
  * the scores against set_regressor(R_k) + apply + normalised_errors on a context with all rows, to rtol 1e-9 (the float32 entries
    are the same; only the order of the float64 sum differs);
  * the installed state against set_regressor(R_best) + apply, bit for bit; ties, repeatability, failed candidates, refusals;
  * the cascade through SupervisedDescentOptimiser.train(..., holdout=h).
Geometry: 7 landmarks (the four eye corners among them), 3 x 3 cells of 16 bins: F = 7 * 144 + 1 = 1 009 = 8 tile columns + the
right-hand-side tile; 195 rows, 150 fitted, 45 held out (neither a multiple of 64: the split pass pads the rows)."""
import numpy as np
import pytest

from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, Regulariser, RegulariserSweep, SdmError,
                                   SupervisedDescentOptimiser, _lib, ibug, synth)

pytestmark = pytest.mark.gpu

IDS = ["31", "37", "40", "43", "46", "49", "55"]
RE, LE = ibug.eye_indices(IDS)
LEVELS = [HoGParam(1, 3, 12, 4, 0.9), HoGParam(1, 3, 8, 4, 0.6)]
N, N_FIT = 195, 150
MANUAL, MATRIX_NORM = 0, 1
PARAMS = {MATRIX_NORM: [0.5, 1.5, 6.0, 40.0], MANUAL: [0.25, 1.0, 8.0, 64.0]}


@pytest.fixture(scope="module")
def data():
    images, boxes, gt = synth.make_faces(39, seed=1901)
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=1902)          # 39 x 5 = 195 rows
    assert x0.shape[0] == N
    return images, x_star, x0, idx


def make_ctx(data, rows=N, x_star=None, images=None):
    imgs, xs, x0, idx = data
    ctx = Context(0)
    ctx.set_model_geometry(len(IDS), RE, LE, LEVELS)
    ctx.upload_images(imgs if images is None else images)
    ctx.set_sample_image_index(idx[:rows])
    ctx.set_x(x0[:rows])
    ctx.set_targets((xs if x_star is None else x_star)[:rows])
    return ctx


def reference_regressors(data, reg_type, params, last_row, x_star=None):
    """The existing path on a context that holds only the fit rows: [(R_k, lambda_k)]."""
    ctx = make_ctx(data, N_FIT, x_star)
    ctx.hog_features(0)
    out = []
    for p in params:
        ctx.gram_rhs(0)
        out.append(ctx.solve(0, reg_type, p, last_row, n_train_global=N_FIT))
    fallbacks = ctx.gram_fallbacks()
    ctx.close()
    return out, fallbacks


def reference_scores(data, Rs, x_star=None):
    """The existing path on a context with all rows, from the pre-level x: [(errors N x L, x after apply, regressor read back)]."""
    ctx = make_ctx(data, N, x_star)
    ctx.hog_features(0)
    out = []
    for R in Rs:
        ctx.set_x(data[2])
        ctx.set_regressor(0, R)
        ctx.apply(0)
        err, _ = ctx.normalised_errors(fetch=True)
        out.append((err, ctx.get_x(), ctx.get_regressor(0)))
    ctx.close()
    return out


_CASES = {}


def sweep_case(data, reg_type, last_row):
    """One sweep + its references per configuration, shared by the tests below (nothing in it is modified afterwards)."""
    key = (reg_type, last_row)
    if key not in _CASES:
        params = PARAMS[reg_type]
        ctx = make_ctx(data)
        rec = ctx.train_level_sweep(0, reg_type, params, last_row, N_FIT)
        Rs = [ctx.sweep_regressor(k) for k in range(len(params))]
        state = (ctx.get_x(), ctx.get_regressor(0))
        ctx.set_x(data[2])
        rec2 = ctx.train_level_sweep(0, reg_type, params, last_row, N_FIT)
        ctx.close()
        ref, _ = reference_regressors(data, reg_type, params, last_row)
        _CASES[key] = dict(rec=rec, rec2=rec2, Rs=Rs, state=state, ref=ref, scores=reference_scores(data, [r for r, _ in ref]))
    return _CASES[key]


CONFIGS = [(MATRIX_NORM, True), (MATRIX_NORM, False), (MANUAL, True), (MANUAL, False)]
CONFIG_IDS = ["matrixnorm-lastrow", "matrixnorm-nolastrow", "manual-lastrow", "manual-nolastrow"]


@pytest.mark.parametrize("reg_type,last_row", CONFIGS, ids=CONFIG_IDS)
def test_regressors_and_lambdas_are_those_of_the_fit_rows_alone(data, reg_type, last_row):
    case = sweep_case(data, reg_type, last_row)
    assert list(case["rec"]["status"]) == [0, 0, 0, 0]
    for k, (R, lam) in enumerate(case["ref"]):
        assert np.isfinite(R).all()
        assert np.array_equal(case["Rs"][k], R), k
        assert np.float32(lam).tobytes() == np.float32(case["rec"]["lambdas"][k]).tobytes(), k
    assert not np.array_equal(case["Rs"][0], case["Rs"][3])                   # (the candidates are different systems)


@pytest.mark.parametrize("reg_type,last_row", CONFIGS, ids=CONFIG_IDS)
def test_scores_are_the_means_of_the_normalised_errors(data, reg_type, last_row):
    case = sweep_case(data, reg_type, last_row)
    for k, (err, _, _) in enumerate(case["scores"]):
        hold = float(np.mean(err[N_FIT:].astype(np.float64)))
        fit = float(np.mean(err[:N_FIT].astype(np.float64)))
        print(k, case["rec"]["holdout_errors"][k], hold, case["rec"]["fit_errors"][k], fit)
        assert np.isclose(case["rec"]["holdout_errors"][k], hold, rtol=1e-9, atol=0.0)
        assert np.isclose(case["rec"]["fit_errors"][k], fit, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("reg_type,last_row", CONFIGS, ids=CONFIG_IDS)
def test_the_winner_is_installed_and_applied_and_two_runs_agree(data, reg_type, last_row):
    case = sweep_case(data, reg_type, last_row)
    rec = case["rec"]
    best = rec["best"]
    assert best == int(np.argmin(rec["holdout_errors"]))
    _, x_want, R_want = case["scores"][best]
    x_got, R_got = case["state"]
    assert np.array_equal(x_got, x_want) and np.array_equal(R_got, R_want)
    for name in ("holdout_errors", "fit_errors", "lambdas"):
        assert rec[name].tobytes() == case["rec2"][name].tobytes(), name
    assert case["rec2"]["best"] == best


def test_a_duplicated_best_value_returns_the_lower_index(data):
    case = sweep_case(data, MATRIX_NORM, True)
    p = PARAMS[MATRIX_NORM]
    best = case["rec"]["best"]
    order = [p[(best + 1) % 4], p[best], p[(best + 2) % 4], p[best]]          # the winner at 1 and at 3
    ctx = make_ctx(data)
    rec = ctx.train_level_sweep(0, MATRIX_NORM, order, True, N_FIT)
    ctx.close()
    assert rec["holdout_errors"][1] == rec["holdout_errors"][3] == case["rec"]["holdout_errors"][best]
    assert rec["best"] == 1


def test_held_out_rows_do_not_leak_into_the_fit(data):
    images, x_star, x0, idx = data
    case = sweep_case(data, MATRIX_NORM, True)
    held_images = np.unique(idx[N_FIT:])
    assert not np.isin(held_images, idx[:N_FIT]).any()                        # (rows of an image are consecutive: 30 + 9 images)
    images2 = np.array(images, copy=True)
    images2[held_images] = images2[held_images][:, ::-1, :]                    # other pixels under the held-out rows
    xs2 = x_star.copy()
    xs2[N_FIT:] += np.float32(3.0)                                            # other targets for them
    ctx = make_ctx(data, N, xs2, images2)
    rec = ctx.train_level_sweep(0, MATRIX_NORM, PARAMS[MATRIX_NORM], True, N_FIT)
    Rs = [ctx.sweep_regressor(k) for k in range(4)]
    ctx.close()
    for k in range(4):
        assert np.array_equal(Rs[k], case["Rs"][k]), k
    assert rec["lambdas"].tobytes() == case["rec"]["lambdas"].tobytes()
    assert rec["fit_errors"].tobytes() == case["rec"]["fit_errors"].tobytes()
    assert not np.array_equal(rec["holdout_errors"], case["rec"]["holdout_errors"])


def test_a_failed_candidate_is_skipped_and_does_not_poison_the_next(data):
    ref, _ = reference_regressors(data, MANUAL, [1.0], True)
    ctx = make_ctx(data)
    rec = ctx.train_level_sweep(0, MANUAL, [-1e9, 1.0], True, N_FIT)
    assert rec["status"][0] == _lib.SDM_ERR_NOT_SPD and rec["status"][1] == 0
    assert rec["holdout_errors"][0] == np.inf and rec["fit_errors"][0] == np.inf
    assert rec["best"] == 1
    assert np.array_equal(ctx.sweep_regressor(1), ref[0][0])
    assert np.float32(rec["lambdas"][1]).tobytes() == np.float32(ref[0][1]).tobytes()
    with pytest.raises(SdmError) as e:
        ctx.sweep_regressor(0)
    assert e.value.code == _lib.SDM_ERR_NOT_SPD
    ctx.close()


def test_when_every_candidate_fails_the_state_is_untouched(data):
    x0 = data[2]
    ctx = make_ctx(data)
    R_before = np.random.default_rng(5).standard_normal((ctx.feature_dim(0), 2 * len(IDS))).astype(np.float32) * np.float32(0.01)
    ctx.set_regressor(0, R_before)
    with pytest.raises(SdmError) as e:
        ctx.train_level_sweep(0, MANUAL, [-1e9], True, N_FIT)
    assert e.value.code == _lib.SDM_ERR_NOT_SPD
    assert np.array_equal(ctx.get_x(), x0)
    assert np.array_equal(ctx.get_regressor(0), R_before)
    with pytest.raises(SdmError):                                             # level 1 never had a regressor and still has none
        ctx.get_regressor(1)
    # the context afterwards: a plain train_level gives the bits of a fresh context
    ctx.train_level(0, MANUAL, 1.0, True)
    got = (ctx.get_x(), ctx.get_regressor(0))
    ctx.close()
    fresh = make_ctx(data)
    fresh.train_level(0, MANUAL, 1.0, True)
    want = (fresh.get_x(), fresh.get_regressor(0))
    fresh.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_bf16_repeat_runs_inside_the_sweep(data):
    """A training target beyond float16's range among the fit rows: the Gram launch repeats itself with three bf16 pieces."""
    xs = data[1].copy()
    xs[5, 3] += 2500.0
    params = PARAMS[MATRIX_NORM]
    ref, ref_fallbacks = reference_regressors(data, MATRIX_NORM, params, True, xs)
    assert ref_fallbacks == len(params)
    ctx = make_ctx(data, N, xs)
    rec = ctx.train_level_sweep(0, MATRIX_NORM, params, True, N_FIT)
    assert ctx.gram_fallbacks() == 1
    for k, (R, lam) in enumerate(ref):
        assert np.array_equal(ctx.sweep_regressor(k), R), k
        assert np.float32(lam).tobytes() == np.float32(rec["lambdas"][k]).tobytes()
    ctx.close()


def test_bad_arguments_and_collectives_are_refused(data):
    ctx = make_ctx(data)
    x0 = data[2]

    def code(fn):
        with pytest.raises(SdmError) as e:
            fn()
        return e.value.code
    assert code(lambda: ctx.train_level_sweep(0, MANUAL, [], True, N_FIT)) == _lib.SDM_ERR_INVALID                      # K = 0
    assert code(lambda: ctx.train_level_sweep(0, MANUAL, [1.0] * 33, True, N_FIT)) == _lib.SDM_ERR_INVALID              # K = 33
    assert code(lambda: ctx.train_level_sweep(0, MANUAL, [1.0], True, 0)) == _lib.SDM_ERR_INVALID
    assert code(lambda: ctx.train_level_sweep(0, MANUAL, [1.0], True, N)) == _lib.SDM_ERR_INVALID
    assert code(lambda: ctx.train_level_sweep(len(LEVELS), MANUAL, [1.0], True, N_FIT)) == _lib.SDM_ERR_INVALID
    assert code(lambda: ctx.train_level_sweep(-1, MANUAL, [1.0], True, N_FIT)) == _lib.SDM_ERR_INVALID
    assert code(lambda: ctx.sweep_regressor(0)) == _lib.SDM_ERR_INVALID                                                # no sweep yet
    ctx.set_allreduce(lambda ptr, count, stream: 0, 1)
    with pytest.raises(SdmError, match="collective") as e:
        ctx.train_level_sweep(0, MANUAL, [1.0], True, N_FIT)
    assert e.value.code == _lib.SDM_ERR_INVALID
    ctx.set_allreduce(None, 1)
    assert np.array_equal(ctx.get_x(), x0)                                    # nothing ran
    rec = ctx.train_level_sweep(0, MANUAL, [1.0], True, N_FIT)                # and the context is usable
    assert rec["best"] == 0 and rec["status"][0] == 0
    ctx.close()


def test_cascade_through_the_optimiser(data):
    images, x_star, x0, idx = data
    h = N - N_FIT
    regs = [LinearRegressor(RegulariserSweep(MATRIX_NORM, PARAMS[MATRIX_NORM], True)) for _ in LEVELS]
    sdo = SupervisedDescentOptimiser(regs)
    hog = HogTransform(images, LEVELS, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx)
    with pytest.raises(ValueError):
        sdo.train(x_star, x0, None, hog)                                      # a sweep needs held-out rows
    with pytest.raises(ValueError):
        sdo.train(x_star, x0, None, hog, holdout=h, allreduce=lambda *a: 0, world_size=2)
    x_train = sdo.train(x_star, x0, None, hog, holdout=h)
    ref_ctx = make_ctx(data)
    before = float(np.mean(ref_ctx.normalised_errors(fetch=True)[0][N_FIT:].astype(np.float64)))
    ref_ctx.close()
    for level, reg in enumerate(regs):
        rec = reg.sweep
        assert sorted(rec) == ["best", "fit_errors", "holdout_errors", "lambdas", "params", "status"]
        assert rec["best"] == int(np.argmin(rec["holdout_errors"]))
        assert reg.regulariser.param == PARAMS[MATRIX_NORM][rec["best"]]
        assert np.float32(reg.last_lambda).tobytes() == np.float32(rec["lambdas"][rec["best"]]).tobytes()
        assert np.array_equal(reg.x, sdo.ctx.get_regressor(level))
    print("held-out error", before, [float(r.sweep["holdout_errors"][r.sweep["best"]]) for r in regs])
    assert regs[1].sweep["holdout_errors"][regs[1].sweep["best"]] < before
    # detection: the same as an optimiser of plain regularisers holding the same arrays
    plain = []
    for reg in regs:
        r = LinearRegressor(Regulariser(MATRIX_NORM, reg.regulariser.param, True))
        r.x = np.array(reg.x, copy=True)
        plain.append(r)
    want = SupervisedDescentOptimiser(plain).test(x0, None, hog)
    got = sdo.test(x0, None, hog)
    assert np.array_equal(got, want)
    assert x_train.shape == got.shape and np.isfinite(x_train).all()
    # a plain Regulariser under holdout is a sweep of one candidate on the same split
    one = [LinearRegressor(Regulariser(MATRIX_NORM, regs[0].regulariser.param, True))]
    hog0 = HogTransform(images, LEVELS[:1], IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx)
    SupervisedDescentOptimiser(one).train(x_star, x0, None, hog0, holdout=h)
    assert np.array_equal(one[0].x, regs[0].x)
