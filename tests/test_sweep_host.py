"""No-GPU checks of the regulariser sweep's host side: what SupervisedDescentOptimiser.train refuses before anything reaches a
device, RegulariserSweep's own checks, and the two new entry points in the binding table."""
import numpy as np
import pytest

from superviseddescent_amd import (HoGParam, HogTransform, LinearRegressor, ModelProjection, Regulariser, RegulariserSweep,
                                   SupervisedDescentOptimiser, _lib, ibug)


class NoDevice:
    """Stands in for a Context: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}) before the arguments were checked")


def hog():
    images = np.zeros((2, 64, 64), np.uint8)
    return HogTransform(images, [HoGParam(1, 3, 8, 4, 0.6)], ibug.RCR22_IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def optimiser(reg):
    return SupervisedDescentOptimiser([LinearRegressor(reg)], ctx=NoDevice())


X = np.zeros((4, 44), np.float32)


def test_a_sweep_without_holdout_is_refused():
    with pytest.raises(ValueError, match="holdout"):
        optimiser(RegulariserSweep(1, [0.5, 1.5])).train(X, X, None, hog())


@pytest.mark.parametrize("kw", [dict(allreduce=lambda *a: 0, world_size=2), dict(rccl=object()), dict(reduce_scatter=lambda *a: 0),
                                dict(rank=0, solve_collectives=(lambda *a: 0, lambda *a: 0))],
                         ids=["allreduce", "rccl", "reduce_scatter", "solve_collectives"])
def test_a_sweep_with_a_collective_is_refused(kw):
    with pytest.raises(ValueError, match="one device"):
        optimiser(RegulariserSweep(1, [0.5, 1.5])).train(X, X, None, hog(), holdout=1, **kw)
    with pytest.raises(ValueError, match="one device"):                      # a plain regulariser under holdout as well
        optimiser(Regulariser(1, 1.5)).train(X, X, None, hog(), holdout=1, **kw)


def test_pose_training_has_no_sweep():
    proj = ModelProjection(np.ones((3, 4), np.float32))
    x = np.zeros((4, 6), np.float32)
    with pytest.raises(ValueError, match="pose"):
        optimiser(RegulariserSweep(0, [1.0, 2.0])).train(x, x, np.zeros((4, 8), np.float32), proj, holdout=1)
    with pytest.raises(ValueError, match="pose"):
        optimiser(Regulariser(0, 1.0)).train(x, x, np.zeros((4, 8), np.float32), proj, holdout=1)


def test_holdout_must_split_the_rows():
    for h in (-1, 4, 5):
        with pytest.raises(ValueError):
            optimiser(RegulariserSweep(1, [0.5])).train(X, X, None, hog(), holdout=h)


def test_regulariser_sweep_is_a_regulariser():
    r = RegulariserSweep(Regulariser.RegularisationType.MatrixNorm, [0.5, 1.5, 4.0], regularise_last_row=False)
    assert isinstance(r, Regulariser) and r.params == [0.5, 1.5, 4.0]
    assert (r.regularisation_type, r.param, r.regularise_last_row) == (1, 0.5, False)
    for bad in ([], [1.0] * 33):
        with pytest.raises(ValueError):
            RegulariserSweep(0, bad)


def test_the_binding_table_knows_the_new_entry_points():
    assert "sdm_train_level_sweep" in _lib.EXPORTED and "sdm_sweep_get_regressor" in _lib.EXPORTED
