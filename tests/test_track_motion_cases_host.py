"""The conditions of tests/track_motion_cases.py proved on the restatement alone (tests/track_motion_ref.py), without a device: the cases
tests/test_gpu_track_motion_edges.py runs really are the edges they are meant to be -- every search reach with the only zero of its
SAD table at the translation, every cell size with a shift taken and a shift refused, the ties, the extremes of the key, the min_gain
boundaries, the landmarks of the second turns, the all-zero window, ids in any order."""
import numpy as np
import pytest

import track_motion_cases as C
import track_motion_ref as R


def test_block_means_on_the_overlapped_part_equal_the_plain_sum():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    for X0, Y0, k, n in ((-7, -5, 3, 8), (10, 4, 1, 32), (40, 30, 5, 6), (-200, -100, 64, 4), (60, 2, 2, 4), (-3, 36, 4, 3), (0, 0, 53, 1)):
        region = np.zeros((n * k, n * k), np.int64)
        for y in range(n * k):
            for x in range(n * k):
                if 0 <= X0 + x < 53 and 0 <= Y0 + y < 37:
                    region[y, x] = img[Y0 + y, X0 + x]
        want = (region.reshape(n, k, n, k).sum(axis=(1, 3)) + k * k // 2) // (k * k)
        assert np.array_equal(R.block_means(img, X0, Y0, k, n), want), (X0, Y0, k, n)


@pytest.mark.parametrize("gain", [255, 0])
@pytest.mark.parametrize("S", [1, 5, 8, 16])
def test_reach(S, gain):
    info = C.case_reach(S, gain)
    assert info["pitch"] == {1: 40, 5: 48, 8: 52, 16: 68}[S] and info["steps"] >= 6
    print(info)


@pytest.mark.parametrize("S", [16, 8])
def test_cells(S):
    rows = [r for scale in C.CELLS for r in C.case_cells(S, scale)]
    C.cells_conditions(rows)
    print([(r[0], r[1], r[2], r[3]) for r in rows])


def test_ties_and_extremes():
    C.case_flat()
    C.case_ties()
    C.case_extremes()


@pytest.mark.parametrize("gain", [0, 1, 255])
def test_boundaries(gain):
    shifts = C.case_boundaries(gain)
    assert shifts.any()                                                # (an accepted non-zero offset is among the rows)


@pytest.mark.parametrize("mode", ["previous", "realign"])
@pytest.mark.parametrize("L", C.LENGTHS)
def test_lengths(L, mode):
    C.case_length(L, mode)


def test_slots_and_rows():
    C.case_slots()
    C.case_many()
