"""Landmark sets of every size the C-ABI takes (2L <= 144), for the tests that run detect, the tracker, the upright path and the warp
at landmark counts other than RCR-22's: the kernels behind them are shaped by L (column tiles of 16 outputs, partial sums in batches
of 24 landmarks, rows strided over 64 lanes), and a model of 5, 30 or 72 points must meet the same code as the benchmark's.

  positions(L)      which of the 68 ibug landmarks a set of L holds (L <= 68), ascending, the four eye ids always among them and
                    landmark 68 the last
  landmark_set(L)   (ids or None, right eye indices, left eye indices)
  rows(x68, L)      N x 136 rows [x.., y..] of the 68 ibug landmarks -> N x 2L rows of the set
  mean(L)           the set's mean shape in unit-box coordinates

A set of 2 cannot hold the four eye ids: it is the two outer eye corners, one per eye.  For L = 69 ... 72 there are no ids: the set
is the 68 landmarks followed by copies of four of them, each moved by a few pixels (rows) or by the same share of the box (mean);
such a model goes through ``Context`` directly.
"""
import numpy as np

from superviseddescent_amd import ibug

EYES = [ibug.IBUG68_IDS.index(i) for i in ibug.RIGHT_EYE_IDS + ibug.LEFT_EYE_IDS]       # 36, 39, 42, 45
COPIED = [30, 8, 27, 57]                    # nose tip, chin, nose bridge, lower lip: the landmarks L = 69 ... 72 repeat
COPY_STEP_PX = (4.0, -3.0)                  # copy k lies (k + 1) x this beside its original, in pixels ...
COPY_STEP_UNIT = (0.025, -0.01875)          # ... or in unit-box coordinates (the same at a box of 160 pixels)


def positions(L):
    if L == 2:
        return [EYES[0], EYES[2]]
    if not 4 <= L <= 68:
        raise ValueError("sets of 2 or 4 ... 68 landmarks are subsets of the 68 ibug ids")
    if L == 4:
        return list(EYES)
    others = [p for p in range(68) if p not in EYES]
    return sorted(EYES + others[:L - 5] + [67])      # (the last landmark of a set is never an eye's)


def landmark_set(L):
    """(ids, right eye indices, left eye indices); ids is None for L > 68"""
    if L > 68:
        ids = ibug.IBUG68_IDS
        re, le = ibug.eye_indices(ids)
        return None, re, le
    pos = positions(L)
    ids = [ibug.IBUG68_IDS[p] for p in pos]
    if L == 2:
        return ids, [0], [1]
    re, le = ibug.eye_indices(ids)
    return ids, re, le


def _select(v68, L, step):
    v68 = np.atleast_2d(np.asarray(v68, np.float32))
    pos = positions(min(L, 68))
    x, y = v68[:, pos], v68[:, [68 + p for p in pos]]
    if L > 68:
        k = np.arange(1, L - 68 + 1, dtype=np.float32)
        x = np.concatenate([x, v68[:, COPIED[:L - 68]] + np.float32(step[0]) * k], 1)
        y = np.concatenate([y, v68[:, [68 + p for p in COPIED[:L - 68]]] + np.float32(step[1]) * k], 1)
    return np.ascontiguousarray(np.concatenate([x, y], 1), np.float32)


def rows(x68, L):
    return _select(x68, L, COPY_STEP_PX)


def mean(L):
    return _select(ibug.MEAN_IBUG_LFPW_68, L, COPY_STEP_UNIT)[0]
