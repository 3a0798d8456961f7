"""cv::resize's vertical taps and what the detect path's pixel kernel (csrc/sdm_hog_packed.hip) derives from them, restated in numpy
for tests/test_gpu_row_carry.py and tests/test_gpu_pair_carry.py; no GPU, no torch.  The CPU tests of those two modules hold these
functions to the oracle (test_restated_taps_are_the_oracles: they reproduce its cv::resize bit for bit, so they ARE the oracle's
taps) and pin the structure they describe; the GPU tests compare the tables the library builds on the device with them.

  resize_taps(S, h)            per destination coordinate of the 2h -> S resize: source index, weights, the two source rows
  resize_with_taps(src, S, t)  orc_resize_u8_linear's arithmetic on those taps
  one_load_eligible(S, h)      row carry: every pixel row's lower source row is one of the previous row's two
  expected_table(S, h)         columns 2..7 of sdm_debug_hog_taps for one half-width
  source_rows(S, h)            the two source rows of every resized row as the device's table holds them
  pair_expected(S, h)          pair carry: (eligible, take-the-spare mask, spare source row per pair, orphan rows)
  eligible_range(S)            the pair-eligible half-widths below 128
"""
import numpy as np


# ---------------------------------------------------------------------------------------------- cv::resize's taps (row carry)
def resize_taps(S, h):
    """Per destination coordinate d of the 2h -> S bilinear 8-bit resize: unclamped source index, the two 11-bit weights, and the
    two source ROWS of the vertical pass (clipped to the patch).  None for the exact-2x reduction (box average, no taps)."""
    sw = 2 * h
    if sw == 2 * S:
        return None
    scale = 1.0 / (float(S) / float(sw))
    d = np.arange(S, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    f = (f - s0.astype(np.float32)).astype(np.float32)
    c0 = np.clip(np.rint((np.float32(1.0) - f) * np.float32(2048.0)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint(f * np.float32(2048.0)), -32768, 32767).astype(np.int64)
    return s0, c0, c1, np.clip(s0, 0, sw - 1), np.clip(s0 + 1, 0, sw - 1)


def resize_with_taps(src, S, taps):
    """orc_resize_u8_linear's arithmetic with the taps above: horizontal taps clamped in the table, vertical rows clipped."""
    sw = src.shape[1]
    s0, c0, c1, r0, r1 = taps
    sx, a0, a1 = s0.copy(), c0.copy(), c1.copy()
    lo, hi = sx < 0, sx >= sw - 1
    sx[lo], a0[lo], a1[lo] = 0, 2048, 0
    sx[hi], a0[hi], a1[hi] = sw - 1, 2048, 0
    sx1 = np.minimum(sx + 1, sw - 1)
    H = src.astype(np.int64)[:, sx] * a0 + src.astype(np.int64)[:, sx1] * a1          # [source row][dx]
    out = (((c0[:, None] * (H[r0] >> 4)) >> 16) + ((c1[:, None] * (H[r1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def one_load_eligible(S, h):
    taps = resize_taps(S, h)
    if taps is None:
        return False
    _, _, _, r0, r1 = taps
    return bool(np.all((r0[1:] == r0[:-1]) | (r0[1:] == r1[:-1])))


def expected_table(S, h):
    """Columns 2..7 of the library's table for one half-width: sy0, sy1, b0 << 12, b1 << 12, carry mask, eligible (rows d < S)."""
    if h == 0:                                   # the empty patch is given a 1-pixel source; never eligible
        scale = 1.0 / (float(S) / 1.0)
        f = ((np.arange(S) + 0.5) * scale - 0.5).astype(np.float32)
        s0 = np.floor(f).astype(np.int64)
        f = (f - s0.astype(np.float32)).astype(np.float32)
        c0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
        c1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
        r0, r1 = np.clip(s0, 0, 0), np.clip(s0 + 1, 0, 0)
        return s0, c0, c1, r0, r1, np.zeros(S, np.int64), 0
    taps = resize_taps(S, h)
    if taps is None:                             # exact 2x: rows 2d, 2d + 1 with weights 1024; the index and horizontal weights as computed
        sw = 2 * h
        f = ((np.arange(S) + 0.5) * 2.0 - 0.5).astype(np.float32)
        s0 = np.floor(f).astype(np.int64)
        f = (f - s0.astype(np.float32)).astype(np.float32)
        c0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
        c1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
        return s0, c0, c1, 2 * np.arange(S), 2 * np.arange(S) + 1, None, 0
    s0, c0, c1, r0, r1 = taps
    mask = np.zeros(S, np.int64)
    mask[1:] = np.where(r0[1:] == r1[:-1], -1, 0)
    return s0, c0, c1, r0, r1, mask, int(one_load_eligible(S, h))


# ---------------------------------------------------------------------------------------------- the pair loop's definition (pair carry)
def source_rows(S, h):
    """The two source rows of every resized row as the device's table holds them (columns 2 and 3 of sdm_debug_hog_taps)."""
    if h == 0:                                   # the empty patch is given a 1-pixel source
        return np.zeros(S, np.int64), np.zeros(S, np.int64)
    taps = resize_taps(S, h)
    if taps is None:                             # exact 2x: rows 2d, 2d + 1
        return 2 * np.arange(S), 2 * np.arange(S) + 1
    return taps[3], taps[4]


def pair_expected(S, h):
    """(eligible, take-the-spare mask [S], spare source row per pair [(S - 1) // 2] or -1, orphan rows) by the definition: every row
    d >= 1 a shift or an orphan row, at most one orphan per pair (2p + 1, 2p + 2), a last row without a partner a shift row."""
    r0, r1 = source_rows(S, h)
    shift, orphan = np.zeros(S, bool), np.zeros(S, bool)
    shift[1:] = r0[1:] == r1[:-1]
    orphan[1:] = r0[1:] == r1[:-1] + 1
    npairs = (S - 1) // 2
    first, second = orphan[1:2 * npairs:2], orphan[2:2 * npairs + 1:2]
    ok = bool((shift | orphan)[1:].all()) and not bool((first & second).any()) and bool(shift[2 * npairs + 1:].all())
    eligible = h >= 1 and 2 * h != 2 * S and ok
    spare = np.where(first, r0[1:2 * npairs:2], np.where(second, r0[2:2 * npairs + 1:2], -1))
    return eligible, np.where(orphan, -1, 0), spare, int(orphan.sum())


def eligible_range(S):
    return [h for h in range(128) if pair_expected(S, h)[0]]
