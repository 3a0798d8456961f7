"""The one-load row loop of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, "row carry"): where the patch is enlarged, a
pixel row loads and filters only the UPPER of its two source rows and takes the lower one from what the previous pixel row holds.
Which half-widths h qualify is decided per (level, h) from cv::resize's vertical taps when the geometry is set.

CPU part: the taps restated in tests/hog_taps_ref.py reproduce the oracle's cv::resize bit for bit (so they ARE the oracle's taps),
and from them every h with 2h <= S of the shipped levels is one-load eligible; the exact-2x reduction never is.

GPU part.  (1) The table the library built on the device (read back with sdm_debug_hog_taps), all 128 half-widths of the four
shipped levels: its taps are the restated ones, its eligibility flag is one_load_eligible() and its carry masks are the expected
ones; the cells launch of levels 1-3 is an instance that holds the one-load loop.  (2) Landmark rows scaled so that h takes every
integer from 1 to S (2h = 2S) at each shipped level, with patches hanging off every image border and wholly outside the image,
in SDM_HOG_COLUMNS mode with the raw-cells launch asserted to be the one in use.  Patch indices are the oracle's.  The float results
of the packed kernel were never the oracle's bits (the separable column sums of its mode), so they are held to the packed mode's
standing bound against the oracle (pixel_kernel_cases.PACKED_MAX_ABS, PACKED_REL_L2) and to BIT IDENTITY
between the one-load and the two-load loop (option hog_two_load) -- feature rows from the raw cells, the landmark update of
sdm_detect_level, and the landmarks bench.py dumps for its own batch.  That bit comparison is the test of the new loop's arithmetic.
The resized ROI bytes of the debug read-back are compared with the oracle as well, but sdm_debug_patch runs a kernel of its own:
it pins the inputs of the sweep (geometry, borders), not the row carry."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hog_taps_ref import expected_table, one_load_eligible, resize_taps, resize_with_taps
from oracle import sdm_oracle as orc
from pixel_kernel_cases import (L22, LE22, O_SHIPPED, PACKED_MAX_ABS, PACKED_REL_L2, RE22, SHIPPED, SIZES, bits, options, scaled_rows,
                                smooth_faces)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- CPU: the restated taps (tests/hog_taps_ref.py)
@pytest.mark.parametrize("S", SIZES)
def test_restated_taps_are_the_oracles(built, S):
    rng = np.random.default_rng(S)
    for h in range(1, S):
        taps = resize_taps(S, h)
        src = rng.integers(0, 256, (2 * h, 2 * h)).astype(np.uint8)
        assert np.array_equal(resize_with_taps(src, S, taps), orc.resize_u8_linear(src, S, S)), h
        # one bright source row at a time: the resized rows it reaches are the rows whose (non-zero-weight) taps name it
        _, c0, c1, r0, r1 = taps
        for r in range(2 * h):
            probe = np.zeros((2 * h, 2 * h), np.uint8)
            probe[r] = 255
            lit = orc.resize_u8_linear(probe, S, S).any(axis=1)
            named = ((r0 == r) & (c0 >= 64)) | ((r1 == r) & (c1 >= 64))        # weights under 64 / 2048 of 255 can round to 0
            assert not (named & ~lit).any(), (h, r)
            assert not (lit & ~((r0 == r) | (r1 == r))).any(), (h, r)


@pytest.mark.parametrize("S", SIZES)
def test_enlarged_patches_are_one_load_eligible(built, S):
    for h in range(1, S + 1):
        if 2 * h <= S:
            assert one_load_eligible(S, h), h
    assert not one_load_eligible(S, S)                        # 2h = 2S: the box average has no taps to carry
    # beyond 2h = S the source step exceeds one row: some resized row skips a source row
    assert not any(one_load_eligible(S, h) for h in range(S // 2 + 2, S))


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_the_librarys_table_is_the_oracles_eligibility(gpu_ctx, options):
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    for level, S in enumerate(SIZES):
        table, info = gpu_ctx.debug_hog_taps(level)
        assert info["cells_launch"] and not info["two_load_option"]
        assert info["one_load_instance"] == (level >= 1), level          # level 0 is compiled without the loop (profiles/hog_row_carry.txt)
        eligible = []
        for h in range(128):
            s0, c0, c1, r0, r1, mask, el = expected_table(S, h)
            t = table[h, :S].astype(np.int64)
            assert np.array_equal(t[:, 0], s0) and np.array_equal(t[:, 1], (c0 & 0xffff) | (c1 << 16)), (level, h)
            assert np.array_equal(t[:, 2], r0) and np.array_equal(t[:, 3], r1), (level, h)
            if mask is None:
                assert np.array_equal(t[:, 4], np.full(S, 1024 << 12)) and np.array_equal(t[:, 5], np.full(S, 1024 << 12)), (level, h)
            else:
                assert np.array_equal(t[:, 4], c0 << 12) and np.array_equal(t[:, 5], c1 << 12), (level, h)
            assert (table[h, :, 7] == el).all(), (level, h)               # every coordinate's entry carries the wave-uniform flag
            if el:
                assert np.array_equal(t[:, 6], mask), (level, h)
                # what the one-load loop does with the masks reproduces the lower source row of every resized row
                held0, held1 = r0[0], r1[0]
                for y in range(1, S):
                    held0 = held1 if t[y, 6] else held0
                    held1 = r1[y]
                    assert held0 == r0[y], (level, h, y)
                eligible.append(h)
        assert eligible == [h for h in range(1, 128) if one_load_eligible(S, h)]
        assert set(range(1, S // 2 + 1)) <= set(eligible)
        print("level %d S %d: one-load eligible half-widths 1..%d" % (level, S, eligible[-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_half_width_sweep(gpu_ctx, options, level):
    images, x0 = smooth_faces()
    x, hs = scaled_rows(x0, level)
    n = x.shape[0]
    idx = (np.arange(n) % images.shape[0]).astype(np.int32)
    S = SIZES[level]
    assert {S // 2, (S + 1) // 2, S // 2 + 1} <= set(hs.tolist())          # 2h = S - 1 / S / S + 1, whichever are even
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    gpu_ctx.upload_images(images)
    gpu_ctx.set_sample_image_index(idx)
    table, info = gpu_ctx.debug_hog_taps(level)
    assert info["cells_launch"]                               # the raw-cells launch (the kernel with the two loops) is what runs below
    assert info["one_load_instance"] == (level >= 1)
    n_one_load = int(sum(int(table[h, 0, 7]) for h in hs)) if info["one_load_instance"] else 0
    assert (n_one_load > 0) == (level >= 1)
    want, widx = orc.hog_features_batch(images, idx, x, RE22, LE22, O_SHIPPED[level], n_threads=os.cpu_count() or 1, want_idx=True)
    assert np.array_equal(widx[:, 0], hs)                                  # the sweep is the one intended
    options("hog_split_store", 1)                             # feature rows through the raw cells of the CELLS pixel kernel
    got = {}
    for two in (False, True):
        options("hog_two_load", int(two))
        assert gpu_ctx.debug_hog_taps(level)[1]["two_load_option"] == two
        gpu_ctx.set_x(x)
        got[two] = gpu_ctx.hog_features(level, fetch=True)
        assert np.array_equal(gpu_ctx.patch_indices(), widx)
    # the landmark update of the detect path (cells -> descriptor x regressor), both loops
    rng = np.random.default_rng(5)
    R = (rng.standard_normal((gpu_ctx.feature_dim(level), 2 * L22)) * 1e-3).astype(np.float32)
    gpu_ctx.set_regressor(level, R)
    upd = {}
    for two in (False, True):
        options("hog_two_load", int(two))
        gpu_ctx.set_x(x)
        gpu_ctx.detect_level(level)
        upd[two] = gpu_ctx.get_x()
    options("hog_split_store", 0)
    options("hog_two_load", 0)
    diff = np.abs(got[False] - want).max()
    rel = float(np.linalg.norm((got[False] - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
    print("level %d: %d rows (%d on the one-load loop), features against the oracle max abs %.3g rel L2 %.3g" % (level, n, n_one_load, diff, rel))
    assert np.array_equal(bits(got[False]), bits(got[True]))
    assert np.array_equal(bits(upd[False]), bits(upd[True]))
    assert diff <= PACKED_MAX_ABS and rel <= PACKED_REL_L2
    # resized ROI bytes through the debug read-back (a kernel of its own, see above): around 2h = S, a border row and the row outside the image
    gpu_ctx.set_x(x)
    picks = [S // 2 - 1, S // 2, S // 2 + 1, S - 1, n - 6, n - 1]
    for s in picks:
        h = int(hs[s])
        for lm in (0, 13):
            rsz, _, _, _ = gpu_ctx.debug_patch(level, s, lm, SHIPPED[level])
            cx, cy = orc.cv_round(x[s, lm]), orc.cv_round(x[s, lm + L22])
            roi = np.zeros((2 * h, 2 * h), np.uint8)
            ys, xs = np.mgrid[cy - h:cy + h, cx - h:cx + h]
            ok = (ys >= 0) & (ys < 256) & (xs >= 0) & (xs < 256)
            roi[ok] = images[idx[s]][ys[ok], xs[ok]]
            assert np.array_equal(rsz, orc.resize_u8_linear(roi, S, S)), (s, lm)


@pytest.mark.gpu
def test_both_loops_on_the_bench_batch(built, tmp_path):
    """bench.py's own batch (its seeds, its model): the dumped landmarks with and without the one-load loop, byte for byte."""
    out = {}
    for two in ("0", "1"):
        d = tmp_path / ("two_load_" + two)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "1024",
                            "--train-rows", "4000", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, SDM_HOG_TWO_LOAD=two))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[two] = np.load(d / "landmarks.npy")
    assert out["0"].shape == (1024, 2 * L22) and np.isfinite(out["0"]).all()
    assert out["0"].tobytes() == out["1"].tobytes()
