"""The pair loop of the detect path's pixel kernel (csrc/sdm_hog_packed.hip, "pair carry"): where the patch is reduced by less than
1.5 (S < 2h < 1.5 S), a pair of pixel rows loads three source rows instead of four -- the upper row of both and one spare -- and
every pixel row takes its lower source row from the previous row's upper one (a SHIFT row) or from the spare (an ORPHAN row: its
lower source row is the one after the previous row's upper one).  Which half-widths qualify, the per-row "take the spare" masks
and the per-pair spare rows are decided per (level, h) on the device from cv::resize's vertical taps.

CPU part: the structure restated in tests/hog_taps_ref.py from its resize_taps (which reproduce the oracle's cv::resize bit for bit):
for S = 55 the half-widths 27 .. 41 are pair eligible and no others (27, 2h = S - 1, has shift rows only), from 28 on they have
2h - 56 orphans, skip no source row and never hold two orphans in an aligned pair of pixel rows, in either pair phase; what the definition gives for S = 50 / 40 / 30.

GPU part.  (1) The table the library built on the device (sdm_debug_hog_pair_taps), all 128 half-widths of the four shipped
levels, equals the CPU expectation, and the table of sdm_debug_hog_taps is what it was.  (2) A half-width sweep at level 0 on NOISE
images (one wrong source row changes cells), once with stride = width and once with stride > width: patch indices are the oracle's,
feature rows are inside the standing bounds of the packed mode against the oracle (pixel_kernel_cases.PACKED_MAX_ABS, PACKED_REL_L2),
and the default is BIT IDENTICAL to option hog_two_load on the feature rows read through the raw cells, on the landmark update of
sdm_detect_level and on a four-level detect_batch of 192 faces."""
import os

import numpy as np
import pytest

from hog_taps_ref import eligible_range, expected_table, one_load_eligible, pair_expected, source_rows
from oracle import sdm_oracle as orc
from pixel_kernel_cases import (EXTRA_H, L22, LE22, O_SHIPPED, PACKED_MAX_ABS, PACKED_REL_L2, RE22, SHIPPED, SIZES, bits, noise, options,
                                pair_sweep_rows, smooth_faces)  # noqa: F401


# ---------------------------------------------------------------------------------------------- CPU: the definition (tests/hog_taps_ref.py)
def test_pair_structure_at_level_0(built):
    S = 55
    for h in range(1, 128):
        el, mask, spare, n_orphans = pair_expected(S, h)
        assert el == (27 <= h <= 41), h                      # 2h = 54 .. 82 (2h = 54: see below), 2h < 1.5 S
        r0, r1 = source_rows(S, h)
        if el:
            assert n_orphans == max(2 * h - 56, 0), h
            assert set(r0) | set(r1) == set(range(2 * h)), h                       # no source row is skipped
            if h >= 28:
                assert (r0[1:] != r0[:-1]).all() and (r1 == r0 + 1).all(), h       # no row repeats its lower row
            else:
                # 2h = S - 1, the slightest enlargement: 55 rows step through -1 .. 53 one source row at a time, and the only repeats
                # are the clamped first and last rows (r0 = r1), which are shift rows by the definition like every other row
                assert (r0[1:] == r1[:-1]).all() and r0[0] == r1[0] == 0 and r0[-1] == r1[-1] == 2 * h - 1, h
            orphan = mask != 0
            for phase in (0, 1):                                                   # pairs (1, 2), (3, 4) ... and (2, 3), (4, 5) ...
                assert not (orphan[1 + phase:S - 1:2] & orphan[2 + phase:S:2]).any(), (h, phase)
            # what the loop does with masks and spares reproduces the lower source row of every resized row
            held = r1[0]
            for y in range(1, S):
                sp = spare[(y - 1) // 2]
                assert (sp if mask[y] else held) == r0[y], (h, y)
                held = r1[y]
            assert (spare >= 0).sum() == n_orphans, h
        elif h <= 26:
            assert ((r0[1:] == r0[:-1]) & (r0[1:] != r1[:-1])).any(), h            # an enlargement repeats lower source rows
        elif h != S:
            orphan = mask != 0
            skipped = (r0[1:] > r1[:-1] + 1).any()
            assert skipped or (orphan[1:S - 1:2] & orphan[2:S:2]).any(), h         # from 2h = 84 on two orphans are adjacent
    # h = 28 (2h = S + 1) is also one-load eligible: no orphan, every spare unused
    assert one_load_eligible(S, 28) and pair_expected(S, 28)[3] == 0 and (pair_expected(S, 28)[2] == -1).all()
    # both positions of a pair hold orphans among the eligible half-widths
    masks = np.stack([pair_expected(S, h)[1] for h in range(27, 42)])
    assert (masks[:, 1::2] != 0).any() and (masks[:, 2::2] != 0).any()


def test_pair_eligibility_of_the_other_levels(built):
    """What the device is expected to report for S = 50 / 40 / 30 (no instance of those runs the loop): S <= 2h <= 1.5 S.  2h = S is
    the identity (shift rows only); beyond it there are 2h - S - 1 orphans, the even S leaving its last row S - 1 without a partner,
    which is a shift row at every one of these half-widths."""
    for S, lo, hi in ((50, 25, 37), (40, 20, 30), (30, 15, 22)):
        assert eligible_range(S) == list(range(lo, hi + 1)), S
        assert 2 * lo == S and 2 * hi <= 1.5 * S < 2 * (hi + 1)
        for h in range(lo, hi + 1):
            el, mask, spare, n_orphans = pair_expected(S, h)
            r0, r1 = source_rows(S, h)
            assert n_orphans == max(2 * h - S - 1, 0) and (spare >= 0).sum() == n_orphans and mask[S - 1] == 0, (S, h)
            assert set(r0) | set(r1) == set(range(2 * h)), (S, h)
        for h in list(range(1, lo)) + list(range(hi + 1, 128)):
            mask = pair_expected(S, h)[1]
            r0, r1 = source_rows(S, h)
            orphan = mask != 0
            neither = (r0[1:] != r1[:-1]) & ~orphan[1:]
            assert h == S or neither.any() or (orphan[1:S - 2:2] & orphan[2:S - 1:2]).any() or orphan[S - 1], (S, h)


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_the_librarys_pair_table(gpu_ctx, options):
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    for level, S in enumerate(SIZES):
        table, info = gpu_ctx.debug_hog_pair_taps(level)
        taps, tinfo = gpu_ctx.debug_hog_taps(level)
        assert not info["two_load_option"]
        print("level %d S %d: pair-loop instance %s" % (level, S, info["pair_instance"]))
        assert not (info["pair_instance"] and tinfo["one_load_instance"])
        assert info["pair_instance"] == (level == 0), level            # the loop ships in the cell-11 instance only (profiles/hog_pair_carry.txt)
        npairs = (S - 1) // 2
        eligible = []
        for h in range(128):
            el, mask, spare, n_orphans = pair_expected(S, h)
            t = table[h].astype(np.int64)
            assert np.array_equal(t[:S, 0], mask), (level, h)
            assert np.array_equal(t[:npairs, 1], spare) and (t[npairs:, 1] == -1).all(), (level, h)
            assert (t[:, 2] == int(el)).all() and (t[:, 3] == n_orphans).all(), (level, h)
            if el:
                eligible.append(h)
            # the existing table is what it was: sy0, sy1, the weights, the one-load mask and flag
            s0, c0, c1, r0, r1, m1, el1 = expected_table(S, h)
            u = taps[h, :S].astype(np.int64)
            assert np.array_equal(u[:, 0], s0) and np.array_equal(u[:, 1], (c0 & 0xffff) | (c1 << 16)), (level, h)
            assert np.array_equal(u[:, 2], r0) and np.array_equal(u[:, 3], r1) and (taps[h, :, 7] == el1).all(), (level, h)
            if el1:
                assert np.array_equal(u[:, 6], m1), (level, h)
        assert eligible == eligible_range(S)
        if level == 0:
            assert eligible == list(range(27, 42))


@pytest.fixture(scope="module")
def sweep():
    """The sweep and its oracle, computed once for both strides."""
    images = noise(24, seed=77)
    _, x0 = smooth_faces()
    x, hs = pair_sweep_rows(x0)
    idx = (np.arange(x.shape[0]) % images.shape[0]).astype(np.int32)
    want, widx = orc.hog_features_batch(images, idx, x, RE22, LE22, O_SHIPPED[0], n_threads=min(os.cpu_count() or 1, 16), want_idx=True)
    assert np.array_equal(widx[:, 0], hs)                                  # the sweep is the one intended
    assert set(range(1, 56)) <= set(hs.tolist()) and set(EXTRA_H) <= set(hs.tolist())
    return dict(images=images, x0=x0, x=x, hs=hs, idx=idx, want=want, widx=widx)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch", [256, 320])
def test_half_width_sweep_on_noise(gpu_ctx, options, sweep, pitch):
    import torch
    images, x, hs, idx, want, widx = (sweep[k] for k in ("images", "x", "hs", "idx", "want", "widx"))
    n = x.shape[0]
    gpu_ctx.set_model_geometry(L22, RE22, LE22, SHIPPED)
    if pitch == 256:
        gpu_ctx.upload_images(images)
    else:                                                     # the same images as views into wider rows of other noise
        big = torch.from_numpy(noise(images.shape[0], seed=78, w=pitch)).cuda()
        big[:, :, :256] = torch.from_numpy(images).cuda()
        gpu_ctx.set_frames_device([big[i, :, :256] for i in range(images.shape[0])])
    table, info = gpu_ctx.debug_hog_pair_taps(0)
    assert gpu_ctx.debug_hog_taps(0)[1]["cells_launch"]      # the raw-cells launch (the kernel with the loops) is what runs below
    assert info["pair_instance"] and not info["two_load_option"]
    n_pair = int(sum(int(table[h, 0, 2]) for h in hs))
    masks = np.stack([table[h, :55, 0] for h in hs if table[h, 0, 2]])
    assert (masks[:, 1::2] != 0).any() and (masks[:, 2::2] != 0).any()          # orphans in both positions of a pair
    got, upd, final = {}, {}, {}
    rng = np.random.default_rng(5)
    Rs = [(rng.standard_normal((gpu_ctx.feature_dim(lv), 2 * L22)) * 1e-3).astype(np.float32) for lv in range(4)]
    for lv in range(4):
        gpu_ctx.set_regressor(lv, Rs[lv])
    x192 = sweep["x0"][:192]
    idx192 = (np.arange(192) % images.shape[0]).astype(np.int32)
    for two in (False, True):
        options("hog_two_load", int(two))
        assert gpu_ctx.debug_hog_pair_taps(0)[1]["two_load_option"] == two
        # feature rows through the raw cells of the CELLS pixel kernel
        options("hog_split_store", 1)
        gpu_ctx.set_sample_image_index(idx)
        gpu_ctx.set_x(x)
        got[two] = gpu_ctx.hog_features(0, fetch=True)
        assert np.array_equal(gpu_ctx.patch_indices(), widx)
        options("hog_split_store", 0)
        # the landmark update of the detect path (cells -> descriptor x regressor)
        gpu_ctx.set_x(x)
        gpu_ctx.detect_level(0)
        upd[two] = gpu_ctx.get_x()
        # four levels on 192 faces
        gpu_ctx.set_sample_image_index(idx192)
        gpu_ctx.set_x(x192)
        final[two] = gpu_ctx.detect_batch()
    diff = np.abs(got[False] - want).max()
    rel = float(np.linalg.norm((got[False] - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
    print("pitch %d: %d rows (%d on the pair loop), features against the oracle max abs %.3g rel L2 %.3g" % (pitch, n, n_pair, diff, rel))
    assert n_pair > 0                                         # the pair loop is taken
    assert np.array_equal(bits(got[False]), bits(got[True]))
    assert np.array_equal(bits(upd[False]), bits(upd[True]))
    assert np.isfinite(final[False]).all() and np.array_equal(bits(final[False]), bits(final[True]))
    assert diff <= PACKED_MAX_ABS and rel <= PACKED_REL_L2
