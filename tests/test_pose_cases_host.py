"""The conditions the head-pose cases (tests/pose_cases.py) must meet for tests/test_gpu_pose_shapes.py to mean what it says, without
a GPU: every Gram instantiation and both cascade paths are reached, the launches fit their LDS limits, the row counts give the block
counts they are named for, every system the GPU module solves is well conditioned, and the float32 restatement of a level -- the
noise floor the GPU module's bounds are scaled by -- is itself within the project's bounds."""
import os
import re

import numpy as np
import pytest

import pose_cases as C
import pose_f64 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_table_restates_the_kernel_constants():
    src = open(os.path.join(ROOT, "superviseddescent_amd", "csrc", "sdm_pose.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (POSE_[A-Z_]+) = (\d+);", src)}
    assert const["POSE_THREADS"] == C.THREADS and const["POSE_GRAM_CHUNK"] == C.GRAM_CHUNK and const["POSE_GRAM_BLOCKS"] == C.GRAM_BLOCKS
    assert const["POSE_CHUNK_PTS"] == C.CHUNK_PTS and const["POSE_PROJ_ROWS"] == C.PROJ_ROWS
    launched = [int(v) for v in re.findall(r"kp <= (\d+)\) hipLaunchKernelGGL\(pose_gram_partial_kernel<\1>", src)]
    assert launched == C.GRAM_KP[:-1] and "pose_gram_partial_kernel<POSE_MAXP>" in src
    assert C.case(C.MAX_K).kp == C.GRAM_KP[-1]                         # POSE_MAXP: pairs per thread at K = 64
    hdr = open(os.path.join(ROOT, "superviseddescent_amd", "csrc", "sdm_kernels.h")).read()
    assert re.search(r"#define SDM_POSE_MAX_K\s+%d\b" % C.MAX_K, hdr) and re.search(r"#define SDM_POSE_MAX_LEVELS\s+%d\b" % C.MAX_LEVELS, hdr)
    for c in C.CASES:
        assert c.T == 2 * c.K + 6 and c.pairs == c.T * (c.T + 1) // 2 and (c.kp - 1) * C.THREADS < c.pairs <= c.kp * C.THREADS
        assert sum(c.chunks) == c.K and all(1 <= n <= C.CHUNK_PTS for n in c.chunks)


def test_every_gram_instantiation_has_a_K_on_each_side_of_its_thresholds():
    inst = {c.K: c.instantiation for c in C.CASES}
    assert sorted(set(inst.values())) == C.GRAM_KP
    # the thresholds themselves, from the pair count of every K the C-ABI takes
    steps = [K for K in range(1, C.MAX_K) if C.case(K).instantiation != C.case(K + 1).instantiation]
    assert steps == [12, 19, 28, 42]
    for K in steps:
        assert K in inst and K + 1 in inst
    for kp in C.GRAM_KP:                                               # the smallest and the largest K of every instantiation
        ks = [K for K in range(1, C.MAX_K + 1) if C.case(K).instantiation == kp]
        assert ks[0] in inst and ks[-1] in inst


def test_both_cascade_paths_have_a_whole_chunk_and_both_tails():
    for staged in (False, True):
        cs = [c for c in C.CASES if (c.K > C.CHUNK_PTS) == staged]
        tails = {c.chunks[-1] for c in cs}
        assert C.CHUNK_PTS in tails and 1 in tails and (15 in tails or C.CHUNK_PTS in tails), (staged, tails)
        assert all((len(c.chunks) > 1) == staged for c in cs)
    assert {len(c.chunks) for c in C.CASES} >= {1, 2, 3, 4}
    assert C.case(17).chunks == [16, 1] and C.case(33).chunks == [16, 16, 1] and C.case(63).chunks == [16, 16, 16, 15]


def test_lds_of_every_launch_fits():
    for K in C.KS + [10]:
        for levels in (1, 3, 4, C.MAX_LEVELS):
            assert C.lds_bytes_cascade(K, levels) <= C.CASCADE_LDS_LIMIT, (K, levels)
        assert C.lds_bytes_solve(K) <= C.SOLVE_LDS_LIMIT, K
    assert C.lds_bytes_cascade(64, 16) == 84736                        # "83 KiB at K = 64" (sdm_launch_pose_cascade)
    assert C.lds_bytes_solve(64) == 128 * 134 * 8                      # 134 KiB beside the 8 KiB of static scratch: below the CU's 160


def test_row_counts_give_the_block_counts_they_are_named_for():
    assert [C.gram_blocks(n) for n in C.N_GRAM] == [1, 1, 2, 3, 9, 512, 257] == [C.GRAM_BLOCKS_OF[n] for n in C.N_GRAM]
    assert [C.gram_rows(n) for n in C.N_GRAM] == [64, 64, 64, 64, 64, 64, 128]        # the step from 64 to 128 rows per block
    groups = [(b // C.REDUCE_GROUP, b % C.REDUCE_GROUP) for b in (C.gram_blocks(n) for n in C.N_GRAM)]
    assert groups == [(0, 1), (0, 1), (0, 2), (0, 3), (1, 1), (64, 0), (32, 1)]      # tail only, eight plus one, no tail, 32 eights + 1
    assert C.N_GRAM[1] % C.GRAM_CHUNK == 0 and C.N_GRAM[2] % C.GRAM_CHUNK == 1       # a whole chunk, a chunk of one row
    blocks = lambda n, per: -(-n // per)                                # noqa: E731
    assert [blocks(n, C.THREADS) for n in C.N_ROWS] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert [blocks(n, C.PROJ_ROWS) for n in C.N_ROWS] == [1, 1, 1, 2, 4, 4, 5, 9]
    assert [n % C.PROJ_ROWS for n in C.N_ROWS] == [1, 63, 0, 1, 63, 0, 1, 1]
    assert blocks(C.N_DEFAULT, C.THREADS) == 2 and C.gram_blocks(C.N_DEFAULT) == 6
    # the rows the bit contracts run as batches of their own: other lanes, and one subset across the block edge
    assert 250 < C.THREADS < 270 and C.N_DEFAULT - 300 != 300 % C.THREADS


def trained_cases():
    """(K, N, regulariser) of every system tests/test_gpu_pose_shapes.py trains"""
    out = [(K, C.N_DEFAULT, reg) for K in C.KS for reg in C.REGULARISERS]
    out += [(K, n, C.REGULARISERS[0]) for K in (13, 43) for n in C.N_GRAM] + [(64, 32769, C.REGULARISERS[0])]
    return out


def test_every_trained_system_is_well_conditioned_at_level_0():
    worst = 0.0
    for K, n, (reg_type, param, last) in trained_cases():
        pts, xs = C.points(K), C.poses(n, K)
        A = P.project(C.start(n), pts) - C.templates(xs, pts)
        lam = P.reference_lambda(A.T @ A, n, reg_type, param)
        _, cond = C.solve64(A, C.start(n) - xs, lam, last)
        worst = max(worst, cond)
        assert cond < C.COND_CAP, (K, n, reg_type, param, last, cond)
    print(f"largest cond(G + Lambda) at level 0: {worst:.3g}")        # measured 6.1e4 (K = 64, Manual 1e-3, last row off)


def test_project32_is_within_the_feature_tolerance():
    for K in C.KS + [10]:
        pts = C.points(K)
        for x in (C.poses(C.N_DEFAULT, K), C.poses(max(C.N_ROWS), 1000 + K)):
            err = C.rel_err(C.project32(x, pts), P.project(x, pts)).max()
            assert err < C.FEAT_TOL, (K, err)                          # measured <= 3.1e-6 (K = 1), <= 1.4e-6 from K = 12 up


@pytest.mark.parametrize("reg", C.REGULARISERS, ids=lambda r: f"type{r[0]}-{r[1]:g}-{'all' if r[2] else 'notlast'}")
def test_level32_noise_floor(reg):
    """Three teacher-forced levels of the float32 restatement against the float64 level from the same x_k.  With the project's own
    regulariser (MatrixNorm 2.0, every row) it is within the project's bounds at every K: measured <= 5.2e-8 of ||x*|| and
    <= 3.4e-6 of the angles' norm (K = 1, level 1: two features, regressor entries up to 6 000), from K = 12 up <= 1.2e-8 / 7.7e-7.
    The other settings are allowed twice the project's bounds, so that four times this floor -- what the GPU module grants the device
    where it is the larger -- is never more than eight times them: measured <= 1.1e-7 / 7.2e-6 (K = 1, Manual, last row free, level 2),
    from K = 12 up <= 4.0e-8 / 2.7e-6.  The systems stay below the condition cap at every level."""
    slack = 1.0 if reg == C.REGULARISERS[0] else 2.0
    worst = (0.0, 0.0)
    for K in C.KS:
        pts, xs = C.points(K), C.poses(C.N_DEFAULT, K)
        y, xk = C.templates(xs, pts), C.start(C.N_DEFAULT)
        for level in range(3):
            R32, lam, x32 = C.level32(xk, xs, y, pts, *reg)
            _, lam64, x64 = C.level64(xk, xs, y, pts, *reg)
            _, cond = C.solve64(C.project32(xk, pts) - y, xk - xs, lam, reg[2])
            full, ang = C.x_errors(x32, x64, xs)
            worst = max(worst, (full, ang))
            assert R32.dtype == np.float32 and x32.dtype == np.float32
            assert cond < C.COND_CAP, (K, level, cond)
            assert full < slack * C.X_TOL and ang < slack * C.ANGLE_TOL, (K, level, full, ang)
            xk = x32
    print(f"level32 vs float64, worst of every K and level: {worst[0]:.3e} of ||x*||, {worst[1]:.3e} of the angles' norm")


def test_cascade32_and_random_regressors():
    """the 16 random levels of the levels test move no parameter by a degree per level (float64), and the float32 cascade follows"""
    K = C.MAX_K
    pts, xs = C.points(K), C.poses(C.N_DEFAULT, K)
    y = C.templates(xs, pts)
    Rs = C.random_regressors(K, C.MAX_LEVELS, y, pts, 7)
    x = C.start(C.N_DEFAULT).astype(np.float64)
    for R in Rs:
        nxt = C.cascade64(x, y, [R], pts)
        assert 0.0 < np.abs(nxt - x).max() < 1.0
        x = nxt
    full, ang = C.x_errors(C.cascade32(C.start(C.N_DEFAULT), y, Rs[:3], pts), C.cascade64(C.start(C.N_DEFAULT), y, Rs[:3], pts), xs)
    assert full < C.X_TOL and ang < C.ANGLE_TOL
