"""The cell columns the two parts of a cut patch's raw cells hold (csrc/sdm_hog_plan.hip: plan_cut_columns; HogPlanHost::cut): host only.

A pass boundary of the packed pixel kernel cuts a patch between pixel columns, and a pixel column feeds its two nearest cell columns
only.  So the pass that holds the patch's column 0 (part 0) has all-zero fold weights for the cell columns right of the overlap, the
other pass (part 1) for those left of it: the plan says which columns a part holds (0 .. jA and jB .. C - 1), the pixel kernel stores
no other and the descriptor kernel loads no other.  Checked here against the plan's own weight table, for the four shipped cell
sizes and 22, 5 and 68 landmarks:

  * every skipped (part, cell column) of every cut landmark has all-zero weights -- else a non-zero cell would be dropped;
  * every kept one has a non-zero weight (nothing is moved for nothing);
  * jA + 1 >= jB: no column is left without an owner;
  * the "stores" bit of the pass's plan words (bit 24, the same for the four lanes of a matrix column) is the kept set;
  * an uncut landmark keeps all C columns in its one part."""
import numpy as np
import pytest

from superviseddescent_amd.engine import hog_plan

C = 5
CELLS = (11, 10, 8, 6)
COUNTS = (22, 5, 68)


def column_weights(plan, pt):
    """W[x][n] of pass pt from the matrix-core operand order: entry ks of lane l is W[4 ks + (l >> 4)][l & 15]"""
    W = np.zeros((64, 16), np.float32)
    for lane in range(64):
        for ks in range(16):
            W[4 * ks + (lane >> 4), lane & 15] = plan["wb"][pt][lane][ks]
    return W


def parts_of(plan):
    """{landmark: {part: (pass, segment)}} from pass_info: part 0 is the pass in which the segment starts its patch"""
    G, P, n_main, Pt = plan["G"], plan["P"], plan["n_main"], plan["Pt"]
    out = {}
    for pt in range(P + Pt):
        info = plan["pass_info"][pt]
        first_bits = (int(info[3]) >> 24) & 7
        for seg in range(3):
            slot = int(info[seg])
            if slot < 0:
                continue
            part = 0 if (first_bits >> seg) & 1 else 1
            lms = [g * G + slot for g in range(n_main)] if pt < P else [n_main * G + slot]
            for lm in lms:
                assert part not in out.setdefault(lm, {}), (lm, part)
                out[lm][part] = (pt, seg)
    return out


@pytest.mark.parametrize("L", COUNTS)
@pytest.mark.parametrize("cell", CELLS)
def test_skipped_columns_have_zero_weights_and_kept_ones_do_not(built, cell, L):
    plan = hog_plan(C, cell, 4, L)
    assert plan is not None
    cols = np.asarray(plan["columns"])
    assert cols.shape == (L, 3) and np.array_equal(cols[:, 0], np.asarray(plan["cut"]))
    parts = parts_of(plan)
    assert sorted(parts) == list(range(L))
    W = {pt: column_weights(plan, pt) for pt in range(plan["P"] + plan["Pt"])}
    stores = {pt: [int(d) >> 24 & 1 for d in plan["lane_tab"][pt]] for pt in W}
    for pt, s in stores.items():
        assert all(s[x] == s[x & 15] for x in range(64)), pt                  # one bit per matrix column, on its four lanes
    skipped = 0
    for lm in range(L):
        cut, jA, jB = (int(v) for v in cols[lm])
        assert sorted(parts[lm]) == ([0, 1] if cut else [0]), lm
        if not cut:
            assert (jA, jB) == (C - 1, C)
        else:
            assert 0 <= jB <= jA + 1 <= C, (lm, jA, jB)                       # every column has an owner
        for part, (pt, seg) in parts[lm].items():
            for j in range(C):
                kept = j <= jA if part == 0 else j >= jB
                nz = bool((W[pt][:, seg * C + j] != 0).any())
                assert kept == nz, (lm, part, j, kept, nz)
                assert stores[pt][seg * C + j] == int(kept), (lm, part, j)
                skipped += not kept
        assert not stores[pt][15]
    ncut = int(cols[:, 0].sum())
    print("cell %d, L %d: %d cut landmarks of %d, %d of their %d (part, column) pairs skipped" % (cell, L, ncut, L, skipped, 2 * C * ncut))
    assert skipped > 0 or ncut == 0


def test_the_shipped_levels_cut_where_the_record_says(built):
    """RCR-22: levels 0 - 2 cut patches and skip columns, level 3 (eleven groups of two whole patches) cuts none."""
    ncut = [int(np.asarray(hog_plan(C, cell, 4, 22)["columns"])[:, 0].sum()) for cell in CELLS]
    assert all(n > 0 for n in ncut[:3]) and ncut[3] == 0, ncut
