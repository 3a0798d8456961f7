#!/usr/bin/env python3
"""Instructions of ONE band fold of the lane-packed HOG kernel's detect instances, from compiled assembly (profiles/hog_fold_cost.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S \
        superviseddescent_amd/csrc/sdm_hog_packed.hip -o packed.s
    (the same source with `fold_band` returning at once in the detect instances -- `if (CELLS && F16F) return;` as its first line,
     HP_FOLD_ABL = 1 of scripts/experiments/hog_fold_ablations.patch -> nofold.s)
    python scripts/isa_fold_count.py packed.s nofold.s

The compiler schedules a fold's instructions among those of the pixel rows around it, so a fold has no borders in the listing.  It is
counted by DIFFERENCE: per detect instance (hog_packed_kernel<4, 5, CELL, true, true>), the instructions of the build minus those of
the build without folds, by class, over the number of fold sites (matrix instructions / 8).  The difference holds the pass's loads of
the fold weights (four 16-byte loads, once per pass, not per fold) -- listed as vector-memory beside the stores.  Classes as in
scripts/isa_pass_setup_count.py, the matrix instructions apart.  Static counts; the script counts, it asserts nothing."""
import collections
import re
import sys

from isa_pass_setup_count import classify, kernels


def histogram(path):
    out = {}
    for name, body in kernels(path).items():
        m = re.search(r"hog_packed_kernelILi4ELi5ELi(\d+)ELb1ELb1EEEv", name)
        if not m or m.group(1) == "0":
            continue
        ops = collections.Counter(op for _, op in body if op is not None)
        cls = collections.Counter()
        for op, n in ops.items():
            cls["matrix" if op.startswith("v_mfma") else classify(op)] += n
        out[int(m.group(1))] = (cls, ops)
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    full, bare = histogram(sys.argv[1]), histogram(sys.argv[2])
    for cell in sorted(full, reverse=True):
        cls, ops = full[cell]
        bcls, bops = bare[cell]
        sites = cls["matrix"] / 8.0 or bcls["matrix"] / 8.0 or 1.0      # (a build without matrix instructions: per instance)
        print("cell %2d  %d fold sites (%d matrix instructions), kernel %d instructions, without folds %d"
              % (cell, sites, cls["matrix"], sum(cls.values()), sum(bcls.values())))
        print("   per fold: " + "  ".join("%s %.1f" % (c, (cls[c] - bcls[c]) / sites)
                                          for c in ("vector", "matrix", "LDS", "vector-memory", "scalar", "waits")))
        diff = {op: ops[op] - bops[op] for op in set(ops) | set(bops) if op.startswith(("v_", "ds_")) and ops[op] != bops[op]}
        print("   by opcode, whole instance: " + ", ".join("%s %+d" % (op, d) for op, d in sorted(diff.items(), key=lambda t: -abs(t[1]))[:14]))


if __name__ == "__main__":
    main()
