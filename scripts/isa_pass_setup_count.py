#!/usr/bin/env python3
"""Instruction counts of the lane-packed HOG kernel's pass set-up, by class, from the compiled assembly
(profiles/hog_pass_setup.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S \
        superviseddescent_amd/csrc/sdm_hog_packed.hip -o packed.s
    python scripts/isa_pass_setup_count.py packed.s [--blocks] [--skip LABEL[,LABEL...]] [--kernel SUBSTRING]

Per detect instance (hog_packed_kernel<4, 5, CELL, true, true>) the instructions are split at the first image load
(buffer_load_ushort): everything above it is the SET-UP of a pass, everything from it on the ROW REGION (rows, band folds, tail).
Classes: vector (VALU, matrix cores included), f64 (VALU on doubles, conversions to and from them included), scalar (SALU and
branches), scalar-memory, LDS, vector-memory, waits (s_waitcnt, s_nop).  The counts are STATIC: a basic block counts once.
--blocks lists the set-up's basic blocks (label, size, last instruction) so that the blocks off the common path -- the
double-precision half-width, the run-time divisions, the per-wave taps -- can be named with --skip, which leaves them out of the
set-up's sums: what remains is the path a wave of the shipped levels executes.  The script classifies and counts; it asserts
nothing."""
import argparse
import collections
import re

CLASSES = ("vector", "f64", "scalar", "scalar-memory", "LDS", "vector-memory", "waits")


def classify(op):
    if op in ("s_waitcnt", "s_nop") or op.startswith("s_waitcnt"):
        return "waits"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar-memory"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector-memory"
    if op.startswith("v_"):
        return "f64" if "f64" in op else "vector"
    return None


def kernels(path):
    """{name: [(label or None, mnemonic), ...]} for every function of the file."""
    out, name = {}, None
    for line in open(path, errors="ignore"):
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            if not m.group(1).startswith(".L"):
                name = m.group(1)
                out[name] = []
            elif name is not None:
                out[name].append((m.group(1), None))
            continue
        if name is None or not s or s.startswith((".", ";", "//")):
            if s.startswith(".Lfunc_end"):
                name = None
            continue
        op = s.split()[0]
        if classify(op) is not None:
            out[name].append((None, op))
    return out


def blocks(body):
    res, label, cur = [], "(entry)", []
    for lab, op in body:
        if lab is not None:
            res.append((label, cur))
            label, cur = lab, []
        else:
            cur.append(op)
            if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
                res.append((label, cur))
                label, cur = label + "+", []
    res.append((label, cur))
    return [(l, b) for l, b in res if b]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="hog_packed_kernelILi4ELi5E", help="substring of the mangled kernel names to count")
    ap.add_argument("--all-forms", action="store_true", help="also the feature-row (training) instances, not only <.., true, true>")
    ap.add_argument("--blocks", action="store_true", help="list the basic blocks of the set-up")
    ap.add_argument("--skip", default="", help="comma-separated block labels left out of the set-up's sums")
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    for name, body in kernels(a.asm).items():
        if a.kernel not in name or (not a.all_forms and "ELb1ELb1EEEv" not in name):
            continue
        bl = blocks(body)
        first = next((i for i, (_, ops) in enumerate(bl) if any(o.startswith("buffer_load_ushort") for o in ops)), len(bl))
        setup, rows = collections.Counter(), collections.Counter()
        listing = []
        for i, (lab, ops) in enumerate(bl):
            if i < first:
                part = ops
            elif i == first:      # the block of the first image load: split at the load
                k = next(j for j, o in enumerate(ops) if o.startswith("buffer_load_ushort"))
                part = ops[:k]
                for o in ops[k:]:
                    rows[classify(o)] += 1
            else:
                for o in ops:
                    rows[classify(o)] += 1
                continue
            skipped = lab.rstrip("+") in skip or lab in skip
            marks = [w for w, pat in (("f64", "f64"), ("int-div", "v_rcp_iflag"), ("f32-div", "v_div_"), ("smem", "s_load"), ("vmem", "global_load"),
                                      ("atomic", "global_atomic"), ("lds", "ds_"), ("readlane", "v_readlane"))
                     if any(pat in o for o in part)]
            listing.append((lab, len(part), (part[-1] if part else "") + "  [" + " ".join(marks) + "]", skipped))
            if not skipped:
                for o in part:
                    setup[classify(o)] += 1
        m = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])", name)
        tag = "cell %s%s" % (m.group(3), "" if m.group(5) == "1" else " (feature rows)") if m else name
        print("%s  %s" % (tag, name[:80]))
        print("  %-12s %s   total" % ("", " ".join("%14s" % c for c in CLASSES)))
        for what, cnt in (("set-up", setup), ("row region", rows)):
            print("  %-12s %s   %5d" % (what, " ".join("%14d" % cnt[c] for c in CLASSES), sum(cnt.values())))
        if a.blocks:
            for lab, n, last, skipped in listing:
                print("    %-14s %4d  %-44s %s" % (lab, n, last, "(skipped)" if skipped else ""))
        print()


if __name__ == "__main__":
    main()
