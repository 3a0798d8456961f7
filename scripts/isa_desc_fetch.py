#!/usr/bin/env python3
"""Where the fused descriptor launch (desc_kernel<..., FUSED = true, ...>, csrc/sdm_desc.hip) waits for memory, from compiled assembly
(profiles/desc_fetch.txt).

    python scripts/isa_desc_fetch.py [SOURCE.hip | LISTING.s] [-D...]

A .hip file (default: superviseddescent_amd/csrc/sdm_desc.hip) is compiled with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S SOURCE -o LISTING
(include path: the default source's directory; further arguments go to the compiler), a .s file is read as it is.  Per fused instance:

  * registers, scratch and the compiler's occupancy figure;
  * the descriptor part (everything in front of the first s_barrier), one line per basic block: L = a global or buffer load, w(n) = s_waitcnt
    vmcnt(n), p = the eight ds_bpermute of the cell norms (the middle of a patch's arithmetic), s = the stores of the staged
    descriptor (its end), `-> label` = the block's branch.  The prefetch of the next patch is the L run in the block of the loop's
    head; a w between it and the s of the same pass is a wait in front of arithmetic that does not need the data yet;
  * behind each s_barrier the order of L, w and M (= v_mfma_*), run lengths as numbers, `|` at a label or a branch.

Loads, waits, matrix instructions and the two markers are counted, nothing else; static text, a block is listed once however often it
runs.  The script prints, it asserts nothing."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "superviseddescent_amd", "csrc", "sdm_desc.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]


def listing(path, extra):
    if path.endswith(".s"):
        return open(path, errors="ignore").read()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "desc.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-I", os.path.dirname(SOURCE)] + extra + [path, "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        return open(out, errors="ignore").read()


def instances(text):
    """[(mangled name, [lines of the body], {figure: value})] of the fused instances, in file order"""
    res, name, body, last, occ = [], None, [], None, {}
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r"^(_Z\w*desc_kernelI\w+):", s)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            m = re.match(r"^; Occupancy: (\d+)", s)
            if m and last is not None:
                occ[last], last = int(m.group(1)), None
            continue
        if s.startswith(".Lfunc_end"):
            res.append([name, body, {}])
            name, last = None, name
            continue
        body.append(s)
    figures = {}
    for m in re.finditer(r"\.name:\s+(_Z\w*desc_kernelI\w+)|\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", text):
        if m.group(1):
            cur = figures.setdefault(m.group(1), {})
        elif figures:
            cur[m.group(2)] = int(m.group(3))
    for r in res:
        r[2] = dict(figures.get(r[0], {}))
    return [r for r in res if "ELb1ELi" in r[0]], occ


def describe(name):
    m = re.search(r"desc_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb1ELi(\d+)ELi(\d+)E(?:Lb([01])E)?", name)
    o, c, v, fb, w, one = m.groups()
    return "%s orientations, %s, %s faces, %s" % (o, "UoCTTI" if v == "1" else "Dalal-Triggs", fb,
                                                  "one tile per wave" if one == "1" else "general")


def tokens(lines):
    """[(kind, text)] of what is counted: block borders, branches, loads, vmcnt waits, matrix instructions, markers, barriers"""
    out = []
    for s in lines:
        if not s or s.startswith((";", "//")):
            continue
        if re.match(r"^\.LBB\w+:", s):
            out.append(("label", s.split(":")[0]))
            continue
        if s.startswith("."):
            continue
        op = s.split()[0]
        if op.startswith(("global_load", "buffer_load")):
            out.append(("L", op))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                out.append(("w", m.group(1)))
        elif op.startswith("v_mfma"):
            out.append(("M", op))
        elif op == "ds_bpermute_b32":
            out.append(("p", op))
        elif op.startswith("ds_write") or op.startswith("ds_store"):
            out.append(("s", op))
        elif op == "s_barrier":
            out.append(("barrier", op))
        elif op.startswith(("s_cbranch", "s_branch")):
            out.append(("branch", s.split()[-1]))
        elif op == "s_endpgm":
            out.append(("branch", "end"))
    return out


def runs(seq):
    """L L w(0) M M M -> 'L2 w(0) M3'"""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        n = j - i
        if seq[i].startswith(("w", "|", "->")):
            out.extend([seq[i]] * n)
        else:
            out.append(seq[i] if n == 1 else "%s%d" % (seq[i], n))
        i = j
    return " ".join(out)


def report(name, body, fig, occ):
    print("%s\n  %s" % (describe(name), name))
    print("  VGPRs %s, scratch %s bytes per lane, spilled VGPRs %s, occupancy %s waves per SIMD"
          % (fig.get("vgpr_count", "?"), fig.get("private_segment_fixed_size", "?"), fig.get("vgpr_spill_count", "?"), occ.get(name, "?")))
    toks = tokens(body)
    parts, cur = [], []
    for t in toks:
        if t[0] == "barrier":
            parts.append(cur)
            cur = []
        else:
            cur.append(t)
    parts.append(cur)
    print("  descriptor part (in front of the first barrier), by basic block:")
    label, line = "(entry)", []

    def flush():
        if any(x[0] in "Lwps" for x in line if len(x[0]) == 1):
            print("    %-10s %s" % (label, runs([x[1] if x[0] == "br" else x[0] if x[0] != "w" else "w(%s)" % x[1] for x in line])))
    for kind, val in parts[0]:
        if kind == "label":
            flush()
            label, line = val, []
        elif kind == "branch":
            line.append(("br", "-> " + val))
        else:
            line.append((kind, val))
    flush()
    for i, part in enumerate(parts[1:], 1):
        seq = []
        for kind, val in part:
            if kind in ("L", "M"):
                seq.append(kind)
            elif kind == "w":
                seq.append("w(%s)" % val)
            elif kind in ("label", "branch") and seq and seq[-1] != "|":
                seq.append("|")
        while seq and seq[-1] == "|":
            seq.pop()
        print("  behind barrier %d: %s" % (i, runs(seq) or "-"))
    n = {k: sum(1 for t in toks if t[0] == k) for k in "LwM"}
    print("  whole instance: %d loads, %d vmcnt waits, %d matrix instructions\n" % (n["L"], n["w"], n["M"]))


def main():
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        raise SystemExit(__doc__)
    path = args[0] if args and not args[0].startswith("-") else SOURCE
    extra = [a for a in args if a.startswith("-")]
    inst, occ = instances(listing(path, extra))
    for name, body, fig in inst:
        report(name, body, fig, occ)


if __name__ == "__main__":
    main()
