"""Is the device code of a set of translation units the same code as at another revision?  For refactors of the pixel kernels:
    python scripts/isa_kernel_identity.py --base HEAD --base-src sdm_hog_fast.hip \\
        --src sdm_hog_fast.hip sdm_hog_packed.hip sdm_hog_plan.hip > profiles/hog_split_isa_identity.txt
Compiles the named files of superviseddescent_amd/csrc -- at revision --base (from git, into a temporary directory) and in the
working tree -- to gfx950 assembly with the Makefile's FLAGS plus --cuda-device-only -S, and compares by symbol:
  * the set of kernel symbols (mangled names),
  * the instruction text of every function (kernels and the device functions that were not inlined), after removing what depends
    only on the position in the file: comments, .file / .loc / .ident / .section lines, the function ordinal in local labels,
  * every kernel's .amdhsa_* descriptor block and its register / LDS / scratch entries in the metadata.
The base is compiled twice first: two compilations of the same source must compare equal, or the comparison means nothing.
--rename OLD=NEW (repeatable) pairs kernels whose symbol changed: a base kernel whose symbol contains OLD is compared with, and listed
under, the working tree's one kernel whose symbol contains NEW and carries the same integer template arguments.
Needs no GPU.  Exit status 0 = identical."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "superviseddescent_amd/csrc"
META_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")


def makefile_flags(csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"FLAGS\s*:=\s*(.*)", line)
        if m:
            return m.group(1).replace("$(ARCH)", "gfx950").split()
    raise SystemExit("no FLAGS in the Makefile")


def compile_asm(tree, names, out_dir, tag):
    csrc = os.path.join(tree, CSRC)
    text = []
    for n in names:
        out = os.path.join(out_dir, "%s_%s.s" % (tag, n))
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + makefile_flags(csrc) +
                              ["--cuda-device-only", "-S", os.path.join(csrc, n), "-o", out], stderr=subprocess.DEVNULL)
        text.append(open(out).read())
    return "\n".join(text)


def normalise(line):
    line = line.split(";", 1)[0].rstrip()
    if re.match(r"\s*\.(file|loc|ident|section)\b", line):
        return ""
    line = re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", line)
    return re.sub(r"\.Lfunc_(end|begin)\d+", r".Lfunc_\1", line)


def parse(asm):
    """-> (functions: name -> normalised text, descriptors: kernel -> .amdhsa block, metadata: kernel -> {key: value})"""
    funcs, desc, meta = {}, {}, {}
    # a kernel's descriptor block sits between its last instruction and its .Lfunc_end label: taken out first
    lines = []
    src = iter(asm.splitlines())
    for line in src:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            lines.append(line)
            continue
        block = []
        for line in src:
            if ".end_amdhsa_kernel" in line:
                break
            block.append(normalise(line).strip())
        desc[m.group(1)] = "\n".join(t for t in block if t)
    ftypes = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", asm, re.M))
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
        if m and m.group(1) in ftypes:
            j = next(k for k in range(i, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[k]))
            funcs[m.group(1)] = "\n".join(t for t in map(normalise, lines[i + 1:j]) if t.strip())
            i = j
        i += 1
    for block in re.split(r"^  - (?=\.)", asm, flags=re.M)[1:]:
        ent = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)\s*$", block, re.M))      # the kernel's own keys (arguments sit deeper)
        if ent.get("name") in desc:
            meta[ent["name"]] = {k: ent.get(k, "-") for k in META_KEYS}
    return funcs, desc, meta


def renamed(base, new, renames):
    """the base's (functions, descriptors, metadata) with every kernel symbol that --rename pairs with a kernel of the working tree replaced by it"""
    ints = lambda n: re.findall(r"Li(\d+)E", n)
    to = {}
    for r in renames:
        old, _, repl = r.partition("=")
        for n in base[1]:
            hits = [m for m in new[1] if old in n and repl in m and ints(m) == ints(n)]
            if len(hits) == 1:
                to[n] = hits[0]
    return tuple({to.get(n, n): v for n, v in part.items()} for part in base), to


def differences(a, b):
    out = []
    for what, x, y in zip(("function", "descriptor", "metadata"), a, b):
        for n in sorted(set(x) | set(y)):
            if n not in x or n not in y:
                out.append("%s %s only in the %s" % (what, n, "new tree" if n in y else "base"))
            elif x[n] != y[n]:
                out.append("%s %s differs" % (what, n))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--base", default="HEAD", help="git revision to compare against")
    ap.add_argument("--base-src", nargs="+", required=True, help="files of %s at the base revision" % CSRC)
    ap.add_argument("--src", nargs="+", required=True, help="files of %s in the working tree" % CSRC)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="pair kernels whose symbol changed")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        base_tree = os.path.join(d, "base")
        os.makedirs(base_tree)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", base_tree], stdin=tar.stdout)
        if tar.wait() != 0:
            raise SystemExit("git archive %s failed" % args.base)
        base1 = parse(compile_asm(base_tree, args.base_src, d, "base1"))
        base2 = parse(compile_asm(base_tree, args.base_src, d, "base2"))
        new = parse(compile_asm(ROOT, args.src, d, "new"))
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", args.base], text=True).strip()
    print("base %s: %s        working tree: %s" % (rev, " ".join(args.base_src), " ".join(args.src)))
    unstable = differences(base1, base2)
    base1, pairs = renamed(base1, new, args.rename)
    for old, to in sorted(pairs.items()):
        print("renamed: %s -> %s" % (old, to))
    print("base compiled twice: %s" % ("identical" if not unstable else "DIFFERENT -- the comparison is not stable"))
    diffs = differences(base1, new)
    funcs, desc, meta = new
    bfuncs, bdesc, bmeta = base1
    print("kernels: base %d, working tree %d (%d with private_segment_fixed_size 0, largest vgpr_count %d); other device functions: base %d, working tree %d"
          % (len(bdesc), len(desc), sum(1 for m in meta.values() if m["private_segment_fixed_size"] == "0"),
             max([int(m["vgpr_count"]) for m in meta.values()] or [0]), len(bfuncs) - len(bdesc), len(funcs) - len(desc)))
    print("\n%-9s %6s  %-12s %s" % ("text", "lines", "sha1", "symbol"))
    for n in sorted(set(funcs) | set(bfuncs)):
        t, bt = funcs.get(n), bfuncs.get(n)
        state = "same" if t == bt else ("new only" if bt is None else ("base only" if t is None else "DIFFERS"))
        print("%-9s %6d  %-12s %s%s" % (state, len((t or bt).splitlines()), hashlib.sha1((t or bt).encode()).hexdigest()[:12], n,
                                        "" if n in desc or n in bdesc else "   (device function)"))
    print("\nmetadata and descriptor (base -> working tree where they differ)")
    print("%-5s %-5s %-5s %-8s %-8s %-6s %-10s %s" % ("vgpr", "sgpr", "agpr", "scratch", "lds", "wg", "descriptor", "kernel"))
    for n in sorted(set(desc) | set(bdesc)):
        m, bm = meta.get(n), bmeta.get(n)
        cols = ["%s" % ((m or bm)[k] if m == bm or m is None or bm is None or m[k] == bm[k] else bm[k] + "->" + m[k]) for k in META_KEYS]
        print("%-5s %-5s %-5s %-8s %-8s %-6s %-10s %s" % (cols[0], cols[1], cols[2], cols[3], cols[4], cols[5],
                                                         "same" if desc.get(n) == bdesc.get(n) else "DIFFERS", n))
    print("\nresult: %s" % ("IDENTICAL: same kernel symbols, same instruction text, same descriptors and metadata" if not diffs and not unstable
                            else "NOT IDENTICAL"))
    for t in unstable:
        print("  base vs base: " + t)
    for t in diffs:
        print("  " + t)
    return 1 if diffs or unstable else 0


if __name__ == "__main__":
    sys.exit(main())
