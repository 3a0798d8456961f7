"""Time of the filtered piecewise-affine warp (Context.warp_crops_tensor(filter="area"), csrc/sdm_warp_area.hip) against the unfiltered warp
(csrc/sdm_warp.hip) and against the rigid area kernel (Context.align_crops_tensor(filter="area"), csrc/sdm_align_area.hip): N = 4 096 rows,
float16 N x 3 x 112 x 112 RGB with mean / std, the RCR-22 template with its Delaunay mesh, everything resident on the device, from
  bgr    64 BGR frames of 256 x 256, used in place
  nv12   8 NV12 surfaces of 1920 x 1080 (Y plane and interleaved UV plane), used in place
as scripts/align_area_timing.py sets them up (+-20 degrees, crop centres around the frame centre), at crop -> source scales of
  0.95             every triangle at (1, 1): the unfiltered call ("plain", both trees), mode AREA ("area") and mode BILINEAR ("filter_bilinear");
                   "plain no copy" and "area no copy" are the C calls with every host pointer NULL -- the launches and the synchronise,
                   without the copy of the matrices, flags and samples
  1.95, 3.9, 7.8   "plain"; "area uniform": the landmarks are a similarity image of the template, one (Sx, Sy) pair per face; "area sheared":
                   the template sheared (+-0.3 along, +-0.2 across the axes) and bent per face first, so that the triangles of one face ask
                   for several pairs -- the gap between the two is the price of divergence; "rigid area": sdm_align_crops_tensor_filtered
                   on the same rows.
"warp faces plain" is the unfiltered warp as scripts/warp_timing.py runs it (64 BGR frames of synthetic faces, rows on their landmarks).
Host clock around a call that ends in the library's own synchronise; per case REPEATS repeats of CALLS calls behind 5 warm-up calls, the
median of every repeat, and over the repeats their median and their spread (max - min).  Sub-samples per second: the warp's
sum over rows and triangles of (labelled pixels of the triangle) Sx Sy, the rigid call's 112 112 (sum over rows of S S), over the median.

Every measurement runs in a child process of its own, one after the other.  --parent-tree DIR (a checkout of the parent commit with its
library built, inside the repository directory) adds children that time what the parent has -- the unfiltered warp and the rigid area call
--, alternating with this tree's: parent / this / parent / this / parent.  The result then holds, per shared case, the parent's median and
its own run-to-run spread (max - min over all of its repeats), this tree's median, and whether this tree stays within "parent's median +
parent's spread"; and for the scale 0.95 cases of the filtered call the same comparison with the parent's unfiltered figure.
Writes profiles/warp_area_timing.json (or --out)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIZE, REPEATS = 4096, 112, 5
SCALES = (0.95, 1.95, 3.9, 7.8)
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def timed(fn, calls):
    """5 warm-up calls, then REPEATS repeats of `calls` calls: the last result and the repeats' medians, median and spread in ms"""
    for _ in range(5):
        r = fn()
    medians = []
    for _ in range(REPEATS):
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()                                             # (ends in the library's stream synchronise)
            ts.append(time.perf_counter() - t0)
        medians.append(float(np.median(ts)) * 1e3)
    return r, {"repeat_medians_ms": medians, "median_ms": float(np.median(medians)), "spread_ms": max(medians) - min(medians),
               "calls_per_repeat": calls}


def child(tree):
    sys.path.insert(0, tree)
    import torch
    from superviseddescent_amd import Context, HoGParam, _lib, alignment_template, delaunay, ibug, synth
    filtered = "sdm_warp_crops_tensor_filtered" in _lib.EXPORTED
    ids = ibug.RCR22_IDS
    L = len(ids)
    re, le = ibug.eye_indices(ids)
    ctx = Context(0)
    ctx.set_model_geometry(L, re, le, [HoGParam(1, 5, 6, 4, 0.6)])
    rng = np.random.default_rng(7)
    lm = np.arange(L)
    tmpl = alignment_template(ibug.select_mean(ids), lm, SIZE, SIZE, 0.1)
    tri = delaunay(tmpl)
    bgr = torch.from_numpy(rng.integers(0, 256, (64, 256, 256, 3), dtype=np.uint8)).cuda()
    nv = torch.from_numpy(rng.integers(0, 256, (8, 1080 + 540, 1920), dtype=np.uint8)).cuda()
    sources = {"bgr": ([(bgr[i].data_ptr(), 256, 256, 256 * 3, "bgr") for i in range(64)], 256, 256),
               "nv12": ([(nv[i].data_ptr(), 1920, 1080, 1920, "nv12") for i in range(8)], 1920, 1080)}
    out = torch.empty((N, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    res = {"device": torch.cuda.get_device_name(0)}
    lib, spec, optr = ctx._lib, _lib.align_tensor_spec(mean=MEAN, std=STD), ctypes.c_void_p(out.data_ptr())
    mid = (SIZE - 1) / 2
    d = tmpl.astype(np.float64) - mid
    for name, (frames, W, H) in sources.items():
        ctx.set_frames_device(frames)
        ctx.set_sample_image_index(np.arange(N) % len(frames))
        ctx.align_set_source_frames(frames)
        ctx.warp_set_mesh(lm, tmpl, tri, SIZE, SIZE)
        area_px = np.bincount(ctx.warp_labels().reshape(-1), minlength=256)[:len(tri)].astype(np.float64)
        for s in SCALES:
            ang = np.deg2rad(rng.uniform(-20, 20, N))
            c, sn = s * np.cos(ang), s * np.sin(ang)
            centre = np.array([(W - 1) / 2, (H - 1) / 2]) + rng.uniform(-0.1, 0.1, (N, 2)) * (W, H)
            shear = np.stack([np.stack([1 + rng.uniform(-0.3, 0.3, N), rng.uniform(-0.2, 0.2, N)], -1),
                              np.stack([rng.uniform(-0.2, 0.2, N), 1 + rng.uniform(-0.3, 0.3, N)], -1)], 1)      # N x 2 x 2
            bend = 0.15 * rng.choice([-1, 1], (N, 2))
            shapes = {"uniform": np.broadcast_to(d, (N,) + d.shape)}
            q = np.einsum("nrc,kc->nkr", shear, d)
            shapes["sheared"] = q + bend[:, None, :] * np.stack([d[:, 1] ** 2 / SIZE, d[:, 0] ** 2 / SIZE], 1)[None]
            calls = 40 if s <= 2 else 15
            for shape, q in shapes.items():
                if shape == "sheared" and (s < 1.0 or not filtered):
                    continue
                x = np.zeros((N, 2 * L), np.float32)
                x[:, :L] = c[:, None] * q[..., 0] - sn[:, None] * q[..., 1] + centre[:, :1]
                x[:, L:] = sn[:, None] * q[..., 0] + c[:, None] * q[..., 1] + centre[:, 1:]
                ctx.set_x(x)
                key = "%s scale %g " % (name, s)
                if shape == "uniform":
                    res[key + "plain"] = timed(lambda: ctx.warp_crops_tensor(out=out, mean=MEAN, std=STD), calls)[1]
                    r, e = timed(lambda: ctx.align_crops_tensor(lm, tmpl, SIZE, SIZE, out=out, mean=MEAN, std=STD, filter="area"), calls)
                    S = np.asarray(r[3], np.float64)
                    e["S_min"], e["S_max"] = int(S.min()), int(S.max())
                    e["sub_samples_per_s"] = float((S ** 2).sum() * SIZE * SIZE / (e["median_ms"] * 1e-3))
                    res[key + "rigid area"] = e
                    if s < 1.0:                                  # the two launches and the synchronise alone: no table is copied home
                        res[key + "plain no copy"] = timed(lambda: lib.sdm_warp_crops_tensor(ctx._h, ctypes.byref(spec), optr, None, None), calls)[1]
                    if filtered and s < 1.0:
                        res[key + "filter_bilinear"] = timed(lambda: ctx.warp_crops_tensor(out=out, mean=MEAN, std=STD, filter="bilinear"), calls)[1]
                        f = _lib.align_filter("area")
                        res[key + "area no copy"] = timed(lambda: lib.sdm_warp_crops_tensor_filtered(ctx._h, ctypes.byref(spec), ctypes.byref(f), optr,
                                                                                                      None, None, None), calls)[1]
                if filtered:
                    r, e = timed(lambda: ctx.warp_crops_tensor(out=out, mean=MEAN, std=STD, filter="area"), calls)
                    smp = np.asarray(r[3], np.int64)
                    per_face = [len({(a, b) for a, b in row}) for row in smp[:256]]
                    e["S_min"], e["S_max"] = int(smp.min()), int(smp.max())
                    e["pairs_per_face_median"], e["pairs_per_face_max"] = float(np.median(per_face)), int(max(per_face))
                    e["sub_samples_per_s"] = float((smp.prod(-1) * area_px[None, :]).sum() / (e["median_ms"] * 1e-3))
                    res[key + ("area" if s < 1.0 else "area " + shape)] = e
        ctx.align_set_source_frames(None)
    # the unfiltered warp, as scripts/warp_timing.py runs it
    gray, _, gt68 = synth.make_faces(64, seed=84)
    sel = np.array([ibug.IBUG68_IDS.index(i) for i in ids] + [68 + ibug.IBUG68_IDS.index(i) for i in ids])
    colour = np.random.default_rng(85).integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    colour[..., 1] = gray
    faces = [torch.from_numpy(c).cuda() for c in colour]
    idx = np.arange(N) % len(faces)
    ctx.set_frames_device(faces)
    ctx.set_sample_image_index(idx)
    ctx.set_x(np.ascontiguousarray(gt68[:, sel], np.float32)[idx] + np.random.default_rng(N).normal(0, 2, (N, 2 * L)).astype(np.float32))
    ctx.align_set_source_frames(faces)
    ctx.warp_set_mesh(lm, tmpl, tri, SIZE, SIZE)
    res["warp faces plain"] = timed(lambda: ctx.warp_crops_tensor(out=out, mean=MEAN, std=STD), 40)[1]
    ctx.align_set_source_frames(None)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_area_timing.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    order = [("this", ROOT)]
    if a.parent_tree:
        p = os.path.abspath(a.parent_tree)
        order = [("parent", p), ("this", ROOT), ("parent", p), ("this", ROOT), ("parent", p)]
    runs = []
    for label, tree in order:
        env = dict(os.environ)
        env.pop("SDM_HIP_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True,
                           text=True, timeout=900, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the %s child failed with status %d" % (label, r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append({"tree": label, "result": json.loads(line[7:])})
        print(label, "done", flush=True)
    doc = {"rows": N, "crop": "112 x 112 x 3 float16 NCHW", "unit": "ms per call, host clock, the call ends in a stream synchronise",
           "repeats": REPEATS, "runs": runs}
    if a.parent_tree:
        doc["against_parent"] = cmp = {}
        pooled = lambda tree, case: [m for r in runs if r["tree"] == tree for m in r["result"][case]["repeat_medians_ms"]]

        def compare(case, yardstick):
            theirs, mine = pooled("parent", yardstick), pooled("this", case)
            e = {"parent_case": yardstick, "parent_median_ms": float(np.median(theirs)), "parent_spread_ms": max(theirs) - min(theirs),
                 "this_median_ms": float(np.median(mine)), "this_spread_ms": max(mine) - min(mine)}
            e["bound_ms"] = e["parent_median_ms"] + e["parent_spread_ms"]
            e["within_bound"] = e["this_median_ms"] <= e["bound_ms"]
            e["excess_percent"] = 100.0 * (e["this_median_ms"] / e["parent_median_ms"] - 1.0)
            cmp[case] = e
            print("%-32s parent %8.3f ms  spread %6.3f ms  this %8.3f ms  %+6.2f %%  %s" % (case, e["parent_median_ms"], e["parent_spread_ms"],
                  e["this_median_ms"], e["excess_percent"], "within" if e["within_bound"] else "EXCEEDS the bound"))

        for case in [k for k, v in runs[0]["result"].items() if isinstance(v, dict)]:
            compare(case, case)
        for case in [k for k in runs[1]["result"] if k.endswith(" scale 0.95 area") or k.endswith(" filter_bilinear")]:
            compare(case, case.rsplit(" ", 1)[0] + " plain")
        for case in [k for k in runs[1]["result"] if k.endswith(" area no copy")]:
            compare(case, case[:-len("area no copy")] + "plain no copy")
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    for run in runs:
        for k, v in run["result"].items():
            if isinstance(v, dict):
                print("%-7s %-32s median %8.3f ms  spread %6.3f ms%s" % (run["tree"], k, v["median_ms"], v["spread_ms"],
                      "  %.3g sub-samples/s" % v["sub_samples_per_s"] if "sub_samples_per_s" in v else ""))


if __name__ == "__main__":
    main()
