"""Time of the piecewise-affine face warp (Context.warp_crops_tensor, the call behind detection_model.warped_crops_tensor; csrc/sdm_warp.hip)
beside the similarity crop (Context.align_crops_tensor, plain bilinear) on the same rows and frames: float16 N x 3 x 112 x 112 RGB with
mean / std from BGR device frames used in place, the RCR-22 template with its Delaunay mesh, at N = 1, 256 and 4 096 rows.
Host clock, 1 000 calls (300 at N = 4 096) behind 5 warm-up calls, p50, each call ended by a synchronise; the two routes alternate in
blocks of 50 calls, so that both see the same machine.  One run gives everything: before it opens the device itself the script starts
`rocprofv3 --kernel-trace --stats -- python <this file> --quick` as a child (N = 4 096, 200 calls of each route) and copies the warp and
align kernels' rows of its statistics into the result.  A host alternative (landmarks to the host, one affine per triangle, an image
library's warp) is not measured: there is no such library beside this one.  Writes profiles/warp_timing.json (or --out).
  --quick: the child's run; prints only.   --no-profile: skip the child."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import Context, HoGParam, alignment_template, delaunay, ibug, synth  # noqa: E402

IDS = ibug.RCR22_IDS
L = len(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
SIZE = 112
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def stats(ts):
    a = np.asarray(ts) * 1e3
    return {"calls": len(ts), "p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "min_ms": float(a.min()),
            "mean_ms": float(a.mean())}


def timed_pair(fa, fb, calls, torch, block=50):
    """fa and fb in alternating blocks; 5 warm-up calls of each first"""
    ta, tb = [], []
    for fn in (fa, fb):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    done = 0
    while done < calls:
        for fn, ts in ((fa, ta), (fb, tb)):
            for _ in range(min(block, calls - done)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        done += block
    return stats(ta), stats(tb)


def run(ctx, n, calls, bgr, gt, torch):
    idx = np.arange(n) % len(bgr)
    lm = np.arange(L)
    mean = ibug.select_mean(IDS)
    tmpl_warp = alignment_template(mean, lm, SIZE, SIZE, 0.1)
    tmpl_crop = alignment_template(mean, lm, SIZE, SIZE, 0.2)
    tri = delaunay(tmpl_warp)
    x = gt[idx] + np.random.default_rng(n).normal(0, 2, (n, 2 * L)).astype(np.float32)
    out_w = torch.empty((n, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    out_c = torch.empty((n, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    ctx.set_frames_device(bgr)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    ctx.align_set_source_frames(bgr)
    ctx.warp_set_mesh(lm, tmpl_warp, tri, SIZE, SIZE)
    labelled = float((ctx.warp_labels() != 255).mean())
    _, _, flags = ctx.warp_crops_tensor(out=out_w, mean=MEAN, std=STD)
    warp, crop = timed_pair(lambda: ctx.warp_crops_tensor(out=out_w, mean=MEAN, std=STD),
                            lambda: ctx.align_crops_tensor(lm, tmpl_crop, SIZE, SIZE, out=out_c, mean=MEAN, std=STD), calls, torch)
    ctx.align_set_source_frames(None)
    return {"warped_crops_tensor": warp, "aligned_crops_tensor_bilinear": crop, "ratio_warp_over_crop_p50": warp["p50_ms"] / crop["p50_ms"],
            "triangles": int(len(tri)), "labelled_share_of_crop": labelled, "rows_flagged": int((flags != 0).sum())}


def kernel_rows(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if "warp_" in r.get("Name", "") or "align" in r.get("Name", ""):
                    rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.json"))
    a = ap.parse_args()
    profile = None
    if not a.quick and not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable,
                                os.path.abspath(__file__), "--quick"], capture_output=True, text=True, timeout=600)
            profile = {"returncode": p.returncode, "kernels": kernel_rows(d)}
            if p.returncode:
                profile["stderr_tail"] = p.stderr[-2000:]
    import torch
    gray, _, gt68 = synth.make_faces(64, seed=84)
    gt = np.ascontiguousarray(gt68[:, SEL], np.float32)
    rng = np.random.default_rng(85)
    colour = rng.integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    colour[..., 1] = gray
    bgr = [torch.from_numpy(c).cuda() for c in colour]                       # 64 separate allocations, used in place
    ctx = Context(0)
    ctx.set_model_geometry(L, *ibug.eye_indices(IDS), [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS])
    sizes = [(4096, 200)] if a.quick else [(1, 1000), (256, 1000), (4096, 300)]
    res = {"crop": f"{SIZE} x {SIZE}", "tensor": "float16 N x 3 x H x W, RGB, mean / std", "landmarks": f"RCR-22, all {L}",
           "mesh": "Delaunay triangulation of alignment_template(mean, margin 0.1)", "source": "64 BGR device frames, used in place",
           "unit": "ms per call, host clock, synchronised; the two routes alternate in blocks of 50 calls",
           "host_alternative": "not measured", "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n, calls in sizes:
        res["sizes"][str(n)] = run(ctx, n, calls, bgr, gt, torch)
        print(n, json.dumps(res["sizes"][str(n)]), flush=True)
    ctx.close()
    if profile is not None:
        res["rocprofv3_kernel_stats_N4096"] = profile
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
