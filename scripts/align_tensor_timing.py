"""Time of the crops as network input tensors (Context.align_crops_tensor, the call behind detection_model.aligned_crops_tensor;
csrc/sdm_align_tensor.hip) against the route that existed before, to the same float16 N x 3 x 112 x 112 RGB tensor with mean / std, at
N = 1, 256 and 4 096 rows, everything resident on the device:
  (a) one call from BGR device frames used in place, and one from NV12 surfaces;
  (b) align_crops(source = a dense BGR stack, out = u8 N x H x W x 3), then permute, channel flip, .half(), subtract, divide in torch.
Host clock, 1 000 calls (300 at N = 4 096), p50, each call ended by a synchronise.  One run gives everything: before it opens the
device itself the script starts `rocprofv3 --kernel-trace --stats -- python <this file> --quick` as a child (N = 4 096, 200 calls of
each route) and copies the align kernels' rows of its statistics into the result.  Writes profiles/align_tensor_timing.json (or --out).
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
from superviseddescent_amd import Context, HoGParam, alignment_template, ibug, synth  # noqa: E402

IDS = ibug.RCR22_IDS
L = len(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
SIZE = 112
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def stats(ts):
    a = np.asarray(ts) * 1e3
    return {"calls": len(ts), "p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "min_ms": float(a.min()),
            "mean_ms": float(a.mean())}


def timed(fn, calls, torch):
    ts = []
    for k in range(calls + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= 5:
            ts.append(time.perf_counter() - t0)
    return stats(ts)


def run(ctx, n, calls, bgr, nv12, stack, gt, torch):
    idx = np.arange(n) % len(bgr)
    tmpl = alignment_template(ibug.select_mean(IDS), np.arange(L), SIZE, SIZE, 0.2)
    lm = np.arange(L)
    x = gt[idx] + np.random.default_rng(n).normal(0, 2, (n, 2 * L)).astype(np.float32)
    out16 = torch.empty((n, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    u8 = torch.empty((n, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    mean = torch.tensor(MEAN, dtype=torch.float16, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float16, device="cuda").view(1, 3, 1, 1)
    res = {}
    # (a) the new call, frames in place
    ctx.set_frames_device(bgr)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    ctx.align_set_source_frames(bgr)
    res["a_tensor_from_bgr_frames"] = timed(lambda: ctx.align_crops_tensor(lm, tmpl, SIZE, SIZE, out=out16, mean=MEAN, std=STD), calls, torch)
    ctx.set_frames_device(nv12)
    ctx.set_x(x)
    ctx.align_set_source_frames(nv12)
    res["a_tensor_from_nv12_surfaces"] = timed(lambda: ctx.align_crops_tensor(lm, tmpl, SIZE, SIZE, out=out16, mean=MEAN, std=STD), calls, torch)
    # (b) the route that existed before: u8 NHWC crops of a dense stack, then torch
    ctx.set_frames_device(bgr)
    ctx.set_x(x)
    ctx.align_set_source(stack)

    def old():
        ctx.align_crops(lm, tmpl, SIZE, SIZE, 3, out=u8)
        return (u8.permute(0, 3, 1, 2).flip(1).half() - mean) / std

    res["b_u8_crops_then_torch"] = timed(old, calls, torch)
    ctx.align_set_source(None)
    res["ratio_b_over_a_bgr_p50"] = res["b_u8_crops_then_torch"]["p50_ms"] / res["a_tensor_from_bgr_frames"]["p50_ms"]
    return res


def kernel_rows(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if "align" in r.get("Name", ""):
                    rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_tensor_timing.json"))
    ap.add_argument("--format", default="nv12", help='the YUV surfaces\' name: "nv12" (value 5), "nv12:bt709", "p010:bt709", ... (P010: 16-bit words)')
    a = ap.parse_args()
    profile = None
    if not a.quick and not a.no_profile:
        with tempfile.TemporaryDirectory() as d:
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable,
                                os.path.abspath(__file__), "--quick", "--format", a.format], capture_output=True, text=True, timeout=600)
            profile = {"returncode": p.returncode, "kernels": kernel_rows(d)}
            if p.returncode:
                profile["stderr_tail"] = p.stderr[-2000:]
    import torch
    gray, _, gt68 = synth.make_faces(64, seed=84)
    gt = np.ascontiguousarray(gt68[:, SEL], np.float32)
    rng = np.random.default_rng(85)
    colour = rng.integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    colour[..., 1] = gray
    stack = torch.from_numpy(colour).cuda()
    bgr = [torch.from_numpy(c).cuda() for c in colour]                       # 64 separate allocations, used in place
    H, W = gray.shape[1:]
    if a.format.lower().startswith("p010"):                                  # the luma as 10-bit samples in bits 15..6, rows of 2 W bytes
        surfaces = [torch.from_numpy(np.concatenate([(g.astype(np.uint16) << 8).view(np.uint8).reshape(H, 2 * W),
                                                     rng.integers(0, 256, (H // 2, 2 * W), dtype=np.uint8)])).cuda() for g in gray]
        nv12 = [(s.data_ptr(), W, H, 2 * W, a.format) for s in surfaces]
    else:
        surfaces = [torch.from_numpy(np.concatenate([g, rng.integers(0, 256, (H // 2, W), dtype=np.uint8)])).cuda() for g in gray]
        nv12 = [(s.data_ptr(), W, H, W, a.format) for s in surfaces]
    ctx = Context(0)
    ctx.set_model_geometry(L, *ibug.eye_indices(IDS), [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS])
    sizes = [(4096, 200)] if a.quick else [(1, 1000), (256, 1000), (4096, 300)]
    res = {"crop": f"{SIZE} x {SIZE}", "tensor": "float16 N x 3 x H x W, RGB, mean / std", "landmarks": f"RCR-22, all {L}",
           "unit": "ms per call, host clock, synchronised", "yuv_format": a.format, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n, calls in sizes:
        res["sizes"][str(n)] = run(ctx, n, calls, bgr, nv12, stack, gt, torch)
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
