"""Time of the aligned crops (Context.align_crops, the call behind detection_model.aligned_crops; csrc/sdm_align.hip) at N = 1, 256 and
4 096 rows, 112 x 112 crops, C = 1 (the context's gray images) and C = 3 (a colour stack resident on the device), the frames resident on
the device.  Per size: the wall time of a call writing into a device tensor (out=, no copy of the crops) and of one fetching the crops
to the host, on the host clock (the call ends with its stream synchronise).  The kernels' own times come from the --quick run under
rocprofv3 --kernel-trace --stats (profiles/align_rocprofv3_*).  Writes profiles/align_timing.json (or --out) and prints it.
  --quick: N = 4 096 only, 200 calls (the run under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import Context, HoGParam, alignment_template, ibug, synth  # noqa: E402

IDS = ibug.RCR22_IDS
L = len(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
SIZE = 112


def stats(ts):
    a = np.asarray(ts) * 1e3
    return {"calls": len(ts), "p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "min_ms": float(a.min()),
            "mean_ms": float(a.mean())}


def run(ctx, n, calls, gray, colour_dev, gt, torch):
    idx = np.arange(n) % gray.shape[0]
    ctx.upload_images(list(gray))
    ctx.set_sample_image_index(idx)
    ctx.set_x(gt[idx] + np.random.default_rng(n).normal(0, 2, (n, 2 * L)).astype(np.float32))
    tmpl = alignment_template(ibug.select_mean(IDS), np.arange(L), SIZE, SIZE, 0.2)
    lm = np.arange(L)
    out = {}
    for C, src in ((1, None), (3, colour_dev)):
        ctx.align_set_source(src)
        dev = torch.empty((n, SIZE, SIZE, C), dtype=torch.uint8, device="cuda")
        res = {}
        for name, kw in (("device_out", {"out": dev}), ("host_out", {})):
            ts = []
            for k in range(calls + 5):
                t0 = time.perf_counter()
                ctx.align_crops(lm, tmpl, SIZE, SIZE, C, **kw)
                if k >= 5:
                    ts.append(time.perf_counter() - t0)
            res[name] = stats(ts)
        res["bytes_written"] = n * SIZE * SIZE * C
        res["write_bound_us_at_6TBps"] = n * SIZE * SIZE * C / 6e12 * 1e6
        out[f"C{C}"] = res
    ctx.align_set_source(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.json"))
    a = ap.parse_args()
    import torch
    gray, _, gt68 = synth.make_faces(64, seed=84)
    gt = np.ascontiguousarray(gt68[:, SEL], np.float32)
    rng = np.random.default_rng(85)
    colour = rng.integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    colour[..., 1] = gray
    colour_dev = torch.from_numpy(colour).cuda()
    ctx = Context(0)
    ctx.set_model_geometry(L, *ibug.eye_indices(IDS), [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS])
    sizes = [(4096, 200)] if a.quick else [(1, 1000), (256, 1000), (4096, 300)]
    res = {"crop": f"{SIZE} x {SIZE}", "landmarks": f"RCR-22, all {L}", "unit": "ms per aligned_crops call",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n, calls in sizes:
        res["sizes"][str(n)] = run(ctx, n, calls, gray, colour_dev, gt, torch)
        print(n, json.dumps(res["sizes"][str(n)]), flush=True)
    ctx.close()
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
