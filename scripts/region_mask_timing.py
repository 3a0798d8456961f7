"""Time of the landmark region masks (Context.align_region_mask, the call behind detection_model.region_masks;
csrc/sdm_region_mask.hip) beside the same session's crop call (Context.align_crops_tensor to a float16 N x 3 x H x W tensor from BGR
frames in place) at the same shapes, everything resident on the device:
  4 096 rows at 112 x 112, 256 rows at 512 x 512, one row at 112 x 112,
on the 68-point model with the region "face outline (27 vertices) minus the outer mouth (12 vertices)", grow 2, feather 6.  To say
where the mask call's time goes it is also timed with a region of one triangle (3 edges instead of 39: what is left is the fit, the
prepare launch, the stores and the call itself).  Host clock, p50 per call, each call ended by a synchronise; every measurement is
taken in three rounds, the p50 of each round is kept and the spread of the three is the session spread.
Writes profiles/region_mask_timing.json (or --out).  --bench FILE...: JSON result lines of bench.py runs of the same job (name=path),
copied into the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import Context, HoGParam, alignment_template, ibug, synth  # noqa: E402

IDS = ibug.IBUG68_IDS
L = len(IDS)
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
ROUNDS = 3


def rounds(fn, calls, torch):
    p50 = []
    for _ in range(ROUNDS):
        ts = []
        for k in range(calls + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= 5:
                ts.append(time.perf_counter() - t0)
        p50.append(float(np.percentile(np.asarray(ts) * 1e3, 50)))
    return {"calls_per_round": calls, "p50_ms_rounds": p50, "p50_ms": float(np.median(p50)),
            "spread_percent": 100.0 * (max(p50) - min(p50)) / float(np.median(p50))}


def run(ctx, n, size, calls, bgr, gt, torch):
    idx = np.arange(n) % len(bgr)
    lm = np.arange(L)
    tmpl = alignment_template(ibug.MEAN_IBUG_LFPW_68, lm, size, size, 0.2)
    pos = lambda ids: [IDS.index(i) for i in ids]
    face, mouth = pos(ibug.REGIONS["face"]), pos(ibug.REGIONS["mouth_outer"])
    x = gt[idx] + np.random.default_rng(n).normal(0, 2, (n, 2 * L)).astype(np.float32)
    ctx.set_frames_device(bgr)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    ctx.align_set_source_frames(bgr)
    out16 = torch.empty((n, 3, size, size), dtype=torch.float16, device="cuda")
    maps = torch.empty((n, size, size), dtype=torch.uint8, device="cuda")
    res = {}
    res["crops_float16_from_bgr_frames"] = rounds(lambda: ctx.align_crops_tensor(lm, tmpl, size, size, out=out16, mean=MEAN, std=STD), calls, torch)
    res["mask_outline_minus_mouth_39_edges"] = rounds(lambda: ctx.align_region_mask(lm, tmpl, size, size, [face], [mouth], grow=2.0, feather=6.0, out=maps),
                                                      calls, torch)
    covered = float((maps > 0).float().mean().item())
    res["mask_one_triangle_3_edges"] = rounds(lambda: ctx.align_region_mask(lm, tmpl, size, size, [pos(["37", "46", "58"])], grow=2.0, feather=6.0, out=maps),
                                              calls, torch)
    ctx.align_set_source_frames(None)
    full, floor, crop = (res[k]["p50_ms"] for k in ("mask_outline_minus_mouth_39_edges", "mask_one_triangle_3_edges", "crops_float16_from_bgr_frames"))
    res["pixels_lit_fraction"] = covered
    res["mask_over_crops_p50"] = full / crop
    res["edge_loop_share_of_mask"] = (full - floor) / full                  # what 36 more edges per pixel cost, of the whole call
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_mask_timing.json"))
    ap.add_argument("--bench", nargs="*", default=[], help="name=path of files whose last JSON line is a bench.py result")
    a = ap.parse_args()
    import torch
    gray, _, gt68 = synth.make_faces(64, seed=84)
    gt = np.ascontiguousarray(gt68, np.float32)
    rng = np.random.default_rng(85)
    colour = rng.integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    colour[..., 1] = gray
    bgr = [torch.from_numpy(c).cuda() for c in colour]                       # 64 separate allocations, used in place
    ctx = Context(0)
    ctx.set_model_geometry(L, *ibug.eye_indices(IDS), [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS])
    res = {"landmarks": "68-point model", "region": "face outline (27) minus outer mouth (12), grow 2, feather 6",
           "unit": "ms per call, host clock, synchronised; p50 of each of three rounds", "device": torch.cuda.get_device_name(0), "shapes": {}}
    for n, size, calls in [(4096, 112, 100), (256, 512, 40), (1, 112, 1000)]:
        key = f"{n} x {size} x {size}"
        res["shapes"][key] = run(ctx, n, size, calls, bgr, gt, torch)
        print(key, json.dumps(res["shapes"][key]), flush=True)
    ctx.close()
    for entry in a.bench:
        name, path = entry.split("=", 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        res.setdefault("bench", {})[name] = json.loads(lines[-1]) if lines else None
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
