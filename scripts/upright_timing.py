"""Wall time of the upright path (csrc/sdm_upright.hip) on a trained RCR-22 cascade (the four shipped levels), frames resident on the
device, chip 256: detect_batch with roll= against plain detect_batch on the same batch at N = 1, 256 and 4 096 rows, and the upright
tracker step against the realign step at S = 1, 256 and 4 096 streams, all in one run.  Host clock around calls that end with the
call's stream synchronise.  Writes profiles/upright_timing.json (or the path given with --out) and prints it.
  --quick: N = S = 4 096 only, 20 calls each (the run under rocprofv3 --kernel-trace --stats: the set-up, chip and back-map launches'
  microseconds come from its statistics), then three aligned_crops calls that write the same N x 256 x 256 bytes through the direct
  warp of csrc/sdm_align.hip (align_warp_kernel), the form the chip launch is compared with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import (HoGParam, HogTransform, LinearRegressor, Regulariser, SupervisedDescentOptimiser,  # noqa: E402
                                   detection_model, ibug, synth)

IDS = ibug.RCR22_IDS
CHIP, GUARD = 256, 32
WRITE_BW = 6.0e12                                                         # bytes / s: the figure the project measures writes against


def trained_model():
    images, boxes, gt = synth.make_faces(600, seed=9200, chunk=32)
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=9201)
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in params])
    sdo.train(x_star, x0, None, HogTransform(images, params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, ibug.select_mean(IDS), IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def stats(ts):
    a = np.asarray(ts) * 1e3
    return {"calls": len(ts), "p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)),
            "min_ms": float(a.min()), "mean_ms": float(a.mean())}


def timed(fn, n, warm=5):
    ts = []
    for k in range(n + warm):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if k >= warm:
            ts.append(dt)
    return stats(ts)


def run_size(dm, N, calls, faces, boxes):
    c = dm.optimised_model.ctx
    F = faces.shape[1]
    idx = (np.arange(N) % F).astype(np.int32)
    b0 = boxes[0][idx]
    rolls = np.random.default_rng(N).uniform(-180, 180, N).astype(np.float32)
    ids = np.arange(N)
    out = {}
    c.upload_images(faces[0])
    c.set_sample_image_index(idx)
    c.set_templates(None)
    c.upright_configure(CHIP, GUARD)

    x0 = np.stack([synth.align_mean(dm.mean, tuple(int(v) for v in b)) for b in b0])

    def plain():                                                          # (one copy in, the cascade, one synchronise behind it)
        c.set_x(x0)
        c.detect_batch(fetch=False)
        c.synchronize()

    out["detect_plain"] = timed(plain, calls)
    out["detect_upright"] = timed(lambda: c.detect_batch_upright(dm.mean, b0, rolls, fetch=False), calls)
    out["detect_extra_share"] = out["detect_upright"]["p50_ms"] / out["detect_plain"]["p50_ms"] - 1.0
    for name, kw in (("step_realign", dict(init="realign")), ("step_upright", dict(init="upright", chip=CHIP, guard=GUARD))):
        tr = dm.tracker(N, min_size=0.0, max_scale_change=0.0, **kw)
        tr.start(ids, b0)
        c.set_sample_image_index(idx)

        def step():
            _, lost = c.track_step(ids, fetch=False)
            if lost.any():
                tr.start(ids[lost != 0], b0[lost != 0])

        out[name] = timed(step, calls)
    out["step_extra_share"] = out["step_upright"]["p50_ms"] / out["step_realign"]["p50_ms"] - 1.0
    out["chip_bytes_bound_us"] = 2.0 * N * CHIP * CHIP / WRITE_BW * 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upright_timing.json"))
    a = ap.parse_args()
    faces, _, boxes = synth.make_tracks(64, 1, seed=81)
    dm = trained_model()
    sizes = [(4096, 20)] if a.quick else [(1, 300), (256, 300), (4096, 60)]
    import torch
    res = {"model": "RCR-22, 4 shipped HOG levels", "chip": CHIP, "unit": "wall ms per call (host clock, includes the call's synchronise)",
           "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", "sizes": {}}
    for N, calls in sizes:
        res["sizes"][str(N)] = run_size(dm, N, calls, faces, boxes)
        print(N, json.dumps(res["sizes"][str(N)]), flush=True)
    if a.quick:                                                           # the direct warp at the chip launch's byte count
        c = dm.optimised_model.ctx
        out = torch.empty((c.N, CHIP, CHIP, 1), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            dm.aligned_crops(CHIP, out=out)
        c.synchronize()
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
