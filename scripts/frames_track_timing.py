"""Tracker step time for 256 streams with three kinds of input (profiles/frames_ingest.txt):
  device BGR   a 256 x H x W x 3 uint8 tensor already on the device (Context.set_frames_device: one conversion launch)
  host BGR     the same frames as host arrays (upload + sdm_upload_images_bgr_u8: what a caller without the device path does)
  device gray  a contiguous 256 x H x W tensor (sdm_set_images_device, in place: the floor)
The variants are alternated, RUNS runs of STEPS steps each; a step ends in a synchronise, so the host clock around it is the step time.
    python scripts/frames_track_timing.py [out.json]"""
import json
import sys
import time

import numpy as np
import torch

from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, ibug, synth

S, STEPS, RUNS = 256, 20, 3


def main():
    ids = ibug.RCR22_IDS
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    rng = np.random.default_rng(3)
    regs = []
    for p in params:
        r = LinearRegressor()
        r.x = rng.normal(0, 1e-3, (len(ids) * p.patch_dim + 1, 2 * len(ids))).astype(np.float32)
        regs.append(r)
    model = detection_model(SupervisedDescentOptimiser(regs), ibug.select_mean(ids), ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    images, boxes, _ = synth.make_faces(S, seed=11)
    bgr = rng.integers(0, 256, images.shape + (3,), dtype=np.uint8)
    bgr[..., 1] = images
    inputs = {"device BGR": torch.from_numpy(bgr).cuda(), "host BGR": bgr, "device gray": torch.from_numpy(images).cuda()}
    tr = model.tracker(S, init="realign", min_size=0.0, max_scale_change=0.0)
    sid = np.arange(S)
    times = {k: [] for k in inputs}
    for run in range(RUNS + 1):                                  # (run 0 warms every variant up)
        for name, frames in inputs.items():
            tr.start(sid, boxes)
            tr.step(sid, frames, fetch=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                tr.step(sid, frames, fetch=False)
            dt = (time.perf_counter() - t0) / STEPS
            if run:
                times[name].append(dt * 1e3)
    out = {"streams": S, "frame": list(images.shape[1:]), "levels": len(params), "steps_per_run": STEPS,
           "ms_per_step": {k: {"runs": v, "mean": float(np.mean(v)), "spread_percent": float(100 * (max(v) - min(v)) / np.mean(v))} for k, v in times.items()}}
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
