"""Planar colour frames straight in (include/sdm.h, "Planar colour frames") against the route a caller with 3 x H x W
uint8 frames had before: `permute(1, 2, 0).contiguous()` of every frame, then the interleaved call -- and, for a paste, the way back into
the planar tensor.  N_FRAMES RGB frames of 1920 x 1080 resident on the device, FACES faces per frame, the shipped HOG parameters with
random regressors (the time does not depend on their values):
  step    Tracker.step on the frames
  crop    detection_model.aligned_crops_tensor, float16 N x 3 x 112 x 112 RGB with mean / std
  paste   detection_model.paste_crops_tensor of such a tensor with a feathered mask
The two routes alternate, RUNS runs of CALLS calls each behind 3 warm-up calls; every call ends in a synchronise (the library's own, and
torch's after the repacking), so the host clock around it is its time.  Per case the median over all calls of a route and the spread of
the runs' medians (max - min).
    python scripts/planar_frames_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, detection_model, feather_mask, ibug, synth  # noqa: E402

N_FRAMES, FACES, W, H, SIZE, CALLS, RUNS = 4, 3, 1920, 1080, 112, 30, 3
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def main():
    ids = ibug.RCR22_IDS
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    rng = np.random.default_rng(3)
    regs = []
    for p in params:
        r = LinearRegressor()
        r.x = rng.normal(0, 1e-4, (len(ids) * p.patch_dim + 1, 2 * len(ids))).astype(np.float32)
        regs.append(r)
    model = detection_model(SupervisedDescentOptimiser(regs), ibug.select_mean(ids), ids, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    faces, fb, _ = synth.make_faces(N_FRAMES * FACES, seed=11)
    host = rng.integers(0, 256, (N_FRAMES, 3, H, W), dtype=np.uint8)
    boxes, index = [], []
    for k in range(N_FRAMES * FACES):                                  # the synthetic faces on the green plane, FACES per frame
        f, (x0, y0) = k // FACES, (100 + 600 * (k % FACES), 300)
        g = faces[k]
        host[f, 1, y0:y0 + g.shape[0], x0:x0 + g.shape[1]] = g
        b = np.asarray(fb[k])
        boxes.append([b[0] + x0, b[1] + y0, b[2], b[3]])
        index.append(f)
    boxes, index = np.array(boxes, np.int32), np.array(index, np.int32)
    planar = torch.from_numpy(host).cuda()                             # N x 3 x H x W: what a decoder behind torch hands out
    n = len(boxes)
    ids_ = np.arange(n)
    tr = model.tracker(n)
    mask = feather_mask(SIZE, 8)
    spec = dict(dtype="float16", layout="nchw", order="rgb", mean=MEAN, std=STD)

    def packed():
        out = [planar[i].permute(1, 2, 0).contiguous() for i in range(N_FRAMES)]
        torch.cuda.synchronize()
        return out

    def step_planar():
        tr.step(ids_, planar, image_index=index, formats="rgb_planar")

    def step_packed():
        tr.step(ids_, packed(), image_index=index, formats="rgb")

    def crop_planar():
        return model.aligned_crops_tensor(SIZE, frames=planar, formats="rgb_planar", **spec)[0]

    def crop_packed():
        return model.aligned_crops_tensor(SIZE, frames=packed(), formats="rgb", **spec)[0]

    y = None

    def paste_planar():
        model.paste_crops_tensor(y, frames=planar, formats="rgb_planar", mask=mask, mean=MEAN, std=STD)

    def paste_packed():
        fr = packed()
        model.paste_crops_tensor(y, frames=fr, formats="rgb", mask=mask, mean=MEAN, std=STD)
        for i in range(N_FRAMES):                                      # the way back into the planar tensor
            planar[i].copy_(fr[i].permute(2, 0, 1))
        torch.cuda.synchronize()

    tr.start(ids_, boxes)
    step_planar()
    y = crop_planar().clone()
    assert torch.equal(y, crop_packed())                               # the two routes give the same tensor
    out = {"frames": N_FRAMES, "faces_per_frame": FACES, "width": W, "height": H, "calls": CALLS, "runs": RUNS, "cases": {}}
    for name, routes in (("step", (step_planar, step_packed)), ("crop", (crop_planar, crop_packed)), ("paste", (paste_planar, paste_packed))):
        times = {0: [], 1: []}
        for _ in range(RUNS):
            for k, fn in enumerate(routes):
                if name == "step":
                    tr.start(ids_, boxes)
                for _ in range(3):
                    fn()
                run = []
                for _ in range(CALLS):
                    t0 = time.perf_counter()
                    fn()
                    run.append((time.perf_counter() - t0) * 1e3)
                times[k].append(run)
        res = {}
        for k, label in enumerate(("planar_in_place", "permute_contiguous")):
            med = [float(np.median(r)) for r in times[k]]
            res[label] = {"median_ms": float(np.median(np.concatenate(times[k]))), "spread_ms": max(med) - min(med)}
        out["cases"][name] = res
        print(name, json.dumps(res), flush=True)
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
