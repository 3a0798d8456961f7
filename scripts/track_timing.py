"""Wall time of one tracker step (detection_model.tracker, csrc/sdm_track.hip) on a trained RCR-22 cascade (the four shipped
levels), at S = 1, 16, 256 and 4 096 streams: host clock around Tracker.step, which ends with the step's one stream synchronise and
returns the landmarks and lost masks.  Per size, frames resident on the device (uploaded once, every step reads them) and frames
uploaded from the host at every step; beside them the per-frame loop of detection_model.detect(image, initialisation) over the same
streams.  Writes profiles/track_timing.json (or the path given with --out) and prints it.
  --quick: S = 256 only, 200 steps (the run under rocprofv3 --kernel-trace --stats).
  --motion: the cost of the motion-compensated initialisation (tracker(motion=True), csrc/sdm_track_motion.hip), resident frames only:
  per size the step with motion never configured and with motion on, in alternating rounds of one process; the added time and its
  share of the step; the bytes a row's search reads.  Writes profiles/track_motion_timing.json.  --plain-only keeps to the tracker
  without motion (it runs on a tree from before the feature too); --root DIR imports the package from another tree, so that one job
  can alternate two builds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[:-1] else ROOT)
from superviseddescent_amd import (HoGParam, HogTransform, LinearRegressor, Regulariser, SupervisedDescentOptimiser,  # noqa: E402
                                   detection_model, ibug, synth)

IDS = ibug.RCR22_IDS


def trained_model():
    images, boxes, gt = synth.make_faces(600, seed=9200, chunk=32)
    params = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=9201)
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in params])
    sdo.train(x_star, x0, None, HogTransform(images, params, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, ibug.select_mean(IDS), IDS, params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def stats(ts):
    a = np.asarray(ts) * 1e3
    return {"steps": len(ts), "p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)),
            "min_ms": float(a.min()), "mean_ms": float(a.mean())}


def run_size(dm, S, steps, faces, boxes, legacy_calls):
    # stream s follows face s % F of the video; frame t of the run shows frame t % 2 of it
    F = faces.shape[1]
    idx = np.arange(S) % F
    frames = [np.ascontiguousarray(faces[t][idx]) for t in range(2)]
    b0 = boxes[0][idx]
    ids = np.arange(S)
    tr = dm.tracker(S, init="realign", min_size=0.0, max_scale_change=0.0)
    out, restarts = {}, 0

    def loop(n, frame_of):
        nonlocal restarts
        ts = []
        tr.start(ids, b0)
        for k in range(n + 5):
            fr = frame_of(k)
            t0 = time.perf_counter()
            _, lost = tr.step(ids, fr)
            dt = time.perf_counter() - t0
            if k >= 5:                                                   # (5 warm-up steps)
                ts.append(dt)
            if lost.any():
                restarts += int((lost != 0).sum())
                tr.start(ids[lost != 0], b0[lost != 0])
        return ts

    dm.optimised_model.ctx.upload_images(frames[0])
    out["resident"] = stats(loop(steps, lambda k: None))
    out["uploaded"] = stats(loop(steps, lambda k: frames[k % 2]))
    out["restarts"] = restarts
    # the per-frame detect(image, initialisation) loop of the reference's API, one call per stream (fewer steps at large S)
    n_legacy = max(2, min(steps, legacy_calls // S))
    x = np.stack([synth.align_mean(dm.mean, tuple(int(v) for v in b)) for b in b0])
    ts = []
    for k in range(n_legacy + 1):
        fr = frames[k % 2]
        t0 = time.perf_counter()
        for s in range(S):
            x[s] = dm.detect(fr[s], initialisation=x[s][None])
        dt = time.perf_counter() - t0
        if k >= 1:
            ts.append(dt)
    out["detect_loop"] = stats(ts)
    return out


def motion_size(dm, S, steps, rounds, faces, boxes, plain_only):
    """p50 of Tracker.step on resident frames: motion never configured / motion on, `rounds` alternating rounds of `steps` steps"""
    F = faces.shape[1]
    idx = np.arange(S) % F
    frame = np.ascontiguousarray(faces[0][idx])
    b0 = boxes[0][idx]
    ids = np.arange(S)
    ts = {"off": [], "on": []}
    for r in range(rounds):
        for kind in ("off",) if plain_only else ("off", "on"):
            tr = dm.tracker(S, init="realign", min_size=0.0, max_scale_change=0.0, **({"motion": True} if kind == "on" else {}))
            dm.optimised_model.ctx.upload_images(frame)
            tr.start(ids, b0)
            for k in range(steps + 5):
                t0 = time.perf_counter()
                tr.step(ids, None)
                dt = time.perf_counter() - t0
                if k >= 5:
                    ts[kind].append(dt)
            if kind == "on" and r == 0:
                k_cells = sorted(set(tr.motion(ids)[1][:, 0].tolist()))
    out = {"off": stats(ts["off"])}
    if not plain_only:
        out["on"] = stats(ts["on"])
        out["added_ms"] = out["on"]["p50_ms"] - out["off"]["p50_ms"]
        out["added_share_of_step"] = out["added_ms"] / out["on"]["p50_ms"]
        out["cell_sizes"] = k_cells
    return out


def motion_main(a):
    faces, _, boxes = synth.make_tracks(64, 2, seed=81)
    dm = trained_model()
    import torch
    # a row's search reads the window of (32 + 2 * 8)^2 cells of k x k bytes, its store the chip of 32^2 cells
    res = {"model": "RCR-22, 4 shipped HOG levels", "unit": "wall ms per step (host clock, includes the step's synchronise), resident frames",
           "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", "search": 8, "scale": 1.25,
           "bytes_read_per_row": {"k=%d" % k: {"search": (48 * k) ** 2 + 1024, "store": (32 * k) ** 2} for k in (6, 40)}, "sizes": {}}
    for S, steps in [(1, 300), (16, 300), (256, 300), (4096, 40)]:
        res["sizes"][str(S)] = motion_size(dm, S, steps, 3, faces, boxes, a.plain_only)
        print(S, json.dumps(res["sizes"][str(S)]), flush=True)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "track_timing.json") else os.path.join(ROOT, "profiles", "track_motion_timing.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_timing.json"))
    ap.add_argument("--legacy-calls", type=int, default=8000, help="detect() calls per size for the per-frame loop")
    a = ap.parse_args()
    if a.motion:
        return motion_main(a)
    faces, _, boxes = synth.make_tracks(64, 2, seed=81)
    dm = trained_model()
    sizes = [(256, 200)] if a.quick else [(1, 1000), (16, 1000), (256, 1000), (4096, 100)]
    import torch
    res = {"model": "RCR-22, 4 shipped HOG levels", "unit": "wall ms per step (host clock, includes the step's synchronise)",
           "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", "sizes": {}}
    for S, steps in sizes:
        res["sizes"][str(S)] = run_size(dm, S, steps, faces, boxes, a.legacy_calls if not a.quick else 256)
        print(S, json.dumps(res["sizes"][str(S)]), flush=True)
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
