"""The tracker's temporal landmark filter (detection_model.tracker(smooth=...), csrc/sdm_track_filter.hip) on a trained RCR-22 cascade
(the four shipped levels), by the method of scripts/track_timing.py: host clock around Tracker.step, which ends with the step's one
stream synchronise, frames resident on the device, in ONE session --
  timing    p50 / p99 wall time of step(ids) and of step(ids, dt=1/30) at S = 1, 256 and 4 096 streams
  quality   synth.make_tracks, 16 streams x 30 frames, dt = 1/30, over a small grid of (min_cutoff, beta): the mean normalised error
            of the filtered rows against the ground truth beside the raw rows' and detect's from the true box, and the RMS
            frame-to-frame displacement (pixels) of the raw rows, the filtered rows and the ground truth
Writes profiles/track_filter_timing.json (or the path given with --out) and prints it.
  --quick: S = 256 only, 200 filtered steps, nothing written (the run under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from superviseddescent_amd import ibug, synth  # noqa: E402
from track_timing import stats, trained_model  # noqa: E402

IDS = ibug.RCR22_IDS
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
DT = 1.0 / 30.0
GRID = [(0.5, 0.0), (1.0, 0.0), (1.0, 5.0), (1.0, 20.0), (3.0, 5.0)]


def run_size(dm, S, steps, faces, boxes, quick):
    F = faces.shape[1]
    idx = np.arange(S) % F
    b0 = boxes[0][idx]
    ids = np.arange(S)
    tr = dm.tracker(S, init="realign", min_size=0.0, max_scale_change=0.0, smooth=(1.0, 5.0))
    dm.optimised_model.ctx.upload_images(np.ascontiguousarray(faces[0][idx]))
    out = {}
    for name, kw in (("step", {}), ("step_dt", {"dt": DT})):
        if quick and not kw:
            continue
        ts = []
        tr.start(ids, b0)
        for k in range(steps + 5):
            t0 = time.perf_counter()
            lost = tr.step(ids, None, **kw)[1]
            t1 = time.perf_counter() - t0
            if k >= 5:                                                   # (5 warm-up steps)
                ts.append(t1)
            if lost.any():
                tr.start(ids[lost != 0], b0[lost != 0])
        out[name] = stats(ts)
    if not quick:
        out["filter_p50_us"] = (out["step_dt"]["p50_ms"] - out["step"]["p50_ms"]) * 1e3
    return out


def rms_step(rows):
    """RMS over streams, frames and landmarks of the distance a landmark moves from one frame to the next"""
    d = np.diff(np.asarray(rows, np.float64), axis=0)
    L = d.shape[2] // 2
    return float(np.sqrt(np.mean(d[:, :, :L] ** 2 + d[:, :, L:] ** 2)))


def quality(dm):
    frames, gt, boxes = synth.make_tracks(16, 30, seed=79)
    n_frames, S = frames.shape[:2]
    c = dm.optimised_model.ctx
    ids = np.arange(S)
    truth = gt[:, :, SEL]

    def run(smooth):
        tr = dm.tracker(S, init="realign", smooth=smooth)
        tr.start(ids, boxes[0])
        rows, errs, restarts = [], [], 0
        for t in range(n_frames):
            res = tr.step(ids, list(frames[t])) if smooth is None else tr.step(ids, list(frames[t]), dt=DT)
            rows.append(res[0])
            c.set_targets(truth[t])
            errs.append(c.normalised_errors(fetch=False)[1])             # (of the current rows: the filtered ones after a step with dt)
            lost = res[1]
            if lost.any():
                restarts += int((lost != 0).sum())
                tr.start(ids[lost != 0], boxes[t][lost != 0])
        return np.stack(rows), float(np.mean(errs)), restarts

    raw, e_raw, restarts = run(None)
    e_detect = []
    for t in range(n_frames):
        dm.detect_batch(list(frames[t]), boxes[t])
        c.set_targets(truth[t])
        e_detect.append(c.normalised_errors(fetch=False)[1])
    out = {"streams": S, "frames": n_frames, "dt": DT, "restarts": restarts, "error_detect": float(np.mean(e_detect)), "error_raw": e_raw,
           "rms_step_raw_px": rms_step(raw), "rms_step_truth_px": rms_step(truth), "grid": []}
    for min_cutoff, beta in GRID:
        rows, e, _ = run((min_cutoff, beta))
        out["grid"].append({"min_cutoff": min_cutoff, "beta": beta, "error_filtered": e, "error_over_raw": e / e_raw,
                            "rms_step_filtered_px": rms_step(rows)})
        print(json.dumps(out["grid"][-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_filter_timing.json"))
    a = ap.parse_args()
    faces, _, boxes = synth.make_tracks(64, 2, seed=81)
    dm = trained_model()
    sizes = [(256, 200)] if a.quick else [(1, 1000), (256, 1000), (4096, 200)]
    import torch
    res = {"model": "RCR-22, 4 shipped HOG levels", "unit": "wall ms per step (host clock, includes the step's synchronise), frames resident",
           "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", "sizes": {}}
    for S, steps in sizes:
        res["sizes"][str(S)] = run_size(dm, S, steps, faces, boxes, a.quick)
        print(S, json.dumps(res["sizes"][str(S)]), flush=True)
    if not a.quick:
        res["quality"] = quality(dm)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
