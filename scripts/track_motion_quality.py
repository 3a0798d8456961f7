"""What the tracker's motion-compensated initialisation (detection_model.tracker(motion=...), csrc/sdm_track_motion.hip) does to a
trained RCR-22 cascade (the four shipped levels, the model of tests/test_gpu_track.py) on synthetic video:
  min_gain   on the slow video (synth.make_tracks defaults, 16 streams x 30 frames, up to 3 pixels per frame) the share of searched
             rows left at shift (0, 0), for min_gain in {0, 16, 32, 64}; the default is the smallest value that leaves at least 90 %,
             or the largest of the four when none does
  quality    on make_tracks(16, 30, size=384, max_step=d), d in {3, 10, 20, 30, 40}: the mean normalised error and the streams lost of
             the plain realign tracker and of the same tracker with motion on, beside detect from each frame's true box
  scale      at the fast step (the smallest d at which the plain tracker fails) the same for chips of 0.75 to 1.5 face sizes
Writes profiles/track_motion_quality.json (or the path given with --out) and prints it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import ibug, synth  # noqa: E402
from superviseddescent_amd.engine import MOTION_MIN_GAIN  # noqa: E402
from track_timing import trained_model  # noqa: E402

IDS = ibug.RCR22_IDS
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])


def run(dm, video, motion):
    """mean normalised errors (tracker, detect from the true box), rows lost, rows searched, searched rows at shift (0, 0)"""
    frames, gt, boxes = video
    S = frames.shape[1]
    c = dm.optimised_model.ctx
    tr = dm.tracker(S, init="realign", motion=motion)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    e_track, e_detect, lost_rows, searched, still = [], [], 0, 0, 0
    for t in range(frames.shape[0]):
        res, lost = tr.step(ids, list(frames[t]))
        c.set_targets(gt[t][:, SEL])
        e_track.append(c.normalised_errors(fetch=False)[1])
        if motion is not None:
            m = tr.motion(ids)[0]
            searched += int(m[:, 5].sum())
            still += int(((m[:, 5] == 1) & (m[:, 0] == 0) & (m[:, 1] == 0)).sum())
        if lost.any():
            lost_rows += int((lost != 0).sum())
            tr.start(ids[lost != 0], boxes[t][lost != 0])
        dm.detect_batch(list(frames[t]), boxes[t])
        c.set_targets(gt[t][:, SEL])
        e_detect.append(c.normalised_errors(fetch=False)[1])
    return {"error": float(np.mean(e_track)), "detect_error": float(np.mean(e_detect)), "lost": lost_rows, "searched": searched,
            "still": still}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_motion_quality.json"))
    a = ap.parse_args()
    dm = trained_model()
    import torch
    res = {"model": "RCR-22, 4 shipped HOG levels", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none",
           "search": 8, "scale": 1.25, "min_gain_grid": {}, "quality": {}}
    slow = synth.make_tracks(16, 30)
    for g in (0, 16, 32, 64):
        r = run(dm, slow, (8, 1.25, g))
        r["still_share"] = r["still"] / max(r["searched"], 1)
        res["min_gain_grid"][str(g)] = r
        print("min_gain", g, json.dumps(r), flush=True)
    ok = [g for g in (0, 16, 32, 64) if res["min_gain_grid"][str(g)]["still_share"] >= 0.9]
    res["min_gain_rule"] = ok[0] if ok else None
    res["min_gain_default"] = MOTION_MIN_GAIN
    for d in (3, 10, 20, 30, 40):
        video = synth.make_tracks(16, 30, size=384, max_step=float(d))
        plain, on = run(dm, video, None), run(dm, video, (8, 1.25, MOTION_MIN_GAIN))
        res["quality"][str(d)] = {"plain": plain, "motion": on, "ratio_motion_to_detect": on["error"] / on["detect_error"]}
        print("d", d, json.dumps(res["quality"][str(d)]), flush=True)
    base = res["quality"]["3"]["plain"]["error"]
    fast = [d for d in (3, 10, 20, 30, 40) if res["quality"][str(d)]["plain"]["error"] >= 3 * base or res["quality"][str(d)]["plain"]["lost"] > 0]
    res["fast_step"] = fast[0] if fast else None
    # the chip's size at the fast step: a smaller chip holds less of a background that does not move with the face
    res["scale_grid"] = {}
    if res["fast_step"]:
        video = synth.make_tracks(16, 30, size=384, max_step=float(res["fast_step"]))
        for scale in (0.75, 1.0, 1.25, 1.5):
            res["scale_grid"][str(scale)] = run(dm, video, (8, scale, MOTION_MIN_GAIN))
            print("scale", scale, json.dumps(res["scale_grid"][str(scale)]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
