"""Time of the colour-to-gray conversion of frames that are already on the device (Context.set_frames_device, csrc/sdm_frames.hip:
one launch for all frames of a call) on its own, without a tracker step behind it:
  bgr 1080p x 8     8 interleaved BGR frames of 1920 x 1080, one stacked tensor
  bgr 256 x 256     256 interleaved BGR frames of 256 x 256, one stacked tensor (the set of scripts/frames_track_timing.py)
  bgra 1080p x 8    8 interleaved BGRA frames of 1920 x 1080
and, where the package knows planar frames (include/sdm.h, "Planar colour frames"), the same pixels as
  rgb_planar 1080p x 8, rgb_planar 256 x 256     N x 3 x H x W tensors
Host clock around the call, which ends in the library's own synchronise (so the time holds the descriptor set-up on the host, the table
copies and the launch); RUNS runs of CALLS calls behind 5 warm-up calls, the cases alternating; per case the median over all calls and
the spread of the runs' medians (max - min).  A tree without planar frames (the parent of that change) runs the interleaved cases alone.
    python scripts/frames_gray_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import Context, _lib  # noqa: E402

CALLS, RUNS = 40, 3


def main():
    rng = np.random.default_rng(5)
    big = torch.from_numpy(rng.integers(0, 256, (8, 1080, 1920, 4), dtype=np.uint8)).cuda()
    small = torch.from_numpy(rng.integers(0, 256, (256, 256, 256, 3), dtype=np.uint8)).cuda()
    cases = {"bgr 1080p x 8": (big[..., :3].contiguous(), "bgr"), "bgr 256 x 256": (small, "bgr"), "bgra 1080p x 8": (big, "bgra")}
    if hasattr(_lib, "frame_planes"):
        cases["rgb_planar 1080p x 8"] = (big[..., :3].permute(0, 3, 1, 2).contiguous(), "rgb_planar")
        cases["rgb_planar 256 x 256"] = (small.permute(0, 3, 1, 2).contiguous(), "rgb_planar")
    ctx = Context(0)
    times = {k: [] for k in cases}
    for _ in range(RUNS):
        for name, (frames, fmt) in cases.items():
            for _ in range(5):
                ctx.set_frames_device(frames, fmt)
            run = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                ctx.set_frames_device(frames, fmt)
                run.append((time.perf_counter() - t0) * 1e3)
            times[name].append(run)
    out = {"calls": CALLS, "runs": RUNS, "unit": "ms per call, host clock, the call ends in a stream synchronise", "cases": {}}
    for name, runs in times.items():
        med = [float(np.median(r)) for r in runs]
        out["cases"][name] = {"median_ms": float(np.median(np.concatenate(runs))), "spread_ms": max(med) - min(med), "run_medians_ms": med}
        print(name, json.dumps(out["cases"][name]), flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
