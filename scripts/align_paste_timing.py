"""Time of the paste-back of crop tensors (detection_model.paste_crops_tensor, csrc/sdm_align_paste.hip) beside the crop call it inverts
(detection_model.aligned_crops_tensor, csrc/sdm_align_tensor.hip) for the same rows in the same session: 256 and 4 096 rows of
112 x 112 float16 NCHW RGB with mean / std, BGR frames of 1920 x 1080 resident on the device and used in place, the crop 100 to 600 frame
pixels wide (crop -> frame scale 100 / 112 ... 600 / 112, +-20 degrees, wholly inside the frame), with
  one     one face per frame (as many frames as rows)
  sixteen 16 faces per frame (rows / 16 frames; the faces overlap where they fall on each other)
Every case runs in a child process of its own under its own time limit, one after the other; the first that fails ends the run.  The
context runs on a torch stream; a call is bracketed by two HIP events on that stream (the call ends in the library's own synchronise),
5 warm-up calls, then CALLS calls: the median and the spread (max - min) of the event times, and the host clock's median beside them.
Bytes: the tensor once (rows x 3 x 112 x 112 x 2), and per frame pixel under a crop three bytes read and three written -- the crops'
area in the frame, (112 scale)^2 summed over the rows, an estimate that counts overlaps twice; the crop call reads about four taps of
three bytes per element and writes the tensor.  Writes profiles/align_paste_timing.json (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, CALLS, W, H = 112, 25, 1920, 1080
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
CASES = [(256, 1), (256, 16), (4096, 1), (4096, 16)]


def timed(torch, stream, fn):
    for _ in range(5):
        fn()
    ev, host = [], []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        fn()                                                   # (ends in the library's stream synchronise)
        b.record(stream)
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ev)), "spread_ms": float(max(ev) - min(ev)), "host_median_ms": float(np.median(host)), "calls": CALLS}


def child(rows, per_frame):
    sys.path.insert(0, ROOT)
    import torch
    from superviseddescent_amd import (HoGParam, LinearRegressor, SupervisedDescentOptimiser, alignment_template, detection_model, feather_mask,
                                       ibug)
    ids = ibug.RCR22_IDS
    L = len(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    stream = torch.cuda.Stream()
    model = detection_model(SupervisedDescentOptimiser([LinearRegressor() for _ in params], stream=stream.cuda_stream), ibug.select_mean(ids), ids,
                            params, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    ctx = model.optimised_model.ctx
    re, le = ibug.eye_indices(ids)
    ctx.set_model_geometry(L, re, le, params)
    rng = np.random.default_rng(7)
    n_frames = rows // per_frame
    store = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    frames = [(store[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)]
    ctx.set_frames_device(frames)
    ctx.set_sample_image_index(np.arange(rows) // per_frame)
    # the rows: the default template seen through a similarity of scale 100 / 112 ... 600 / 112, the crop wholly inside the frame
    tmpl = alignment_template(model.mean, np.arange(L), SIZE, SIZE, 0.2).astype(np.float64)
    s = rng.uniform(100.0, 600.0, rows) / SIZE
    ang = np.deg2rad(rng.uniform(-20, 20, rows))
    c, sn = s * np.cos(ang), s * np.sin(ang)
    half = 0.5 * SIZE * s * (np.abs(np.cos(ang)) + np.abs(np.sin(ang))) + 2
    centre = np.stack([rng.uniform(half, W - 1 - half), rng.uniform(half, H - 1 - half)], 1)
    q = tmpl - (SIZE - 1) / 2
    x = np.zeros((rows, 2 * L), np.float32)
    x[:, :L] = c[:, None] * q[:, 0] - sn[:, None] * q[:, 1] + centre[:, :1]
    x[:, L:] = sn[:, None] * q[:, 0] + c[:, None] * q[:, 1] + centre[:, 1:]
    ctx.set_x(x)
    out = torch.empty((rows, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    mask = torch.from_numpy(feather_mask(SIZE, 8)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "rows": rows, "faces_per_frame": per_frame, "frames": n_frames}
    res["crop"] = timed(torch, stream, lambda: model.aligned_crops_tensor(SIZE, frames=frames, out=out, mean=MEAN, std=STD))
    _, _, flags = model.aligned_crops_tensor(SIZE, frames=frames, out=out, mean=MEAN, std=STD)
    res["paste"] = timed(torch, stream, lambda: model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD, mask=mask))
    res["paste_no_mask"] = timed(torch, stream, lambda: model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD))
    _, f2 = model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD, mask=mask)
    res["rows_flagged"] = int((flags != 0).sum() + (f2 != 0).sum())
    tensor_bytes = rows * 3 * SIZE * SIZE * 2
    under = float(((SIZE * s) ** 2).sum())
    res["paste"]["bytes_read_estimate"] = res["paste_no_mask"]["bytes_read_estimate"] = int(tensor_bytes + 3 * under)
    res["paste"]["bytes_written_estimate"] = res["paste_no_mask"]["bytes_written_estimate"] = int(3 * under)
    res["crop"]["bytes_read_estimate"] = int(rows * SIZE * SIZE * 4 * 3)
    res["crop"]["bytes_written"] = tensor_bytes
    res["paste_over_crop"] = res["paste"]["median_ms"] / res["crop"]["median_ms"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_paste_timing.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    runs = []
    for rows, per_frame in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), str(per_frame)], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the child for %d rows, %d per frame failed with status %d" % (rows, per_frame, r.returncode))
        e = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        runs.append(e)
        print("%5d rows, %2d per frame: crop %8.3f ms  paste %8.3f ms (no mask %8.3f ms)  ratio %.2f" %
              (rows, per_frame, e["crop"]["median_ms"], e["paste"]["median_ms"], e["paste_no_mask"]["median_ms"], e["paste_over_crop"]), flush=True)
    doc = {"tensor": "112 x 112 x 3 float16 NCHW RGB, mean / std", "frames": "BGR 1920 x 1080, in place", "crop_width_in_frame": "100 ... 600 pixels",
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call",
           "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
