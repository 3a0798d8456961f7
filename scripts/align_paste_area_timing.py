"""Time of the filtered paste (detection_model.paste_crops_tensor(filter="area"), csrc/sdm_align_paste.hip: paste_kernel_t<false, true>) beside the
unfiltered paste of the same rows in the same session, where the crop outsizes the face: 256 rows of C x C float16 NCHW RGB with
mean / std and a feathered opacity map, C = 256 and 512, BGR frames of 1920 x 1080 resident on the device and written in place, the crop
64 to 200 frame pixels wide (crop -> frame scale 64 / C ... 200 / C, +-20 degrees, wholly inside the frame: S spans 2 to 8), with
  one     one face per frame (256 frames)
  sixteen 16 faces per frame (16 frames; the faces overlap where they fall on each other)
Every case runs in a child process of its own under its own time limit, one after the other; the first that fails ends the run.  The
context runs on a torch stream; a call is bracketed by two HIP events on that stream (the call ends in the library's own synchronise),
5 warm-up calls, then CALLS calls: the median and the spread (max - min) of the event times, and the host clock's median beside them.
Per case: both times, their ratio, the mean S and mean S^2 of the rows, the time per sub-sample per frame pixel -- the filtered time over
the sum of (crop width in the frame)^2 S^2 --, and bytes: the tensor once (what a decode-once kernel would have to read), the taps the
kernel asks for (sub-samples x 4 taps x 3 channels x 2 bytes, nearly all served by the caches), and per frame pixel under a crop three
bytes read and three written.  Writes profiles/paste_area_timing.json (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, CALLS, W, H = 256, 25, 1920, 1080
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
CASES = [(256, 1), (256, 16), (512, 1), (512, 16)]                 # (crop size, faces per frame)


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


def child(size, per_frame):
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
    n_frames = ROWS // per_frame
    store = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    frames = [(store[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)]
    ctx.set_frames_device(frames)
    ctx.set_sample_image_index(np.arange(ROWS) // per_frame)
    # the rows: the default template seen through a similarity of scale 64 / size ... 200 / size, the crop wholly inside the frame
    tmpl = alignment_template(model.mean, np.arange(L), size, size, 0.2).astype(np.float64)
    width = rng.uniform(64.0, 200.0, ROWS)
    s = width / size
    ang = np.deg2rad(rng.uniform(-20, 20, ROWS))
    c, sn = s * np.cos(ang), s * np.sin(ang)
    half = 0.5 * size * s * (np.abs(np.cos(ang)) + np.abs(np.sin(ang))) + 2
    centre = np.stack([rng.uniform(half, W - 1 - half), rng.uniform(half, H - 1 - half)], 1)
    q = tmpl - (size - 1) / 2
    x = np.zeros((ROWS, 2 * L), np.float32)
    x[:, :L] = c[:, None] * q[:, 0] - sn[:, None] * q[:, 1] + centre[:, :1]
    x[:, L:] = sn[:, None] * q[:, 0] + c[:, None] * q[:, 1] + centre[:, 1:]
    ctx.set_x(x)
    out = torch.empty((ROWS, 3, size, size), dtype=torch.float16, device="cuda")
    mask = torch.from_numpy(feather_mask(size, size // 14)).cuda()
    model.aligned_crops_tensor(size, frames=frames, out=out, mean=MEAN, std=STD)
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "crop": size, "faces_per_frame": per_frame, "frames": n_frames}
    res["unfiltered"] = timed(torch, stream, lambda: model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD, mask=mask))
    res["area"] = timed(torch, stream, lambda: model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD, mask=mask, filter="area"))
    _, flags, S = model.paste_crops_tensor(out, frames=frames, mean=MEAN, std=STD, mask=mask, filter="area")
    S = S.astype(np.float64)
    res["rows_flagged"] = int((flags != 0).sum())
    res["S_min"], res["S_max"], res["S_mean"], res["S2_mean"] = int(S.min()), int(S.max()), float(S.mean()), float((S * S).mean())
    res["area_over_unfiltered"] = res["area"]["median_ms"] / res["unfiltered"]["median_ms"]
    under = float((width ** 2).sum())                                        # frame pixels under the crops (overlaps counted twice)
    subs = float((width ** 2 * S * S).sum())
    res["frame_pixels_under_crops"] = int(under)
    res["sub_samples"] = int(subs)
    res["area"]["ns_per_sub_sample"] = res["area"]["median_ms"] * 1e6 / subs
    res["unfiltered"]["ns_per_frame_pixel"] = res["unfiltered"]["median_ms"] * 1e6 / under
    res["area"]["ns_per_frame_pixel"] = res["area"]["median_ms"] * 1e6 / under
    res["area"]["bytes_tensor_once"] = ROWS * 3 * size * size * 2
    res["area"]["bytes_taps_requested_estimate"] = int(subs * 4 * (3 * 2 + 1))
    res["area"]["bytes_frame_read_estimate"] = res["area"]["bytes_frame_written_estimate"] = int(3 * under)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_area_timing.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    runs = []
    for size, per_frame in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), str(per_frame)], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the child for crop %d, %d per frame failed with status %d" % (size, per_frame, r.returncode))
        e = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        runs.append(e)
        print("crop %3d, %2d per frame: unfiltered %8.3f ms  area %8.3f ms  ratio %6.2f  mean S %.2f  mean S^2 %.1f  %.3f ns per sub-sample" %
              (size, per_frame, e["unfiltered"]["median_ms"], e["area"]["median_ms"], e["area_over_unfiltered"], e["S_mean"], e["S2_mean"],
               e["area"]["ns_per_sub_sample"]), flush=True)
    doc = {"tensor": "C x C x 3 float16 NCHW RGB, mean / std, feathered opacity map", "frames": "BGR 1920 x 1080, in place",
           "crop_width_in_frame": "64 ... 200 pixels", "rows": ROWS,
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call",
           "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
