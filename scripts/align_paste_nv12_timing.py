"""Time of the paste into NV12 frames (Context.align_paste_tensor_at on "nv12" destinations, csrc/sdm_align_paste.hip: paste_kernel_t<true, AREA>)
beside the paste of the same rows into BGR frames of the same size through the existing calls (sdm_align_paste_tensor_at and
sdm_align_paste_tensor_at_filtered: paste_kernel_t<false, AREA>, the yardstick) in the same session.  Rows of C x C float16 NCHW
RGB with mean / std and a feathered opacity map, frames of 1920 x 1080 resident on the device and written in place, +-20 degrees, wholly
inside the frame:
  bilinear   C = 112, the crop 100 to 600 frame pixels wide (the configuration of scripts/align_paste_timing.py)
  area       C = 256, the crop 64 to 200 frame pixels wide, filter "area": S spans 2 to 4 (scripts/align_paste_area_timing.py's)
with one face per frame or 16 faces per frame (the faces overlap where they fall on each other).  Every case runs in a child process of
its own under its own time limit, one after the other; the first that fails ends the run.  The context runs on a torch stream; a call is
bracketed by two HIP events on that stream (the call ends in the library's own synchronise), 5 warm-up calls, then CALLS calls: the median
and the spread (max - min) of the event times, and the host clock's median beside them.  Per case: both times, their ratio, ns per frame
pixel under a crop, both forms a second time in turn (the spread between repeats), and the frame bytes each form moves per such pixel (BGR: 3 read + 3 written; NV12: 1.5 + 1.5).
Writes profiles/align_paste_nv12_timing.json (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, W, H = 25, 1920, 1080
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
# (rows, faces per frame, crop size, narrowest and widest crop in the frame, filter)
CASES = [(256, 1, 112, 100, 600, "none"), (256, 16, 112, 100, 600, "none"), (4096, 16, 112, 100, 600, "none"),
         (256, 1, 256, 64, 200, "area"), (256, 16, 256, 64, 200, "area")]


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


def child(rows, per_frame, size, lo, hi, filt, fmt="nv12"):
    sys.path.insert(0, ROOT)
    import torch
    from superviseddescent_amd import Context, feather_mask
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(7)
    n_frames = rows // per_frame
    bgr = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    nv12 = torch.empty((n_frames, H + H // 2, W), dtype=torch.uint8, device="cuda").random_(0, 256)       # the UV plane behind Y
    f_bgr = [(bgr[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)]
    f_nv12 = [(nv12[i].data_ptr(), W, H, W, fmt) for i in range(n_frames)]
    index = np.arange(rows) // per_frame
    width = rng.uniform(float(lo), float(hi), rows)
    s = width / size
    ang = np.deg2rad(rng.uniform(-20, 20, rows))
    c, sn = s * np.cos(ang), s * np.sin(ang)
    half = 0.5 * size * s * (np.abs(np.cos(ang)) + np.abs(np.sin(ang))) + 2
    centre = np.stack([rng.uniform(half, W - 1 - half), rng.uniform(half, H - 1 - half)], 1)
    mid = (size - 1) / 2
    mats = np.zeros((rows, 2, 3), np.float32)
    mats[:, 0] = np.stack([c, -sn, centre[:, 0] - (c - sn) * mid], 1)
    mats[:, 1] = np.stack([sn, c, centre[:, 1] - (sn + c) * mid], 1)
    y = torch.empty((rows, 3, size, size), dtype=torch.float16, device="cuda").normal_(0, 1)
    mask = torch.from_numpy(feather_mask(size, max(8, size // 14))).cuda()
    kw = dict(image_index=index, mask=mask, mean=MEAN, std=STD)
    if filt == "area":
        kw["filter"] = "area"
    res = {"device": torch.cuda.get_device_name(0), "rows": rows, "faces_per_frame": per_frame, "frames": n_frames, "crop": size,
           "crop_width_in_frame": [lo, hi], "filter": filt, "format": fmt}
    res["bgr"] = timed(torch, stream, lambda: ctx.align_paste_tensor_at(mats, y, f_bgr, **kw))
    res["nv12"] = timed(torch, stream, lambda: ctx.align_paste_tensor_at(mats, y, f_nv12, **kw))
    res["bgr_again"] = timed(torch, stream, lambda: ctx.align_paste_tensor_at(mats, y, f_bgr, **kw))       # the two forms in turn: the
    res["nv12_again"] = timed(torch, stream, lambda: ctx.align_paste_tensor_at(mats, y, f_nv12, **kw))     # repeats show the spread
    got = ctx.align_paste_tensor_at(mats, y, f_nv12, **kw)
    flags, S = (got, np.ones(rows, np.int32)) if filt != "area" else got
    res["rows_flagged"] = int((flags != 0).sum())
    res["S_min"], res["S_max"], res["S_mean"] = int(S.min()), int(S.max()), float(S.mean())
    under = float((width ** 2).sum())                                        # frame pixels under the crops (overlaps counted twice)
    res["frame_pixels_under_crops"] = int(under)
    for name, per_pixel in (("bgr", 3.0), ("nv12", 1.5)):
        res[name]["ns_per_frame_pixel"] = res[name]["median_ms"] * 1e6 / under
        res[name]["bytes_frame_read_estimate"] = res[name]["bytes_frame_written_estimate"] = int(per_pixel * under)
    res["nv12_over_bgr"] = res["nv12"]["median_ms"] / res["bgr"]["median_ms"]
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_paste_nv12_timing.json"))
    ap.add_argument("--format", default="nv12", help='the NV12 destinations\' name: "nv12" (value 5), "nv12:bt709", "nv12:bt2020:full", ...')
    ap.add_argument("--child", nargs=6, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*[int(v) for v in a.child[:5]], a.child[5], a.format)
    runs = []
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--format", a.format, "--child"] + [str(v) for v in case], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the child for %s failed with status %d" % (case, r.returncode))
        e = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        runs.append(e)
        print("%5d rows, %2d per frame, crop %3d, %s: BGR %8.3f ms  NV12 %8.3f ms  ratio %.2f  (%.3f / %.3f ns per frame pixel)" %
              (e["rows"], e["faces_per_frame"], e["crop"], e["filter"], e["bgr"]["median_ms"], e["nv12"]["median_ms"], e["nv12_over_bgr"],
               e["bgr"]["ns_per_frame_pixel"], e["nv12"]["ns_per_frame_pixel"]), flush=True)
    doc = {"format": a.format, "tensor": "C x C x 3 float16 NCHW RGB, mean / std, feathered opacity map", "frames": "1920 x 1080, BGR and NV12 (UV behind Y), in place",
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call",
           "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
