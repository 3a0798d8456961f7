"""Time of the filtered piecewise-affine paste (Context.warp_paste_tensor(filter=...), csrc/sdm_warp_paste.hip:
warp_paste_kernel_t<true, true> behind the counts stage) beside the unfiltered call on the same frames and rows, in the same process: DESIGN
4.18's shapes -- 256 rows of 256 x 256 float16 NCHW RGB with mean / std, the RCR-22 Delaunay mesh, frames of 1920 x 1080 resident on the
device and written in place, one face per frame or 16 faces per frame (the faces overlap where they fall on each other), the face's crop
60, 120 or 250 frame pixels wide (+-20 degrees, wholly inside the frame): a 256-pixel network's output going back onto a small, a medium
and a near-full-size face.  BGR frames (the context's images) and NV12 frames of their size (the UV plane behind Y).  Three legs per
format: the unfiltered call, the filtered call with mode "area" at max_samples 16, and the filtered call with mode "bilinear" -- which
writes the unfiltered bytes through the new kernel and so shows what the new path costs when it does nothing.  Every case runs in a child
process of its own under its own time limit, one after the other; the first that fails ends the run.  The context runs on a torch
stream; a call is bracketed by two HIP events on that stream (the call ends in the library's own synchronise), 5 warm-up calls, then CALLS
calls: the median and the spread (max - min) of the event times, and the host clock's median beside them.  A record with no threshold.
Writes profiles/warp_paste_area_timing.json (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, CALLS, W, H, ROWS = 256, 25, 1920, 1080, 256
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
CASES = [(per_frame, width) for per_frame in (1, 16) for width in (60, 120, 250)]
LEGS = [("unfiltered", {}), ("area", dict(filter="area", max_samples=16)), ("bilinear", dict(filter="bilinear"))]


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


def child(per_frame, width):
    sys.path.insert(0, ROOT)
    import torch
    from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, alignment_template, detection_model, ibug
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
    nv12 = torch.empty((n_frames, H + H // 2, W), dtype=torch.uint8, device="cuda").random_(0, 256)        # the UV plane behind Y
    lists = {"bgr": [(store[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)],
             "nv12": [(nv12[i].data_ptr(), W, H, W, "nv12") for i in range(n_frames)]}
    ctx.set_frames_device(lists["bgr"])
    ctx.set_sample_image_index(np.arange(ROWS) // per_frame)
    tmpl = alignment_template(model.mean, np.arange(L), SIZE, SIZE, 0.2).astype(np.float64)
    s = np.full(ROWS, width / SIZE)
    ang = np.deg2rad(rng.uniform(-20, 20, ROWS))
    c, sn = s * np.cos(ang), s * np.sin(ang)
    half = 0.5 * SIZE * s * (np.abs(np.cos(ang)) + np.abs(np.sin(ang))) + 2
    centre = np.stack([rng.uniform(half, W - 1 - half), rng.uniform(half, H - 1 - half)], 1)
    q = tmpl - (SIZE - 1) / 2
    x = np.zeros((ROWS, 2 * L), np.float32)
    x[:, :L] = c[:, None] * q[:, 0] - sn[:, None] * q[:, 1] + centre[:, :1]
    x[:, L:] = sn[:, None] * q[:, 0] + c[:, None] * q[:, 1] + centre[:, 1:]
    ctx.set_x(x)
    out = torch.empty((ROWS, 3, SIZE, SIZE), dtype=torch.float16, device="cuda")
    norm = dict(mean=MEAN, std=STD)
    model.warped_crops_tensor(SIZE, frames=lists["bgr"], out=out, **norm)     # (sets the mesh, once; the tensor: the faces themselves)
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "faces_per_frame": per_frame, "frames": n_frames, "face_width": width,
           "triangles": int(ctx.warp_mesh[0])}
    for fmt, lst in lists.items():
        res[fmt] = {name: timed(torch, stream, lambda: ctx.warp_paste_tensor(out, lst, **norm, **kw)) for name, kw in LEGS}
        samples = ctx.warp_paste_tensor(out, lst, filter="area", **norm)[2]
        res[fmt]["samples_min_max"] = [int(samples.min()), int(samples.max())]
        res[fmt]["area_over_unfiltered"] = res[fmt]["area"]["median_ms"] / res[fmt]["unfiltered"]["median_ms"]
        res[fmt]["bilinear_over_unfiltered"] = res[fmt]["bilinear"]["median_ms"] / res[fmt]["unfiltered"]["median_ms"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_paste_area_timing.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    runs = []
    for per_frame, width in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(per_frame), str(width)], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the child for %d per frame, %d pixels failed with status %d" % (per_frame, width, r.returncode))
        e = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        runs.append(e)
        for fmt in ("bgr", "nv12"):
            print("%2d per frame, %3d px, %-4s: unfiltered %7.3f ms  area %7.3f ms (x %.2f, counts %s)  bilinear %7.3f ms (x %.2f)" %
                  (per_frame, width, fmt, e[fmt]["unfiltered"]["median_ms"], e[fmt]["area"]["median_ms"], e[fmt]["area_over_unfiltered"],
                   e[fmt]["samples_min_max"], e[fmt]["bilinear"]["median_ms"], e[fmt]["bilinear_over_unfiltered"]), flush=True)
    doc = {"tensor": "256 x 256 x 3 float16 NCHW RGB, mean / std", "mesh": "RCR-22, Delaunay", "rows": ROWS,
           "frames": "1920 x 1080, BGR and NV12 (UV behind Y), in place", "crop_width_in_frame": "60, 120, 250 pixels",
           "legs": "unfiltered: sdm_warp_paste_tensor[_nv12]; area: sdm_warp_paste_tensor_filtered, max_samples 16; bilinear: the same call, mode BILINEAR",
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
