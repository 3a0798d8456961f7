"""Time of the piecewise-affine paste (Context.warp_paste_tensor, csrc/sdm_warp_paste.hip) beside the rigid paste
(Context.align_paste_tensor, csrc/sdm_align_paste.hip) on the same rows in the same process: 256 and 4 096 rows of 112 x 112
float16 NCHW RGB with mean / std, the RCR-22 Delaunay mesh, BGR frames of 1920 x 1080 resident on the device and used in place, the
face's crop 100 to 600 frame pixels wide (+-20 degrees, wholly inside the frame), with
  one     one face per frame (as many frames as rows)
  sixteen 16 faces per frame (rows / 16 frames; the faces overlap where they fall on each other)
Every case runs in a child process of its own under its own time limit, one after the other; the first that fails ends the run.  The
context runs on a torch stream; a call is bracketed by two HIP events on that stream (the call ends in the library's own synchronise),
5 warm-up calls, then CALLS calls: the median and the spread (max - min) of the event times, and the host clock's median beside them.
Pixels written: counted, not estimated -- a tensor that decodes to 255 everywhere is pasted without a map into zeroed frames, and the
frame pixels that are no longer 0 are the pixels either paste stores to (an opacity above 0 blends 255 into 0 as at least 1).  The
mesh's hull covers about 28 % of its crop, so the two pastes are compared by time per pixel written.  Writes
profiles/warp_paste_timing.json (or --out)."""
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
    n_frames = rows // per_frame
    store = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    frames = [(store[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)]
    ctx.set_frames_device(frames)
    ctx.set_sample_image_index(np.arange(rows) // per_frame)
    # the rows: the rigid crop's default template seen through a similarity of scale 100 / 112 ... 600 / 112, the crop wholly inside the frame
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
    res = {"device": torch.cuda.get_device_name(0), "rows": rows, "faces_per_frame": per_frame, "frames": n_frames}
    # the Context's calls are timed, the mesh set once: detection_model.paste_warped_tensor sets the mesh again in every call (a label map
    # on the host), which is no part of the kernels' time
    idx = np.arange(L)
    rigid_tmpl = alignment_template(model.mean, idx, SIZE, SIZE, 0.2)
    norm = dict(mean=MEAN, std=STD)
    model.warped_crops_tensor(SIZE, frames=frames, out=out, **norm)
    res["warp_paste"] = timed(torch, stream, lambda: ctx.warp_paste_tensor(out, frames, **norm))
    _, f1 = ctx.warp_paste_tensor(out, frames, **norm)
    res["triangles"] = int(ctx.warp_mesh[0])
    model.aligned_crops_tensor(SIZE, frames=frames, out=out, **norm)
    res["rigid_paste"] = timed(torch, stream, lambda: ctx.align_paste_tensor(idx, rigid_tmpl, out, frames, **norm))
    _, f2 = ctx.align_paste_tensor(idx, rigid_tmpl, out, frames, **norm)
    res["rows_flagged"] = int((f1 != 0).sum() + (f2 != 0).sum())
    # the pixels each paste stores to: 255 everywhere into zeroed frames
    out.fill_(255.0)
    for name, call in (("warp_paste", lambda: ctx.warp_paste_tensor(out, frames)), ("rigid_paste", lambda: ctx.align_paste_tensor(idx, rigid_tmpl, out, frames))):
        store.zero_()
        torch.cuda.synchronize()
        call()
        n = 0
        for i in range(0, n_frames, 64):                       # (in slices: no second copy of the frames)
            n += int((store[i:i + 64] != 0).any(-1).sum().item())
        res[name]["pixels_written"] = n
        res[name]["ns_per_pixel"] = res[name]["median_ms"] * 1e6 / max(n, 1)
    res["warp_over_rigid_per_call"] = res["warp_paste"]["median_ms"] / res["rigid_paste"]["median_ms"]
    res["warp_over_rigid_per_pixel"] = res["warp_paste"]["ns_per_pixel"] / res["rigid_paste"]["ns_per_pixel"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_paste_timing.json"))
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
        print("%5d rows, %2d per frame: warp paste %8.3f ms, %9d px, %6.3f ns/px   rigid paste %8.3f ms, %9d px, %6.3f ns/px   ratio per pixel %.2f" %
              (rows, per_frame, e["warp_paste"]["median_ms"], e["warp_paste"]["pixels_written"], e["warp_paste"]["ns_per_pixel"],
               e["rigid_paste"]["median_ms"], e["rigid_paste"]["pixels_written"], e["rigid_paste"]["ns_per_pixel"], e["warp_over_rigid_per_pixel"]),
              flush=True)
    doc = {"tensor": "112 x 112 x 3 float16 NCHW RGB, mean / std", "mesh": "RCR-22, Delaunay", "frames": "BGR 1920 x 1080, in place",
           "crop_width_in_frame": "100 ... 600 pixels",
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call",
           "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
