"""Time of the piecewise-affine paste into NV12 frames (Context.warp_paste_tensor on "nv12" destinations, csrc/sdm_warp_paste.hip:
warp_paste_kernel_t<true, false>) beside the unchanged warp_paste_kernel_t<false, false> on BGR frames of the same size and rows, in the same process: the faces
and settings of scripts/warp_paste_timing.py -- 256 and 4 096 rows of 112 x 112 float16 NCHW RGB with mean / std, the RCR-22 Delaunay
mesh, frames of 1920 x 1080 resident on the device and written in place, the face's crop 100 to 600 frame pixels wide (+-20 degrees,
wholly inside the frame), one face per frame or 16 faces per frame (the faces overlap where they fall on each other).  The BGR frames are
the context's images; the NV12 frames (the UV plane behind Y) have their size.  Every case runs in a child process of its own under its
own time limit, one after the other; the first that fails ends the run.  The context runs on a torch stream; a call is bracketed by two
HIP events on that stream (the call ends in the library's own synchronise), 5 warm-up calls, then CALLS calls: the median and the spread
(max - min) of the event times, and the host clock's median beside them; both forms a second time in turn (the spread between repeats).
Luma pixels written: counted, not estimated, as scripts/warp_paste_timing.py counts them -- a tensor that decodes to 255 everywhere
pasted without a map into zeroed planes.  Beside each BGR figure stands the figure of profiles/warp_paste_timing.json for the same case
(--reference), which shows whether the session is comparable.  A record with no threshold.  Writes
profiles/warp_paste_nv12_timing.json (or --out)."""
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


def child(rows, per_frame, fmt="nv12"):
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
    nv12 = torch.empty((n_frames, H + H // 2, W), dtype=torch.uint8, device="cuda").random_(0, 256)        # the UV plane behind Y
    frames = [(store[i].data_ptr(), W, H, W * 3, "bgr") for i in range(n_frames)]
    f_nv12 = [(nv12[i].data_ptr(), W, H, W, fmt) for i in range(n_frames)]
    ctx.set_frames_device(frames)
    ctx.set_sample_image_index(np.arange(rows) // per_frame)
    # the rows of scripts/warp_paste_timing.py: the same generator, the same draws
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
    norm = dict(mean=MEAN, std=STD)
    model.warped_crops_tensor(SIZE, frames=frames, out=out, **norm)          # (sets the mesh, once)
    res["triangles"] = int(ctx.warp_mesh[0])
    res["bgr"] = timed(torch, stream, lambda: ctx.warp_paste_tensor(out, frames, **norm))
    res["nv12"] = timed(torch, stream, lambda: ctx.warp_paste_tensor(out, f_nv12, **norm))
    res["bgr_again"] = timed(torch, stream, lambda: ctx.warp_paste_tensor(out, frames, **norm))
    res["nv12_again"] = timed(torch, stream, lambda: ctx.warp_paste_tensor(out, f_nv12, **norm))
    _, f1 = ctx.warp_paste_tensor(out, frames, **norm)
    _, f2 = ctx.warp_paste_tensor(out, f_nv12, **norm)
    res["rows_flagged"] = int((f1 != 0).sum() + (f2 != 0).sum())
    # the pixels each form stores to: 255 everywhere into zeroed planes
    out.fill_(255.0)
    store.zero_()
    nv12.zero_()
    torch.cuda.synchronize()
    ctx.warp_paste_tensor(out, frames)
    ctx.warp_paste_tensor(out, f_nv12)
    n_bgr = n_luma = n_chroma = 0
    for i in range(0, n_frames, 64):                           # (in slices: no second copy of the frames)
        n_bgr += int((store[i:i + 64] != 0).any(-1).sum().item())
        n_luma += int((nv12[i:i + 64, :H] != 0).sum().item())
        n_chroma += int((nv12[i:i + 64, H:].reshape(-1, H // 2, W // 2, 2) != 0).any(-1).sum().item())
    res["bgr"]["pixels_written"], res["nv12"]["pixels_written"], res["nv12"]["chroma_samples_written"] = n_bgr, n_luma, n_chroma
    for name in ("bgr", "nv12"):
        res[name]["ns_per_pixel"] = res[name]["median_ms"] * 1e6 / max(res[name]["pixels_written"], 1)
    res["nv12_over_bgr"] = res["nv12"]["median_ms"] / res["bgr"]["median_ms"]
    res["nv12_over_bgr_again"] = res["nv12_again"]["median_ms"] / res["bgr_again"]["median_ms"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_paste_nv12_timing.json"))
    ap.add_argument("--reference", default=os.path.join(ROOT, "profiles", "warp_paste_timing.json"))
    ap.add_argument("--format", default="nv12", help='the NV12 destinations\' name: "nv12" (value 5), "nv12:bt709", "nv12:bt2020:full", ...')
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.format)
    recorded = {}
    if os.path.exists(a.reference):
        recorded = {(r["rows"], r["faces_per_frame"]): r["warp_paste"]["median_ms"] for r in json.load(open(a.reference))["runs"]}
    runs = []
    for rows, per_frame in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--format", a.format, "--child", str(rows), str(per_frame)], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the child for %d rows, %d per frame failed with status %d" % (rows, per_frame, r.returncode))
        e = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        e["bgr_recorded_median_ms"] = recorded.get((rows, per_frame))
        runs.append(e)
        print("%5d rows, %2d per frame: BGR %8.3f ms (recorded %s)  NV12 %8.3f ms  ratio %.2f (again %.2f)  %9d / %9d px  %6.3f / %6.3f ns/px" %
              (rows, per_frame, e["bgr"]["median_ms"], e["bgr_recorded_median_ms"], e["nv12"]["median_ms"], e["nv12_over_bgr"],
               e["nv12_over_bgr_again"], e["bgr"]["pixels_written"], e["nv12"]["pixels_written"], e["bgr"]["ns_per_pixel"],
               e["nv12"]["ns_per_pixel"]), flush=True)
    doc = {"tensor": "112 x 112 x 3 float16 NCHW RGB, mean / std", "mesh": "RCR-22, Delaunay",
           "frames": "1920 x 1080, BGR and NV12 (UV behind Y), in place", "crop_width_in_frame": "100 ... 600 pixels",
           "unit": "ms per call between two HIP events on the context's stream; host_median_ms: the host clock around the same call",
           "bgr_recorded_median_ms": "warp_paste of " + os.path.basename(a.reference) + " for the same case", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
