"""Time of the head-pose kernels (csrc/sdm_pose.hip) at N = 10^6 rows, measured with torch.cuda events on the stream the
context runs on: the fused 3-level cascade (sdm_pose_test: test / predict) and one training level (sdm_pose_train_level:
projection, normal equations, LU solve, update) for the example's K = 10 model and for K = 64.  Prints one JSON object."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_f64 as P  # noqa: E402
from superviseddescent_amd import Context, ModelProjection  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)
    out = {"n": n, "levels": 3, "unit": "us", "device": torch.cuda.get_device_name(0)}
    for K in (10, 64):
        pts = P.EXAMPLE_POINTS if K == 10 else rng.uniform(-60, 60, (K, 3)).astype(np.float32)
        proj = ModelProjection(np.concatenate([pts.T, np.ones((1, K), np.float32)]))
        xs = np.zeros((n, 6), np.float32)
        xs[:, :3] = rng.uniform(-30, 30, (n, 3))
        xs[:, 5] = -2000.0
        tmpl = proj(xs)
        x0 = np.tile(P.EXAMPLE_X0, (n, 1))
        ctx.pose_set_model(pts)
        ctx.pose_set_x(x0)
        ctx.pose_set_templates(tmpl)
        ctx.pose_set_targets(xs)
        for lvl in range(3):
            ctx.pose_train_level(lvl, 1, 2.0, True)
        ctx.pose_set_x(x0)
        train = timed(lambda: ctx.pose_train_level(0, 1, 2.0, True), 10)
        ctx.pose_set_x(x0)
        fused = timed(lambda: ctx.pose_test(0, 3), 50)
        level = timed(lambda: ctx.pose_test(0, 1), 50)
        hbm = n * (8 * K + 48)
        out[f"K{K}"] = {"cascade3_median_us": fused[0], "cascade3_min_us": fused[1], "cascade1_median_us": level[0],
                        "train_level_median_us": train[0], "train_level_min_us": train[1],
                        "cascade_hbm_bytes": hbm, "cascade3_GBps": hbm / fused[0] / 1e3}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
