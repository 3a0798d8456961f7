"""Time of the regulariser sweep (Context.train_level_sweep; csrc/sdm_capi_sweep.hip) against the existing path, RCR-22 at the shipped
parameters (level 0 of ibug.SHIPPED_HOG_PARAMS, Regulariser(MatrixNorm, 1.5 x 2^j), regularise_last_row off): 100 000 fit rows plus
10 000 held out, K = 1, 4 and 8 candidates, three repetitions each, all in one run:
  * existing path: on a context holding the 100 000 fit rows, features once, then K x (gram_rhs + solve) -- what trying K values costs
    today without extracting the features again; t_solve = its REG + FACTOR stage time per pass (sdm_get_timing);
  * sweep: the wall time of one train_level_sweep call (features, one Gram product, snapshot, K passes, scoring, install + apply)
    and its per-stage times.
The aim DESIGN.md 4.10 states: t_sweep(K) - t_sweep(1) <= 1.2 x (K - 1) x t_solve.  Writes profiles/sweep_timing.json (or --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superviseddescent_amd import Context, HoGParam, ibug, synth  # noqa: E402

IDS = ibug.RCR22_IDS
N_FIT, N_HOLD = 100000, 10000
KS = (1, 4, 8)
REPS = 3
MATRIX_NORM = 1


def candidates(K):
    return [1.5 * 2.0 ** (j - K // 2) for j in range(K)]


def make_ctx(images, idx, x0, x_star, rows):
    ctx = Context(0)
    ctx.set_model_geometry(len(IDS), *ibug.eye_indices(IDS), [HoGParam(*ibug.SHIPPED_HOG_PARAMS[0])])
    ctx.upload_images(images)
    ctx.set_sample_image_index(idx[:rows])
    ctx.set_x(x0[:rows])
    ctx.set_targets(x_star[:rows])
    ctx.enable_timing(True)
    return ctx


def stages(ctx):
    return {k: round(v[0], 4) for k, v in ctx.get_timing(reset=True).items() if v[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_timing.json"))
    ap.add_argument("--images", type=int, default=2200)          # x 50 rows each = 110 000
    a = ap.parse_args()
    import torch
    per = (N_FIT + N_HOLD) // a.images
    images, boxes, gt = synth.make_faces(a.images, seed=9200, chunk=32, workers=8)
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=per - 1, seed=9201)
    N = x0.shape[0]
    assert N == N_FIT + N_HOLD, N
    res = {"model": "RCR-22, level 0 of the shipped parameters", "fit_rows": N_FIT, "held_out_rows": N_HOLD, "unit": "ms",
           "device": torch.cuda.get_device_name(0), "repetitions": REPS, "K": {}}

    # ---- the existing path: K x (gram_rhs + solve) on the fit rows ----
    ctx = make_ctx(images, idx, x0, x_star, N_FIT)
    ctx.hog_features(0)
    ctx.gram_rhs(0); ctx.solve(0, MATRIX_NORM, 1.5, False, N_FIT, fetch=False)      # (warm-up: allocations, first launches)
    ctx.synchronize(); ctx.get_timing(reset=True)
    existing = {}
    for K in KS:
        runs = []
        for _ in range(REPS):
            ctx.synchronize()
            t0 = time.perf_counter()
            for p in candidates(K):
                ctx.gram_rhs(0)
                ctx.solve(0, MATRIX_NORM, p, False, N_FIT, fetch=False)
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            st = stages(ctx)
            runs.append({"wall": round(wall, 4), "stages": st, "t_solve": round((st.get("reg", 0.0) + st.get("factor_solve", 0.0)) / K, 4)})
        existing[K] = runs
    ctx.close()
    t_solve = float(np.median([r["t_solve"] for K in KS for r in existing[K]]))

    # ---- the sweep ----
    ctx = make_ctx(images, idx, x0, x_star, N)
    ctx.train_level_sweep(0, MATRIX_NORM, candidates(KS[-1]), False, N_FIT)        # (warm-up: the slots of the largest K, first launches)
    ctx.synchronize(); ctx.get_timing(reset=True)
    sweep = {}
    for K in KS:
        runs = []
        for _ in range(REPS):
            ctx.set_x(x0)
            ctx.synchronize()
            t0 = time.perf_counter()
            rec = ctx.train_level_sweep(0, MATRIX_NORM, candidates(K), False, N_FIT)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append({"wall": round(wall, 4), "stages": stages(ctx), "best": rec["best"],
                         "holdout_errors": [float(v) for v in rec["holdout_errors"]]})
        sweep[K] = runs
    ctx.close()

    t1 = float(np.median([r["wall"] for r in sweep[1]]))
    for K in KS:
        tK = float(np.median([r["wall"] for r in sweep[K]]))
        entry = {"candidates": candidates(K), "sweep": sweep[K], "existing_path": existing[K], "t_sweep_median": round(tK, 4),
                 "t_existing_median": round(float(np.median([r["wall"] for r in existing[K]])), 4)}
        if K > 1:
            entry["extra_per_candidate"] = round((tK - t1) / (K - 1), 4)
            entry["ratio_to_t_solve"] = round((tK - t1) / ((K - 1) * t_solve), 4)      # the aim: <= 1.2
        res["K"][str(K)] = entry
    res["t_solve_median"] = round(t_solve, 4)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
