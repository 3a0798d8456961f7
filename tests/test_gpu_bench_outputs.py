"""bench.py's plain run (the headline alone) against --full: the same seeded inputs and the same model, so --dump-outputs writes
the same landmarks bit for bit; the plain line carries the headline fields and none of the legs that moved behind --full.  The
dumped landmarks are also checked against the ground truth of the faces, regenerated here from the bench's seeds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# batch 300: not a whole number of 32-face chunks; --rcr68-shard 512: --full draws more faces than the plain run does
ARGS = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "300", "--train-rows", "4000", "--rcr68-shard", "512")


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out_dir), *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_full_run_computes(built, tmp_path):
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", "--full", "--no-cpu")
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k]
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert not {"train", "roofline", "rcr68_train", "sustained", "config3_train"} & set(plain)
    assert full["train"]["sec_per_cascade"] > 0 and full["rcr68_detect_shard"]["value"] > 0
    a = np.load(tmp_path / "plain" / "landmarks.npy")
    b = np.load(tmp_path / "full" / "landmarks.npy")
    assert a.dtype == np.float32 and a.shape == (300, 44) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the faces of the batch as bench.py makes them on one GPU (512 faces in all: one seeded stream, chunks of 32): the cascade
    # must have moved the initial landmarks towards the ground truth
    from superviseddescent_amd import ibug, synth
    _, boxes, gt = synth.make_faces(320, seed=synth.SEED, chunk=32)
    x_star, x0, _ = synth.make_samples(boxes[:300], gt[:300], ibug.RCR22_IDS, 0, seed=synth.SEED + 1)
    err0 = np.linalg.norm(x0 - x_star) / np.linalg.norm(x_star)
    err = np.linalg.norm(a - x_star) / np.linalg.norm(x_star)
    assert err < 0.5 * err0, (err0, err)          # (the CPU oracle with the same rows: 0.30)
