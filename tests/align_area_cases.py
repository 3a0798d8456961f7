"""The rows that tests/test_gpu_align_area.py runs on the device and tests/test_align_area_host.py runs through the host build of the
kernel's per-pixel code, on the frame sets of tests/align_tensor_cases.py: similarities whose scales make S take 1, 2, 3, 5 and 16 (and the
capped and gated cases), rotated, with footprints that hang over the frames' edges; and the 1-pixel stripes."""
import numpy as np

import align_area_ref as R
import align_ref as A

L = 22                                  # landmarks per row (the RCR-22 model of the device tests)
LM = np.array([3, 6, 9, 12, 15])
# crop -> source scale of a class, well inside its S: (scale, S)
CLASSES = [(0.8, 1), (1.7, 2), (2.6, 3), (4.5, 5), (15.5, 16)]


def similarity(f, w, h, scale, rng):
    """a crop -> source similarity of that scale, +-45 degrees, the crop centre within 0.3 frame sizes of the frame centre (float64)"""
    S = A.similarity(scale, rng.uniform(-45, 45), 0, 0)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    S[:, 2] = np.array([(f["w"] - 1) / 2, (f["h"] - 1) / 2]) + rng.uniform(-0.3, 0.3, 2) * (f["w"], f["h"]) - S[:, :2] @ c
    return S


def variants(f, w, h, seed):
    """[(similarity, (mode, max_samples, min_scale), S)] for one frame: every class, the cap, the gate and mode BILINEAR"""
    rng = np.random.default_rng(seed)
    out = [(similarity(f, w, h, s, rng), (R.AREA, 16, 1.0), S) for s, S in CLASSES]
    out.append((similarity(f, w, h, 40.0, rng), (R.AREA, 16, 1.0), 16))                 # no S <= 16 reaches s2: the cap
    out.append((similarity(f, w, h, 7.0, rng), (R.AREA, 4, 1.0), 4))
    out.append((similarity(f, w, h, 1.7, rng), (R.AREA, 16, 2.0), 1))                   # below the gate
    out.append((similarity(f, w, h, 4.5, rng), (R.BILINEAR, 16, 1.0), 1))
    return out


def mixed_rows(frames, w, h, seed, per_call=10):
    """calls of `per_call` rows that together put every frame at every class, each call mixing all five classes:
    [(row -> frame index, similarities, S per row)]"""
    rng = np.random.default_rng(seed)
    n = len(frames)
    pairs = [(p % n, (p // n + p % n) % len(CLASSES)) for p in range(n * len(CLASSES))]
    calls = []
    for at in range(0, len(pairs), per_call):
        part = pairs[at:at + per_call]
        assert {c for _, c in part} == set(range(len(CLASSES)))
        calls.append(([im for im, _ in part], [similarity(frames[im], w, h, CLASSES[c][0], rng) for im, c in part],
                      [CLASSES[c][1] for _, c in part]))
    return calls


def stripes(scale):
    """(frame of 1-pixel vertical stripes 0, 255, 0, ..., one landmark row, template, crop width, height, the exact crop -> source matrix):
    the landmarks are scale * q_k + (tx, ty), all integers, the template's mean is an integer point and the scale a power of two, so every
    step of the double fit is exact.  Every sub-sample's footprint lies inside the frame."""
    w = h = 12
    tmpl = np.array([[2, 2], [9, 3], [6, 6], [3, 9], [10, 10]], np.float32)
    tx, ty = scale // 2 + 3, scale // 2 + 2
    frame = np.zeros((scale * h + ty + 8, scale * w + tx + 8), np.uint8)
    frame[:, 1::2] = 255
    x = np.zeros((1, 2 * L), np.float32)
    x[0, LM] = scale * tmpl[:, 0] + tx
    x[0, L + LM] = scale * tmpl[:, 1] + ty
    return frame, x, tmpl, w, h, np.array([[scale, 0, tx], [0, scale, ty]], np.float64)
