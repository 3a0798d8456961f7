"""The cases of the filtered paste (include/sdm.h, "Pasting crops back, filtered") that tests/test_align_paste_area_host.py runs through
the host build of the per-pixel code and tests/test_gpu_align_paste_area.py on the device: the frames, tensors and opacity maps of
tests/paste_cases.py, with crops that outsize the face -- matrices whose inverse W has a scale above 1."""
import itertools

import numpy as np

import align_ref as A
import paste_area_ref as Q
import paste_cases as C

f32 = np.float32
CROPS = [(16, 16), (33, 20), (64, 64)]
W_SCALES = [0.8, 1.7, 2.6, 4.5, 20.0]                     # crop pixels per frame pixel: S = 1, 2, 3, 5 and 16 (capped)
W_SAMPLES = [1, 2, 3, 5, 16]
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
# (mode, max_samples, min_scale): the default, a cap, a scale gate, plain bilinear
FILTERS = [(Q.AREA, 16, 1.0), (Q.AREA, 16, 1.0), (Q.AREA, 4, 1.0), (Q.AREA, 16, 2.0), (Q.BILINEAR, 16, 1.0)]


def minifying(f, cw, ch, seed, n=5, scales=W_SCALES):
    """n crop -> frame similarities for frame f: the W scales of ``scales`` in turn (mixed S on the one frame), +-45 degrees, the crop
    centre anywhere in the frame -- so rows lie partly outside"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        s, ang = scales[r % len(scales)], rng.uniform(-45.0, 45.0)
        R = A.similarity(1.0 / s, ang, 0.0, 0.0)[:, :2]
        target = np.array([rng.uniform(0, f["w"]), rng.uniform(0, f["h"])])
        t = target - R @ np.array([(cw - 1) / 2.0, (ch - 1) / 2.0])
        out.append(np.concatenate([R, t[:, None]], 1).astype(f32))
    return out


def special_matrices(f, cw, ch):
    """wholly outside the frame at W scale 2.6, a NaN, d == 0"""
    far = A.similarity(1.0 / 2.6, 30.0, f["w"] + 40.0, -ch - 40.0).astype(f32)
    return [far, np.array([[1, 0, np.nan], [0, 1, 0]], f32), np.array([[1, 2, 3], [2, 4, 1]], f32)]


def host_cases():
    """one frame with eight rows per case: three crop sizes x the seven frames of paste_cases.FRAMES x two passes; the dtypes, layouts,
    channel counts and orders in turn; no opacity map, one for all rows, one per row"""
    buf, frames = C.place(C.FRAMES, 5)
    cases = []
    for rep, (cw, ch), (i, f) in itertools.product(range(2), CROPS, enumerate(frames)):
        k = len(cases)
        dtype, layout, channels, order = COMBOS[(5 * k + rep) % len(COMBOS)]
        mats = minifying(f, cw, ch, 400 + k) + special_matrices(f, cw, ch)
        mode = k % 3
        x = C.tensor(len(mats), cw, ch, dtype, layout, channels, 500 + k)
        alpha = None if mode == 0 else C.alpha_maps(1 if mode == 1 else len(mats), cw, ch, 600 + k, zero_band=k % 2 == 1)
        cases.append(dict(f=f, cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14 + k % 2, mats=mats,
                          x=x, alpha=alpha, mode=mode, filter=FILTERS[k % len(FILTERS)],
                          frame=buf[f["off"]:f["off"] + C.owned_bytes(f)].copy()))
    return cases


def known_answer():
    """(M, crop 16 x 16 uint8, S, expected 8 x 8 x 3 BGR frame): W = [4 0 -6.5; 0 4 -2.5], so the sixteen sub-samples of frame pixel
    (X, Y) in [2, 5] x [1, 4] are exactly the crop pixels of one 4 x 4 block, and every other frame pixel's lie outside the crop"""
    M = np.array([[0.25, 0, 2 - 0.375], [0, 0.25, 1 - 0.375]], f32)
    crop = np.random.default_rng(9).integers(0, 256, (16, 16), dtype=np.uint8)
    want = np.zeros((8, 8, 3), np.uint8)
    blocks = (crop.astype(np.int64).reshape(4, 4, 4, 4).sum((1, 3)) + 8) // 16
    want[1:5, 2:6] = blocks[..., None]
    return M, crop, 4, want


def checkerboard(theta):
    """(M, crop 64 x 64 uint8: a 1-pixel 0 / 255 checkerboard, frame 40 x 40 x 3 of value 128, the interior 8 x 8 window): pasted at
    scale 0.27 and rotated by theta (radians).  Rotated, the crop's centre (31.5, 31.5) lies on the frame's (19.5, 19.5): the sampling
    grid meets the board at every phase, and the restatements give 112 (unfiltered) and 4 (area) in the window.  At theta = 0 the phase
    is the same in every row and column, and with centre on centre no window pixel comes nearer than 0.06 to a crop pixel centre: the
    unfiltered rule shows a swing of 98 only (area: 1).  There crop pixel (32, 32) lies on frame pixel (20, 20), so that a window pixel
    reads the board at a pixel centre, where plain bilinear sampling returns the full swing (unfiltered 128, area 2).  (That placement
    under theta = 0.3 gives 128 and 5.)"""
    j, i = np.meshgrid(np.arange(64), np.arange(64))
    crop = (((i + j) & 1) * 255).astype(np.uint8)
    c, s = 0.27 * np.cos(theta), 0.27 * np.sin(theta)
    R = np.array([[c, -s], [s, c]])
    t = np.array([20.0, 20.0]) - R @ np.array([32.0, 32.0]) if theta == 0 else np.array([19.5, 19.5]) - R @ np.array([31.5, 31.5])
    M = np.concatenate([R, t[:, None]], 1).astype(f32)
    return M, crop, np.full((40, 40, 3), 128, np.uint8), (slice(16, 24), slice(16, 24))
