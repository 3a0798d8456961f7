"""Rolled synthetic faces for the upright path's tests: the ground truth of synth's recipe (align_mean(mean, box) + jitter), rotated
about the integer box centre (x + w // 2, y + h // 2) and drawn with synth's background and blobs.  Positive roll is clockwise on
screen (x right, y down): p' = R (p - centre) + centre, R = [[cos, -sin], [sin, cos]].

  rotate(gt68, boxes, roll_deg)                    the rotated ground truth
  make_rolled_faces(n, roll_deg, seed, size, ...)  (images, boxes, gt68 rotated): the same faces for the same seed whatever the roll
  make_rolled_tracks(S, T, step_deg, seed, size)   video whose faces turn by step_deg per frame: (frames T x S, gt68, boxes, rolls)
  ragged_frames(), ROLLS, IDX, BOXES               five device frames of different sizes and formats and twelve rolled rows over them
"""
import numpy as np

from superviseddescent_amd import ibug, synth


def rotate(gt68, boxes, roll_deg):
    gt68 = np.atleast_2d(np.asarray(gt68, np.float64))
    boxes = np.asarray(boxes).reshape(-1, 4)
    roll = np.broadcast_to(np.asarray(roll_deg, np.float64).reshape(-1), (gt68.shape[0],))
    L = gt68.shape[1] // 2
    cx = (boxes[:, 0] + boxes[:, 2] // 2)[:, None].astype(np.float64)
    cy = (boxes[:, 1] + boxes[:, 3] // 2)[:, None].astype(np.float64)
    c, s = np.cos(np.deg2rad(roll))[:, None], np.sin(np.deg2rad(roll))[:, None]
    x, y = gt68[:, :L] - cx, gt68[:, L:] - cy
    return np.concatenate([c * x - s * y + cx, s * x + c * y + cy], 1).astype(np.float32)


def _boxes(rng, n, size, lo, hi, jitter):
    wh = rng.integers(lo, hi + 1, size=n)
    bx = (size - wh) // 2 + rng.integers(-jitter, jitter + 1, size=n)
    by = (size - wh) // 2 + rng.integers(-jitter, jitter + 1, size=n)
    return np.stack([bx, by, wh, wh], 1).astype(np.int32)


def _scene(rng, n, size):
    gcx = rng.random((n, 6)).astype(np.float32) * size
    gcy = rng.random((n, 6)).astype(np.float32) * size
    gsig = (12 + 28 * rng.random((n, 6))).astype(np.float32)
    gamp = (48 * (2 * rng.random((n, 6)) - 1)).astype(np.float32)
    return synth._background(gcx, gcy, gsig, gamp, size)


def make_rolled_faces(n, roll_deg, seed, size=320, box=(150, 190), jitter=6):
    """n faces in size x size images, boxes of box[0] .. box[1] pixels centred +- jitter, each rolled by roll_deg (a scalar or n
    angles) about its box centre.  The boxes, shapes, backgrounds and noise depend on the seed alone."""
    rng = np.random.default_rng(seed)
    boxes = _boxes(rng, n, size, box[0], box[1], jitter)
    field = _scene(rng, n, size)
    gt = np.stack([synth.align_mean(ibug.MEAN_IBUG_LFPW_68, b) for b in boxes])
    gt = gt + (1.5 * rng.standard_normal((n, 136))).astype(np.float32)
    gt = rotate(gt, boxes, roll_deg)
    return synth._draw_faces(rng, field, gt, size), boxes, gt


def make_rolled_tracks(n_streams, n_frames, step_deg, seed, size=320, box=(150, 190), jitter=6, roll0=0.0):
    """Video of n_streams faces that stay in place and turn by step_deg per frame from roll0, fresh noise every frame.  Returns
    (frames uint8 [T, S, size, size], gt68 float32 [T, S, 136], boxes int32 [S, 4], rolls float64 [T])."""
    rng = np.random.default_rng(seed)
    boxes = _boxes(rng, n_streams, size, box[0], box[1], jitter)
    background = _scene(rng, n_streams, size)
    shape = np.clip(1.5 * rng.standard_normal((n_streams, 136)), -4.5, 4.5).astype(np.float32)
    upright = np.stack([synth.align_mean(ibug.MEAN_IBUG_LFPW_68, b) for b in boxes]) + shape
    rolls = roll0 + step_deg * np.arange(n_frames)
    frames = np.empty((n_frames, n_streams, size, size), np.uint8)
    gt = np.empty((n_frames, n_streams, 136), np.float32)
    for t in range(n_frames):
        gt[t] = rotate(upright, boxes, rolls[t])
        frames[t] = synth._draw_faces(rng, background.copy(), gt[t], size)
    return frames, gt, boxes, rolls


def ragged_frames():
    """five frames of different sizes on the device -- gray, a pitched odd-aligned view, gray, BGR, NV12 -- and their gray host copies
    (the colour frame's is None: the context's conversion is read back)"""
    import torch
    rng = np.random.default_rng(99)
    g0 = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    wide = rng.integers(0, 256, (131, 128), dtype=np.uint8)
    g2 = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    bgr = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    nv = rng.integers(0, 256, (75, 72), dtype=np.uint8)                # 70 x 50 luma rows of 72 bytes, 25 chroma rows behind
    keep = [torch.from_numpy(a).cuda() for a in (g0, wide, g2, bgr, nv)]
    frames = [keep[0], keep[1][:, 5:102], keep[2], keep[3], (keep[4].data_ptr(), 70, 50, 72, "nv12")]
    grays = [g0, np.ascontiguousarray(wide[:, 5:102]), g2, None, np.ascontiguousarray(nv[:50, :70])]
    return frames, grays, keep


ROLLS = np.array([0, 0, 90, 180, -90, 17.3, -33, 45, 135, -150, 271, 360.5], np.float32)
IDX = np.array([0, 0, 0, 1, 1, 1, 2, 3, 3, 4, 4, 2], np.int32)
# boxes of 30 ... 70 pixels; rows 2, 5 and 8 hang over a frame edge, row 11 lies wholly outside its frame
BOXES = np.array([[40, 30, 50, 50], [80, 40, 70, 60], [130, 80, 60, 55], [20, 40, 45, 45], [30, 60, 40, 50], [-20, 10, 50, 64],
                  [10, 12, 40, 40], [20, 5, 36, 36], [50, 30, 44, 30], [15, 8, 30, 30], [25, 10, 33, 35], [100, -90, 40, 40]], np.int32)
