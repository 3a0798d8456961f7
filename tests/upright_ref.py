"""Host restatement of upright-normalised detect and tracking (include/sdm.h, "Rolled faces"; csrc/sdm_upright.hip), in the device's
arithmetic: the rotation in double, the matrices rounded to float32, points in float32 with every operation rounded.

  roll_cs(roll_deg)                    (c, s) in double of a roll in degrees (a float32), exact at multiples of 90
  matrices(c, s, ix, iy, chip)         M (chip -> frame) and W (frame -> chip), 2 x 3 float32 each
  points(A, rows)                      landmark rows (n x 2L) through the row's matrix A (n x 2 x 3, or one 2 x 3)
  back(M, rows)                        = points(M, rows): chip coordinates -> frame coordinates
  roll_from_eyes(row, re, le)          (c, s) of a tracked row's eye line
  centre_of(row)                       (ix, iy) of a tracked row: the centre of its enclosing box, floored
  chip_box(box, chip)                  the box of the face inside its chip: (hc - w / 2, hc - h / 2, w, h)
  detect_setup(boxes, rolls, chip)     per row: M, W, the chip boxes
  chips(frame, M, chip)                align_ref.warp(frame, M, chip, chip)
  track_init(prev, W, mean)            track_ref.realign of W p
  near_edge(q, chip, guard)            the NEAR_EDGE rule on chip-coordinate rows
  flags(M, q, chip, guard, W, H)       PARTIAL | NEAR_EDGE per row
"""
import numpy as np

import align_ref
import track_ref

PARTIAL, NEAR_EDGE = 1, 2
f32 = np.float32


def roll_cs(roll_deg):
    d = float(f32(roll_deg))
    q = d / 90.0
    if q == np.floor(q):
        k = int(q % 4)
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[k]
    a = d * np.pi / 180.0
    return float(np.cos(a)), float(np.sin(a))


def matrices(c, s, ix, iy, chip):
    hc = float(chip // 2)
    c, s, ix, iy = float(c), float(s), float(ix), float(iy)
    M = np.array([[c, -s, ix - (c * hc - s * hc)], [s, c, iy - (s * hc + c * hc)]], np.float64).astype(f32)
    W = np.array([[c, s, hc - (c * ix + s * iy)], [-s, c, hc - (c * iy - s * ix)]], np.float64).astype(f32)
    return M, W


def points(A, rows):
    rows = np.atleast_2d(np.asarray(rows, f32))
    A = np.asarray(A, f32)
    if A.ndim == 2:
        A = np.broadcast_to(A, (rows.shape[0], 2, 3))
    L = rows.shape[1] // 2
    x, y = rows[:, :L], rows[:, L:]
    out = np.empty_like(rows)
    out[:, :L] = (A[:, 0, 0, None] * x + A[:, 0, 1, None] * y) + A[:, 0, 2, None]
    out[:, L:] = (A[:, 1, 0, None] * x + A[:, 1, 1, None] * y) + A[:, 1, 2, None]
    return out


back = points


def roll_from_eyes(row, right_eye, left_eye):
    row = np.asarray(row, f32).reshape(-1)
    L = row.size // 2
    c = []
    for eye in (right_eye, left_eye):
        sx, sy = f32(0), f32(0)
        for i in eye:
            sx, sy = f32(sx + row[i]), f32(sy + row[L + i])
        c.append((f32(sx / f32(len(eye))), f32(sy / f32(len(eye)))))
    dx, dy = float(f32(c[1][0] - c[0][0])), float(f32(c[1][1] - c[0][1]))
    n = np.sqrt(dx * dx + dy * dy)
    if n == 0.0 or not np.isfinite(n):
        return 1.0, 0.0
    return dx / n, dy / n


def centre_of(row):
    row = np.asarray(row, f32).reshape(-1)
    L = row.size // 2
    lim = f32(2.0 ** 20)
    out = []
    for v in (row[:L], row[L:]):
        m = f32(f32(v.min() + v.max()) * f32(0.5))
        out.append(int(np.floor(min(max(m, -lim), lim))))
    return tuple(out)


def chip_box(box, chip):
    x, y, w, h = (int(v) for v in box)
    hc = chip // 2
    return (hc - w // 2, hc - h // 2, w, h)


def detect_setup(boxes, rolls, chip):
    boxes = np.asarray(boxes).reshape(-1, 4)
    rolls = np.broadcast_to(np.asarray(rolls, f32).reshape(-1), (boxes.shape[0],))
    Ms, Ws, cb = [], [], []
    for b, r in zip(boxes, rolls):
        x, y, w, h = (int(v) for v in b)
        c, s = roll_cs(r)
        M, W = matrices(c, s, x + w // 2, y + h // 2, chip)
        Ms.append(M)
        Ws.append(W)
        cb.append(chip_box(b, chip))
    return np.stack(Ms), np.stack(Ws), np.array(cb, np.int32)


def track_setup(prev, right_eye, left_eye, chip):
    prev = np.atleast_2d(np.asarray(prev, f32))
    Ms, Ws = [], []
    for row in prev:
        c, s = roll_from_eyes(row, right_eye, left_eye)
        ix, iy = centre_of(row)
        M, W = matrices(c, s, ix, iy, chip)
        Ms.append(M)
        Ws.append(W)
    return np.stack(Ms), np.stack(Ws)


def chips(frame, M, chip):
    return align_ref.warp(frame, M, chip, chip)


def track_init(prev, W, mean):
    return track_ref.realign(points(W, prev), mean)


def near_edge(q, chip, guard):
    q = np.atleast_2d(np.asarray(q, f32))
    L = q.shape[1] // 2
    g, hi = f32(guard), f32(chip - 1)
    with np.errstate(invalid="ignore"):
        ok = (q[:, :L] >= g) & (q[:, L:] >= g) & (hi - q[:, :L] >= g) & (hi - q[:, L:] >= g)
    return ~ok.all(1)


def flags(M, q, chip, guard, width, height):
    q = np.atleast_2d(q)
    n = q.shape[0]
    Wd, Hd = np.broadcast_to(np.asarray(width), (n,)), np.broadcast_to(np.asarray(height), (n,))
    out = np.zeros(n, np.int32)
    ne = near_edge(q, chip, guard)
    for r in range(n):
        if align_ref.partial(M[r], chip, chip, int(Wd[r]), int(Hd[r])):
            out[r] |= PARTIAL
        if ne[r]:
            out[r] |= NEAR_EDGE
    return out
